#!/bin/sh
# vr_denoise_host under AddressSanitizer and UBSan, on the CPU: vanrijn_amd/csrc/vr_host_denoise.cpp alone (it has
# no device call) and tools/denoise_host_check.cpp (its own main) in one program.  No GPU is used, nothing is
# loaded into python, and the library need not be built.
#     sh tools/denoise_asan.sh [build directory]
set -eu
root=$(cd "$(dirname "$0")/.." && pwd)
out=${1:-$(mktemp -d)}
${CXX:-g++} -std=c++17 -O1 -g -ffp-contract=off -fno-omit-frame-pointer -fsanitize=address,undefined -Wall "$root/vanrijn_amd/csrc/vr_host_denoise.cpp" "$root/tools/denoise_host_check.cpp" -o "$out/denoise_host_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$out/denoise_host_check"
