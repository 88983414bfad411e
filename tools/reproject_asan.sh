#!/bin/sh
# vr_reproject_host under AddressSanitizer and UBSan, on the CPU: vanrijn_amd/csrc/vr_host_reproject.cpp alone (it
# has no device call) and tools/reproject_host_check.cpp (its own main) in one program.  No GPU is used, nothing
# is loaded into python, and the library need not be built.  The unit takes the camera rule from vr_camera.h,
# which includes the HIP runtime's header for its host / device markers: only that header is needed (ROCM_PATH,
# default /opt/rocm), nothing of HIP is linked.
#     sh tools/reproject_asan.sh [build directory]
set -eu
root=$(cd "$(dirname "$0")/.." && pwd)
out=${1:-$(mktemp -d)}
${CXX:-g++} -std=c++17 -O1 -g -ffp-contract=off -fno-omit-frame-pointer -fsanitize=address,undefined -Wall -I"${ROCM_PATH:-/opt/rocm}/include" -D__HIP_PLATFORM_AMD__ "$root/vanrijn_amd/csrc/vr_host_reproject.cpp" "$root/tools/reproject_host_check.cpp" -o "$out/reproject_host_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$out/reproject_host_check"
