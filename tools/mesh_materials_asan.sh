#!/bin/sh
# The host-only path of the per-triangle materials under AddressSanitizer and UBSan, on the CPU: the
# host translation units are compiled with -fsanitize=address,undefined and linked with
# tools/mesh_materials_check.cpp (its own main) into one program, whose sanitized definitions of the C
# ABI are the ones it calls.  The kernel launch wrappers (never called on a VR_SCENE_HOST_ONLY scene)
# come from the built library, so `python -m vanrijn_amd.build` must have run.  No GPU is used and
# nothing is loaded into python.
#     sh tools/mesh_materials_asan.sh [build directory]
set -eu
root=$(cd "$(dirname "$0")/.." && pwd)
out=${1:-$(mktemp -d)}
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
flags=$(python3 "$root/vanrijn_amd/build.py" --print-flags)
san="-Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer -g"
[ -f "$root/vanrijn_amd/lib/libvanrijn_amd.so" ] || { echo "build the library first" >&2; exit 2; }
objs=""
for f in vr_host vr_host_bvh vr_host_scene vr_host_edit vr_host_rays vr_host_film vr_host_io; do
    "$hipcc" $flags $san -c "$root/vanrijn_amd/csrc/$f.cpp" -o "$out/$f.o" &
    objs="$objs $out/$f.o"
done
wait
"$hipcc" $flags $san -c "$root/tools/mesh_materials_check.cpp" -o "$out/main.o"
"$hipcc" --offload-arch=gfx950 -fsanitize=address,undefined "$out/main.o" $objs -L"$root/vanrijn_amd/lib" -lvanrijn_amd \
    -Wl,-rpath,"$root/vanrijn_amd/lib" -lz -o "$out/mesh_materials_check"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$out/mesh_materials_check" "$out/check.obj"
