#!/bin/bash
# Build several A/B variants of the library in parallel into abx/lib<name>.so (travels to the GPU box; git-ignored): the other
# translation units are compiled once; each variant recompiles vr_render.hip with its own flags.
#   bash tools/variant_libs.sh base "" split "-DVR_NODE_SPLIT_LOAD" ...
set -eu
cd "$(dirname "$0")/.."
# the product build's compile flags (vanrijn_amd/build.py FLAGS), so a variant differs only by its own
FLAGS=$(python3 vanrijn_amd/build.py --print-flags)
COMMON=$(mktemp -d)
mkdir -p abx
OTHERS=$(python3 vanrijn_amd/build.py --print-sources | tr ' ' '\n' | grep -v '^vr_render.hip$')
for s in $OTHERS; do
  /opt/rocm/bin/hipcc $FLAGS -c vanrijn_amd/csrc/$s -o $COMMON/${s%.*}.o &
done
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  ( /opt/rocm/bin/hipcc $FLAGS $flags -c vanrijn_amd/csrc/vr_render.hip -o $COMMON/render_$name.o 2>/dev/null ) &
  NAMES="${NAMES:-} $name"
done
wait
for name in $NAMES; do
  OBJS=""
  for s in $OTHERS; do OBJS="$OBJS $COMMON/${s%.*}.o"; done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $COMMON/render_$name.o $OBJS -lz -o abx/lib$name.so
  echo abx/lib$name.so
done
rm -rf "$COMMON"
