#!/bin/bash
# Build the library of a git revision (its csrc + include) into abx/lib<NAME>.so for A/B timing
# against the working tree (abx/ travels to the GPU box; the in-tree library is untouched):
#   bash tools/build_rev.sh HEAD base
# Compiled with the product build's flags (vanrijn_amd/build.py FLAGS, the working tree's: both sides
# of an A/B get the same ones); further arguments are appended to them.
set -eu
cd "$(dirname "$0")/.."
REV=$1; NAME=$2; shift 2
SRC=$(mktemp -d)
git archive "$REV" vanrijn_amd/csrc include | tar -x -C "$SRC"
FLAGS=$(python3 vanrijn_amd/build.py --print-flags)
PIDS=""
# the revision's own translation units (an older one may have fewer than the working tree)
for s in $(cd $SRC/vanrijn_amd/csrc && ls *.hip *.cpp); do
  /opt/rocm/bin/hipcc $FLAGS "$@" -c $SRC/vanrijn_amd/csrc/$s -o $SRC/${s%.*}.o 2>/dev/null &
  PIDS="$PIDS $!"
done
for p in $PIDS; do wait $p; done
mkdir -p abx
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $SRC/*.o -lz -o abx/lib$NAME.so
rm -rf "$SRC"
echo abx/lib$NAME.so
