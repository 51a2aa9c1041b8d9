#!/bin/bash
# Debug build with the in-kernel timeline stamps (tools/timeline.py): lib/libspconv_amd_dbg.so.  Every translation unit
# of the product build (build.sh --list) compiled with -DSPX_TIMELINE into lib/dbg/.
#   build_debug.sh --list    print the object files the library is linked from, one per line
set -e
cd "$(dirname "$0")"
OUT=../lib
OBJS=""
for o in $(bash build.sh --list); do OBJS="$OBJS $OUT/dbg/$o"; done
if [ "$1" = "--list" ]; then
  for o in $OBJS; do echo $o; done
  exit 0
fi
mkdir -p $OUT/dbg
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -mllvm -amdgpu-kernarg-preload-count=16 -DSPX_TIMELINE"
pids=()
for o in $OBJS; do
  f=$(basename $o .o)
  if [ -f $f.hip ]; then $HIPCC $FLAGS -c $f.hip -o $o & else $HIPCC $FLAGS -x hip -c $f.cpp -o $o & fi
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done   # a failed compile aborts the build (set -e)
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $OUT/libspconv_amd_dbg.so $OBJS
echo built $OUT/libspconv_amd_dbg.so
