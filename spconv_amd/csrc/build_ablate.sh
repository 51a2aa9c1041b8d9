#!/bin/bash
# Measurement builds of igemm.hip with ONE part of a gather-GEMM step compiled out (SPX_ABL in igemm.hip:
# 1 = weights staged once, 2 = also no per-step barrier, 3 = no MFMAs, 4 = no gathered-row loads, 5 = no
# pair-word loads; 0 = nothing removed): lib/libspconv_amd_abl<N>.so, selected with SPX_LIB.  Results of
# ablated runs are wrong by design; tools/dense_probe.py times them.  (f16 kernels only: every other object is
# linked from the product build -- build.sh --list --, csrc/build.sh first.)
#   build_ablate.sh --list [N]    print the object files library N (default 0) is linked from, one per line
set -e
cd "$(dirname "$0")"
OUT=../lib
objs() {   # of library $1: the product build's objects, with its own igemm
  for o in $(bash build.sh --list); do
    if [ "$o" = "igemm.o" ]; then echo $OUT/abl/igemm$1.o; else echo $OUT/$o; fi
  done
}
if [ "$1" = "--list" ]; then
  objs ${2:-0}
  exit 0
fi
mkdir -p $OUT/abl
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-value -mllvm -amdgpu-kernarg-preload-count=16"
for v in ${@:-0 1 2 3 4 5}; do
  ( $HIPCC $FLAGS -DSPX_ABLATE=$v -c igemm.hip -o $OUT/abl/igemm$v.o &&
    $HIPCC --offload-arch=gfx950 -shared -fPIC -o $OUT/libspconv_amd_abl$v.so $(objs $v) &&
    echo built $OUT/libspconv_amd_abl$v.so ) &
done
wait
