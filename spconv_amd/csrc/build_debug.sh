#!/bin/bash
# Debug build with the in-kernel timeline stamps (tools/timeline.py): lib/libspconv_amd_dbg.so
set -e
cd "$(dirname "$0")"
OUT=../lib
mkdir -p $OUT/dbg
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -mllvm -amdgpu-kernarg-preload-count=16 -DSPX_TIMELINE"
$HIPCC $FLAGS -c rulebook.hip -o $OUT/dbg/rulebook.o &
$HIPCC $FLAGS -c igemm.hip -o $OUT/dbg/igemm.o &
$HIPCC $FLAGS -c pool.hip -o $OUT/dbg/pool.o &
$HIPCC $FLAGS -c igemm_gen1.hip -o $OUT/dbg/igemm_gen1.o &
for f in igemm_wgrad igemm_bf16 igemm_f32 igemm_f64 igemm_i8 igemm_wide igemm_ws; do $HIPCC $FLAGS -c $f.hip -o $OUT/dbg/$f.o & done
$HIPCC $FLAGS -c igemm_bwdn.hip -o $OUT/dbg/igemm_bwdn.o &
$HIPCC $FLAGS -c rowsort.hip -o $OUT/dbg/rowsort.o &
$HIPCC $FLAGS -c norm.hip -o $OUT/dbg/norm.o &
$HIPCC $FLAGS -c dense.hip -o $OUT/dbg/dense.o &
$HIPCC $FLAGS -c union.hip -o $OUT/dbg/union.o &
$HIPCC $FLAGS -c collapse.hip -o $OUT/dbg/collapse.o &
$HIPCC $FLAGS -c pointvoxel.hip -o $OUT/dbg/pointvoxel.o &
$HIPCC $FLAGS -c voxelize.hip -o $OUT/dbg/voxelize.o &
$HIPCC $FLAGS -c hash.hip -o $OUT/dbg/hash.o &
$HIPCC $FLAGS -x hip -c common.cpp -o $OUT/dbg/common.o &
wait
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $OUT/libspconv_amd_dbg.so $OUT/dbg/rulebook.o $OUT/dbg/igemm.o $OUT/dbg/igemm_wgrad.o $OUT/dbg/pool.o $OUT/dbg/igemm_gen1.o $OUT/dbg/igemm_bf16.o $OUT/dbg/igemm_f32.o $OUT/dbg/igemm_f64.o $OUT/dbg/igemm_i8.o $OUT/dbg/igemm_wide.o $OUT/dbg/igemm_ws.o $OUT/dbg/igemm_bwdn.o $OUT/dbg/rowsort.o $OUT/dbg/norm.o $OUT/dbg/dense.o $OUT/dbg/union.o $OUT/dbg/collapse.o $OUT/dbg/pointvoxel.o $OUT/dbg/voxelize.o $OUT/dbg/hash.o $OUT/dbg/common.o
echo built $OUT/libspconv_amd_dbg.so
