// What the farthest-point sampling units share (sample.hip: the scan path; fps_bucket.hip: the bucket path): the
// workgroup's shape, the 16-byte record of a streamed point, the fold of a squared distance into t, and the maximum of a
// 64-bit key over a wave.  Internal linkage.
#pragma once
#include "common.h"
#include "scenes.h"

// no multiply-add pair of this header may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kFpsBlock = 1024, kFpsWaves = kFpsBlock / kWave;
constexpr int kMaxSamples = 1 << 16;

struct __attribute__((aligned(16))) FpsRec {
  float x, y, z, t;
};

template <int NDIM> __device__ __forceinline__ float fold(float t, const float (&p)[NDIM], const float (&c)[NDIM]) {
  float d[NDIM];
#pragma unroll
  for (int j = 0; j < NDIM; ++j) d[j] = p[j] - c[j];
  const float d2 = dist2<NDIM>(d);
  return d2 < t ? d2 : t;                             // (false for t < 0: a non-candidate stays one)
}

// max(k, k of the lane the DPP control names): both halves move with the same control
template <int CTRL> __device__ __forceinline__ u64 dpp_max(u64 k) {
  const uint32_t lo = static_cast<uint32_t>(
      __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<uint32_t>(k)), CTRL, 0xf, 0xf, false));
  const uint32_t hi = static_cast<uint32_t>(
      __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<uint32_t>(k >> 32)), CTRL, 0xf, 0xf, false));
  const u64 o = (static_cast<u64>(hi) << 32) | lo;
  return o > k ? o : k;
}

// The maximum over the wave, in every lane (all 64 active).  Inside a row of 16 lanes a butterfly of DPP moves -- lane ^
// 1, lane ^ 2 (quad permutes), then the mirrored half row and the mirrored row, which reach the other quad / half row: a
// maximum does not mind which lane of it -- and the four row results through readlane.
__device__ __forceinline__ u64 wave_max(u64 k) {
  k = dpp_max<0xB1>(k);                                 // quad_perm:[1,0,3,2]
  k = dpp_max<0x4E>(k);                                 // quad_perm:[2,3,0,1]
  k = dpp_max<0x141>(k);                                // row_half_mirror
  k = dpp_max<0x140>(k);                                // row_mirror
  u64 r = 0ull;
#pragma unroll
  for (int row = 0; row < kWave; row += 16) {
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(k)), row));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(k >> 32)), row));
    const u64 o = (static_cast<u64>(hi) << 32) | lo;
    r = o > r ? o : r;
  }
  return r;
}

}  // namespace
}  // namespace spx
