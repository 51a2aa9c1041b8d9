// Exact farthest-point sampling with bucket pruning (spx_fps_bucket_build, spx_fps_bucket): the contract of spx_fps
// (sample.hip) -- the same validity rule, slot 0 the lowest valid point index, ties to the lowest point index, chosen
// points leave the candidate set, -1 at or behind count -- with the SAME indices bit for bit; a step visits only the
// points it can change.
//
//   build     scene boxes (a workgroup per scene: fp32 min / max of the valid points, exact in any order); a 64-bit key
//             per scene-list position (scene << 30 | the Morton code of the coordinates quantised to 10 bits per axis
//             inside the scene's box; all ones for a position in no scene and for an invalid point: the quantisation
//             decides speed, never a result); spx_serialize over the keys (the stable LSD radix sort of serialize.hip and
//             its scene offsets: every scene is a run of sorted positions, invalid points behind all of them); {x, y, z,
//             t} records and the point index of every sorted position.
//   buckets   a BUCKET is a run of 64 << shift consecutive sorted positions of a scene, shift the smallest that keeps
//             the scene at or under kBucketCap buckets (from the scene's own count: uniform).  Per bucket the LDS table
//             holds the box of its points, its best key -- the bits of the largest candidate t above the inverted POINT
//             INDEX, so equal t resolves to the lowest point index whatever the sorted order; 0: no candidate -- and the
//             coordinates of that point.
//   sampling  one workgroup of 1024 lanes per scene.  Init: a wave per bucket reduces box and best key (t = +inf).  A
//             step: every lane reduces the keys of its buckets (tid, tid + 1024), wave_max, 16 LDS slots: the winner, its
//             coordinates c and its bucket; every lane computes the box distance of its buckets to c; a bucket is ACTIVE
//             when that is < its largest candidate t, or when it holds the winner (which must get t = -1 even when all of
//             its bucket ties at 0); active buckets are listed per wave by ballot and prefix popcount, the wave totals
//             scanned through LDS; waves take list entries w, w + 16, ...: a record load per lane (the next one in
//             flight), fold, the store of a changed t, wave_max, one lane rewrites the table entry.  Three barriers per
//             step, all in control flow uniform over the workgroup: trip counts come from LDS words every lane reads or
//             from the scene's offsets.  No spin wait, no cross-workgroup step, no atomics, no scratch.
//
// EXACTNESS.  Rounding is monotone: for a <= b, fl(a - c) <= fl(b - c), and for 0 <= a <= b, fl(a * a) <= fl(b * b) and
// fl(a + x) <= fl(b + x).  The box distance takes per axis lo_j - c_j if that is positive, else hi_j - c_j if that is
// negative, else 0, and squares and sums the terms in the order of dist2 with no FMA contraction.  A point p inside the
// box has lo_j <= p_j <= hi_j, so |fl(p_j - c_j)| >= |the box term| on every axis, and operation by operation
// fl-dist2(p - c) >= the fl-box distance.  If the box distance is >= the bucket's largest candidate t, then d2 < t is
// false for every candidate of the bucket: the step changes none of its t, and skipping the bucket changes nothing.
#include <math.h>

#include "common.h"
#include "fps.h"
#include "scenes.h"

// no multiply-add pair of this unit may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kBucketPoints = kWave;                 // records of a bucket at shift 0: one coalesced wave load
constexpr int kBucketCap = 1280;                     // buckets of a scene: the table stays inside 64 KB of static LDS
constexpr int kBucketPer = (kBucketCap + kFpsBlock - 1) / kFpsBlock;   // buckets a lane owns
constexpr int kBucketMaxShift = 8;
constexpr int kKeyBlock = 256;
constexpr int kSceneShift = 30;                      // 3 x 10 Morton bits below the scene
constexpr long long kBucketMaxPoints = static_cast<long long>(kBucketCap) * (kBucketPoints << kBucketMaxShift);

// -------------------------------------------------------------------------------------------- build

// One workgroup per scene: lo[3], hi[3] of its valid points (+inf / -inf for a scene without one).
template <int NDIM>
__global__ void __launch_bounds__(kFpsBlock)
scene_box_kernel(const float *__restrict__ points, int nfeat, int n_cap, const int32_t *__restrict__ offsets,
                 const int32_t *__restrict__ list, float *__restrict__ boxes) {
  __shared__ float s_box[kFpsWaves][6];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int beg, end;
  scene_range(offsets, n_cap, b, beg, end);
  float lo[3], hi[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) lo[j] = __builtin_huge_valf(), hi[j] = -__builtin_huge_valf();
  for (int pos = beg + tid; pos < end; pos += kFpsBlock) {
    float p[NDIM];
    int pi;
    if (load_point<NDIM>(points, nfeat, n_cap, list, pos, p, pi)) {
#pragma unroll
      for (int j = 0; j < NDIM; ++j) lo[j] = fminf(lo[j], p[j]), hi[j] = fmaxf(hi[j], p[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
      lo[j] = fminf(lo[j], __shfl_xor(lo[j], m, kWave));
      hi[j] = fmaxf(hi[j], __shfl_xor(hi[j], m, kWave));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) s_box[wave][j] = lo[j], s_box[wave][3 + j] = hi[j];
  }
  __syncthreads();
  if (tid < 6) {
    float v = s_box[0][tid];
    for (int w = 1; w < kFpsWaves; ++w) v = tid < 3 ? fminf(v, s_box[w][tid]) : fmaxf(v, s_box[w][tid]);
    boxes[b * 6 + tid] = v;
  }
}

// bit i of v (10 bits) to bit 3 i / 2 i
__device__ __forceinline__ unsigned spread3(unsigned v) {
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
__device__ __forceinline__ unsigned spread2(unsigned v) {
  v = (v | (v << 8)) & 0x00ff00ffu;
  v = (v | (v << 4)) & 0x0f0f0f0fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}

// One lane per position of the scene list: its key.  The scene of a position is the last b with offsets[b] <= pos.
template <int NDIM>
__global__ void __launch_bounds__(kKeyBlock)
bucket_keys_kernel(const float *__restrict__ points, int nfeat, int n_cap, const int32_t *__restrict__ offsets,
                   const int32_t *__restrict__ list, int batch, const float *__restrict__ boxes,
                   unsigned long long *__restrict__ keys) {
  const int pos = blockIdx.x * kKeyBlock + threadIdx.x;
  if (pos >= n_cap) return;
  int lo = 0, hi = batch + 1;                          // the first b with offsets[b] > pos
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] > pos) hi = mid; else lo = mid + 1;
  }
  const int b = lo - 1;
  unsigned long long key = ~0ull;
  float p[NDIM];
  int pi;
  if (b >= 0 && b < batch && load_point<NDIM>(points, nfeat, n_cap, list, pos, p, pi)) {
    unsigned q[NDIM];
#pragma unroll
    for (int j = 0; j < NDIM; ++j) {
      const float l = boxes[b * 6 + j], ext = boxes[b * 6 + 3 + j] - l;
      const float scale = (ext > 0.f && finite(ext)) ? 1024.f / ext : 0.f;     // (a zero extent: cell 0)
      const float cell = fminf(fmaxf((p[j] - l) * scale, 0.f), 1023.f);        // (NaN -> 0)
      q[j] = static_cast<unsigned>(cell);
    }
    const unsigned code = NDIM == 3 ? (spread3(q[0]) << 2) | (spread3(q[1]) << 1) | spread3(q[NDIM - 1])
                                    : (spread2(q[0]) << 1) | spread2(q[1]);
    key = (static_cast<unsigned long long>(b) << kSceneShift) | code;
  }
  keys[pos] = key;
}

// One lane per sorted position: the record and the point index of a live position, {0, 0, 0, -1} / -1 behind them.
template <int NDIM>
__global__ void __launch_bounds__(kKeyBlock)
bucket_records_kernel(const float *__restrict__ points, int nfeat, int n_cap, const int32_t *__restrict__ list,
                      const int32_t *__restrict__ order, const int32_t *__restrict__ soffsets, int batch,
                      FpsRec *__restrict__ recs, int32_t *__restrict__ pidx) {
  const int t = blockIdx.x * kKeyBlock + threadIdx.x;
  if (t >= n_cap) return;
  const int live = min(max(soffsets[batch], 0), n_cap);
  FpsRec r = {0.f, 0.f, 0.f, -1.f};
  int pi = -1;
  if (t < live) {
    const int pos = order[t];
    float p[NDIM];
    if (static_cast<unsigned>(pos) < static_cast<unsigned>(n_cap) &&                     // (checked, not trusted)
        load_point<NDIM>(points, nfeat, n_cap, list, pos, p, pi)) {
      r.x = p[0], r.y = p[1], r.z = NDIM == 3 ? p[NDIM - 1] : 0.f, r.t = __builtin_huge_valf();
    } else {
      pi = -1;
    }
  }
  recs[t] = r;
  pidx[t] = pi;
}

// -------------------------------------------------------------------------------------------- sampling

struct BucketShared {
  float lo[3][kBucketCap], hi[3][kBucketCap];         // the box of a bucket's points
  u64 key[kBucketCap];                                // bits(largest candidate t) << 32 | ~point index; 0: no candidate
  float c[3][kBucketCap];                             // the coordinates of that point
  uint16_t list[kFpsWaves][kBucketPer * kWave];       // the active buckets a wave found
  int cnt[kFpsWaves];                                 // ... and how many
  u64 wkey[kFpsWaves];                                // a wave's winner of the table
  float4 wpt[kFpsWaves];                              // ... {its coordinates, its bucket as bits}
};
static_assert(sizeof(BucketShared) <= 64 * 1024, "the table fits static LDS: no opt-in to more");
static_assert(kBucketCap <= 0xffff, "bucket numbers are listed as 16-bit words");
static_assert(kFpsWaves <= kWave, "the wave totals are scanned by one wave's lanes");

// the smallest shift that keeps n points at or under kBucketCap buckets of kBucketPoints << shift
__host__ __device__ inline int bucket_shift(int n) {
  int shift = 0;
  while (shift < kBucketMaxShift && ((static_cast<long long>(n) + (kBucketPoints << shift) - 1) >> (6 + shift)) > kBucketCap)
    ++shift;
  return shift;
}
static_assert(kBucketPoints == 64, "bucket_shift divides by 64 << shift");

// A lane's best candidate of a bucket: the key and the coordinates that travel with it.
template <int NDIM> struct BucketBest {
  u64 key;
  float c[NDIM];
  __device__ __forceinline__ void clear() {
    key = 0ull;
#pragma unroll
    for (int j = 0; j < NDIM; ++j) c[j] = 0.f;
  }
  __device__ __forceinline__ void consider(float t, int pi, const float (&p)[NDIM]) {
    const u64 k = t >= 0.f ? (static_cast<u64>(__float_as_uint(t)) << 32) | static_cast<uint32_t>(~pi) : 0ull;
    const bool take = k > key;
    key = take ? k : key;
#pragma unroll
    for (int j = 0; j < NDIM; ++j) c[j] = take ? p[j] : c[j];
  }
  // the wave's best into the table entry of bucket bk (point indices are distinct: one lane holds the maximum)
  __device__ __forceinline__ void publish(BucketShared &sh, int bk, int lane) const {
    const u64 wmax = wave_max(key);
    if (wmax != 0ull ? key == wmax : lane == 0) {
      sh.key[bk] = wmax;
#pragma unroll
      for (int j = 0; j < NDIM; ++j) sh.c[j][bk] = c[j];
    }
  }
};

template <int NDIM>
__global__ void __launch_bounds__(kFpsBlock)
fps_bucket_kernel(FpsRec *recs, const int32_t *__restrict__ pidx, const int32_t *__restrict__ soffsets, int n_cap, int K,
                  int32_t *__restrict__ idx, int32_t *__restrict__ count, int32_t *__restrict__ visits) {
  __shared__ BucketShared sh;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int beg, end;
  scene_range(soffsets, n_cap, b, beg, end);
  const int n = static_cast<int>(min(static_cast<long long>(end - beg), kBucketMaxPoints));   // uniform: the scene's own count
  int32_t *out = idx + static_cast<long long>(b) * K;
  const int trips = min(n, K);                          // (every sorted position of a scene is a valid point)
  for (int s = trips + tid; s < K; s += kFpsBlock) out[s] = -1;
  if (tid == 0) count[b] = trips;
  if (n == 0) {                                         // before the first barrier
    if (tid == 0 && visits) visits[b] = 0;
    return;
  }
  const int shift = bucket_shift(n), mask = (1 << shift) - 1;
  const int nb = (n + (kBucketPoints << shift) - 1) >> (6 + shift);
  FpsRec *rec = recs + beg;
  const int32_t *pi_b = pidx + beg;

  // init: a wave per bucket
  for (int bk = wave; bk < nb; bk += kFpsWaves) {
    float lo[NDIM], hi[NDIM];
#pragma unroll
    for (int j = 0; j < NDIM; ++j) lo[j] = __builtin_huge_valf(), hi[j] = -__builtin_huge_valf();
    BucketBest<NDIM> best;
    best.clear();
    for (int sub = 0; sub <= mask; ++sub) {
      const int pos = (((bk << shift) + sub) << 6) + lane;
      if (pos < n) {
        const FpsRec r = rec[pos];
        const float p[3] = {r.x, r.y, r.z};
        float q[NDIM];
#pragma unroll
        for (int j = 0; j < NDIM; ++j) q[j] = p[j], lo[j] = fminf(lo[j], p[j]), hi[j] = fmaxf(hi[j], p[j]);
        const int pi = pi_b[pos];
        const float t = pi >= 0 ? __builtin_huge_valf() : -1.f;
        rec[pos].t = t;                                 // (a second sampling of one build starts over)
        best.consider(t, pi, q);
      }
    }
    best.publish(sh, bk, lane);
#pragma unroll
    for (int j = 0; j < NDIM; ++j) {
#pragma unroll
      for (int m = kWave / 2; m >= 1; m >>= 1) {
        lo[j] = fminf(lo[j], __shfl_xor(lo[j], m, kWave));
        hi[j] = fmaxf(hi[j], __shfl_xor(hi[j], m, kWave));
      }
      if (lane == 0) sh.lo[j][bk] = lo[j], sh.hi[j][bk] = hi[j];
    }
  }
  long long seen = nb;                                  // table entries written: the init's, then every step's
  __syncthreads();

  for (int s = 0; s < trips; ++s) {
    // the argmax over the table: a lane's buckets, the wave, the 16 slots
    u64 k[kBucketPer], mine = 0ull;
    int mb = 0;
#pragma unroll
    for (int j = 0; j < kBucketPer; ++j) {
      const int bk = tid + j * kFpsBlock;
      k[j] = bk < nb ? sh.key[bk] : 0ull;
      if (k[j] > mine) mine = k[j], mb = bk;
    }
    const u64 wmax = wave_max(mine);
    if (wmax != 0ull ? mine == wmax : lane == 0) {
      sh.wkey[wave] = wmax;
      sh.wpt[wave] = make_float4(sh.c[0][mb], sh.c[1][mb], NDIM == 3 ? sh.c[NDIM - 1][mb] : 0.f, __int_as_float(mb));
    }
    __syncthreads();
    u64 win = 0ull;
    int slot = 0;
#pragma unroll
    for (int w = 0; w < kFpsWaves; ++w) {
      const u64 v = sh.wkey[w];
      if (v > win) win = v, slot = w;
    }
    slot = __builtin_amdgcn_readfirstlane(slot);
    const float4 cw = sh.wpt[slot];
    const int chosen = __builtin_amdgcn_readfirstlane(static_cast<int>(~static_cast<uint32_t>(win)));
    const int cb = __builtin_amdgcn_readfirstlane(__float_as_int(cw.w));
    if (tid == 0) out[s] = chosen;                      // (the point index itself: the key carries it)
    if (s + 1 == trips) break;                          // uniform
    float c[NDIM];
    c[0] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(cw.x)));
    c[1] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(cw.y)));
    if (NDIM == 3) c[NDIM - 1] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(cw.z)));

    // the active buckets of this wave's lanes
    int found = 0;
#pragma unroll
    for (int j = 0; j < kBucketPer; ++j) {
      const int bk = tid + j * kFpsBlock;
      bool act = false;
      if (bk < nb) {
        float d[NDIM];
#pragma unroll
        for (int a = 0; a < NDIM; ++a) {
          const float below = sh.lo[a][bk] - c[a], above = sh.hi[a][bk] - c[a];
          d[a] = below > 0.f ? below : (above < 0.f ? above : 0.f);
        }
        act = (k[j] != 0ull && dist2<NDIM>(d) < __uint_as_float(static_cast<uint32_t>(k[j] >> 32))) || bk == cb;
      }
      const unsigned long long bal = __ballot(act);
      const int rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bal >> 32),
                                                 __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bal), 0u));
      if (act) sh.list[wave][found + rank] = static_cast<uint16_t>(bk);
      found += __popcll(bal);
    }
    if (lane == 0) sh.cnt[wave] = found;
    __syncthreads();

    // the inclusive scan of the wave totals, in the first 16 lanes of every wave
    int incl = lane < kFpsWaves ? sh.cnt[lane] : 0;
#pragma unroll
    for (int d = 1; d < kFpsWaves; d <<= 1) {
      const int u = __shfl_up(incl, d, kWave);
      if (lane >= d) incl += u;
    }
    const int na = __builtin_amdgcn_readlane(incl, kFpsWaves - 1);
    seen += na;

    // list entries wave, wave + 16, ...: item i is sub-wave (i & mask) of this wave's entry (i >> shift)
    const int items = na > wave ? ((na - wave + kFpsWaves - 1) / kFpsWaves) << shift : 0;
    int bk = 0, pos = n, pi = -1, bk_n = 0, pos_n = n, pi_n = -1;
    FpsRec r = {0.f, 0.f, 0.f, -1.f}, r_n = r;
    auto fetch = [&](int i, int &f_bk, int &f_pos, int &f_pi, FpsRec &f_r) {
      f_pos = n, f_pi = -1, f_r.x = f_r.y = f_r.z = 0.f, f_r.t = -1.f;
      if (i >= items) return;                           // uniform over the wave
      const int e = wave + (i >> shift) * kFpsWaves;
      const int seg = __popcll(__ballot(lane < kFpsWaves && incl <= e));     // (the wave that listed entry e)
      const int base = seg > 0 ? __builtin_amdgcn_readlane(incl, seg - 1) : 0;
      f_bk = __builtin_amdgcn_readfirstlane(static_cast<int>(sh.list[seg][e - base]));
      f_pos = (((f_bk << shift) + (i & mask)) << 6) + lane;
      if (f_pos < n) f_r = rec[f_pos], f_pi = pi_b[f_pos];
    };
    fetch(0, bk, pos, pi, r);
    BucketBest<NDIM> best;
    best.clear();
    for (int i = 0; i < items; ++i) {
      fetch(i + 1, bk_n, pos_n, pi_n, r_n);             // the next record in flight
      const float p3[3] = {r.x, r.y, r.z};
      float p[NDIM];
#pragma unroll
      for (int j = 0; j < NDIM; ++j) p[j] = p3[j];
      const float t = pi == chosen ? -1.f : fold<NDIM>(r.t, p, c);
      if (pos < n && t != r.t) rec[pos].t = t;
      best.consider(t, pi, p);
      if ((i & mask) == mask) {
        best.publish(sh, bk, lane);
        best.clear();
      }
      bk = bk_n, pos = pos_n, pi = pi_n, r = r_n;
    }
    __syncthreads();                                    // the table is rewritten before it is read
  }
  if (tid == 0 && visits) visits[b] = static_cast<int32_t>(min(seen, 0x7fffffffLL));
}

int bit_length(unsigned v) {
  int bits = 0;
  for (; v; v >>= 1) ++bits;
  return bits;
}

// scratch of the bucket path: what the build writes and the sampling reads, then the sort's own
struct BucketWs {
  float *boxes;
  unsigned long long *keys;
  int32_t *order, *inverse, *soffsets, *pidx;
  FpsRec *recs;
  void *sort;
  size_t sort_bytes, bytes;
  BucketWs(void *ws, int n_cap, int batch) {
    Carver c(ws);
    const size_t nn = n_cap > 0 ? n_cap : 1;
    recs = c.take<FpsRec>(nn);
    pidx = c.take<int32_t>(nn);
    soffsets = c.take<int32_t>(static_cast<size_t>(batch) + 1);
    boxes = c.take<float>(static_cast<size_t>(batch) * 6);
    keys = c.take<unsigned long long>(nn);
    order = c.take<int32_t>(nn);
    inverse = c.take<int32_t>(nn);
    sort_bytes = align_up(spx_serialize_ws_bytes(n_cap, 1, kSceneShift + bit_length(static_cast<unsigned>(batch))), 256);
    sort = c.take<char>(sort_bytes);
    bytes = c.off;
  }
};

// 0 = ok: the checks of a bucket call that need no pointer
int check_bucket(int n_cap, int batch, int ndim) {
  SPX_CHECK(ndim == 2 || ndim == 3, "ndim must be 2 or 3, got %d", ndim);
  SPX_CHECK(n_cap >= 0, "bad point counts %d", n_cap);
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  SPX_CHECK(n_cap <= kBucketMaxPoints, "the bucket path takes up to %lld points (%d buckets of up to %d), got %d",
            kBucketMaxPoints, kBucketCap, kBucketPoints << kBucketMaxShift, n_cap);
  return 0;
}

int check_bucket_ws(int n_cap, int batch, int ndim, const void *ws, size_t ws_bytes) {
  SPX_CHECK(ws && ws_bytes >= spx_fps_bucket_ws_bytes(n_cap, batch, ndim), "workspace too small: %zu < %zu", ws_bytes,
            spx_fps_bucket_ws_bytes(n_cap, batch, ndim));
  SPX_CHECK(aligned_to(ws, 16), "workspace not aligned to 16 bytes");
  return 0;
}

}  // namespace
}  // namespace spx

// -------------------------------------------------------------------------------------------- host side

extern "C" {

int spx_fps_bucket_cap(void) { return spx::kBucketCap; }
int spx_fps_bucket_points(void) { return spx::kBucketPoints; }

size_t spx_fps_bucket_ws_bytes(int n_cap, int batch, int ndim) {
  if ((ndim != 2 && ndim != 3) || n_cap < 0 || batch < 1 || n_cap > spx::kBucketMaxPoints) return 0;
  return spx::BucketWs(nullptr, n_cap, batch).bytes;
}

int spx_fps_bucket_build(const float *points, int nfeat, int n_cap, int ndim, const int32_t *offsets, const int32_t *list,
                         int batch, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_bucket(n_cap, batch, ndim)) return rc;
  SPX_CHECK(nfeat >= ndim, "points need at least %d columns, got %d", ndim, nfeat);
  SPX_CHECK(offsets && (n_cap == 0 || (points && list)), "points / offsets / list is NULL");
  SPX_CHECK(aligned_to(points, 4) && aligned_to(offsets, 4) && aligned_to(list, 4), "pointer not aligned to its elements");
  if (int rc = check_bucket_ws(n_cap, batch, ndim, ws, ws_bytes)) return rc;
  const BucketWs w(ws, n_cap, batch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 per_point(static_cast<unsigned>(div_up(n_cap, kKeyBlock)));
  if (n_cap > 0) {
    if (ndim == 3) {
      hipLaunchKernelGGL((scene_box_kernel<3>), dim3(batch), dim3(kFpsBlock), 0, s, points, nfeat, n_cap, offsets, list,
                         w.boxes);
      hipLaunchKernelGGL((bucket_keys_kernel<3>), per_point, dim3(kKeyBlock), 0, s, points, nfeat, n_cap, offsets, list, batch,
                         w.boxes, w.keys);
    } else {
      hipLaunchKernelGGL((scene_box_kernel<2>), dim3(batch), dim3(kFpsBlock), 0, s, points, nfeat, n_cap, offsets, list,
                         w.boxes);
      hipLaunchKernelGGL((bucket_keys_kernel<2>), per_point, dim3(kKeyBlock), 0, s, points, nfeat, n_cap, offsets, list, batch,
                         w.boxes, w.keys);
    }
    SPX_LAUNCH_CHECK();
  }
  // the one sort of the library, through its entry: order, and the scenes' offsets among the sorted positions
  if (int rc = spx_serialize(reinterpret_cast<const uint64_t *>(w.keys), n_cap, 1,
                             kSceneShift + bit_length(static_cast<unsigned>(batch)), batch, kSceneShift, w.order, w.inverse,
                             w.soffsets, w.sort, w.sort_bytes, stream))
    return rc;
  if (n_cap > 0) {
    if (ndim == 3)
      hipLaunchKernelGGL((bucket_records_kernel<3>), per_point, dim3(kKeyBlock), 0, s, points, nfeat, n_cap, list, w.order,
                         w.soffsets, batch, w.recs, w.pidx);
    else
      hipLaunchKernelGGL((bucket_records_kernel<2>), per_point, dim3(kKeyBlock), 0, s, points, nfeat, n_cap, list, w.order,
                         w.soffsets, batch, w.recs, w.pidx);
    SPX_LAUNCH_CHECK();
  }
  return 0;
}

int spx_fps_bucket(int n_cap, int ndim, int batch, int num_samples, int32_t *idx, int32_t *count, int32_t *visits, void *ws,
                   size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_bucket(n_cap, batch, ndim)) return rc;
  SPX_CHECK(num_samples >= 1 && num_samples <= kMaxSamples, "num_samples must be in 1 .. %d, got %d", kMaxSamples,
            num_samples);
  SPX_CHECK(static_cast<long long>(batch) * num_samples < 0x80000000LL, "batch * num_samples must stay below 2^31, got %d x %d",
            batch, num_samples);
  SPX_CHECK(idx && count, "idx / count is NULL");
  SPX_CHECK(aligned_to(idx, 4) && aligned_to(count, 4) && aligned_to(visits, 4), "pointer not aligned to its elements");
  if (int rc = check_bucket_ws(n_cap, batch, ndim, ws, ws_bytes)) return rc;
  const BucketWs w(ws, n_cap, batch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (ndim == 3)
    hipLaunchKernelGGL((fps_bucket_kernel<3>), dim3(batch), dim3(kFpsBlock), 0, s, w.recs, w.pidx, w.soffsets, n_cap,
                       num_samples, idx, count, visits);
  else
    hipLaunchKernelGGL((fps_bucket_kernel<2>), dim3(batch), dim3(kFpsBlock), 0, s, w.recs, w.pidx, w.soffsets, n_cap,
                       num_samples, idx, count, visits);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
