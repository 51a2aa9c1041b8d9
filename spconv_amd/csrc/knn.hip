// k-nearest-neighbour query over raw points with inverse-distance weights (spx_knn_query): the three_nn of pointnet2's
// feature propagation (k = 3, width 4: the table spx_interp_fwd / spx_interp_bwd blend) and the knn_query of pointops
// (the rows spx_group_fwd / spx_group_bwd gather).  Scenes (sample.hip says what one is), the validity of a point and of
// a query, the distance, the scene walk and the host checks of such a call are scenes.h's.
//
//   result    per valid query the min(valid points of its scene, k) smallest candidates under the TOTAL ORDER (d2, point
//             index), in that order.  One 64-bit key per candidate -- the bits of d2 (a non-negative float orders as its
//             bits) above the point index -- decides both fields with one compare, so the result does not depend on the
//             order in which points are met.
//   kernel    one lane per query, workgroups of 256 consecutive queries, the scene walk and the staged tiles of
//             scenes.h: ascending scenes of the workgroup's queries, tiles of 1024 {x, y, z, index} records in LDS,
//             eight staged points tested at a time.  The gate is one float compare per point against the d2 of the
//             lane's worst kept key; only a point that passes it builds its key.
//   list      a lane keeps T = 4 / 16 / 64 keys sorted ascending in registers (the tier: the smallest T >= k).  Slots
//             [0, T - k) hold key 0 and never move, the k best are slots [T - k, T): the worst kept key is the STATIC
//             slot T - 1 whatever k is.  An insertion shifts the statically indexed slots in place, in blocks of
//             eight; a block wholly inside the dead slots is skipped by a uniform branch.  An empty slot holds the
//             sentinel {+inf, 0xffffffff}, above every real key.
// Every barrier sits in control flow that is uniform over the workgroup (see sample.hip).  Distances, square roots and
// divisions are fp32 operations rounded on their own, so a host loop reproduces every output bit for bit.
#include "common.h"
#include "scenes.h"

// no multiply-add pair of this unit may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kKnnChain = 8;                         // slots of a block of an insertion
constexpr int kKnnMaxK = 64;
constexpr u64 kEmpty = (0x7f800000ull << 32) | 0xffffffffull;    // d2 = +inf, no point index

struct KnnArgs : SceneArgs {
  int k, width;
  float eps;
  int flags;
  int32_t *rows, *count;
  float *dist2, *weights, *out_offsets;
};

// The sorted list of a lane.  `dead` = T - k is uniform over the launch.
template <int T> struct KnnList {
  u64 a[T];
  __device__ __forceinline__ void clear(int dead) {
#pragma unroll
    for (int i = 0; i < T; ++i) a[i] = i < dead ? 0ull : kEmpty;
  }
  __device__ __forceinline__ float worst_d2() const { return __uint_as_float(static_cast<uint32_t>(a[T - 1] >> 32)); }
  // Slot i takes its lower neighbour where x belongs below that one, x where x belongs exactly here, and stays
  // otherwise; walked from the top, every slot reads values not yet overwritten, and the compares -- all against the
  // same x -- do not wait for one another.  A key that is not below the worst kept one changes nothing.
  __device__ __forceinline__ void insert(u64 x, int dead) {
    constexpr int kBlk = T < kKnnChain ? T : kKnnChain;
    bool here = x < a[T - 1];
#pragma unroll
    for (int blk = T - kBlk; blk >= 0; blk -= kBlk) {
      if (blk + kBlk <= dead) continue;                 // uniform: the block holds dead slots only (key 0: they stay)
#pragma unroll
      for (int i = blk + kBlk - 1; i >= blk; --i) {
        const bool below = i > 0 && x < a[i > 0 ? i - 1 : 0];
        a[i] = below ? a[i > 0 ? i - 1 : 0] : here ? x : a[i];
        here = below;
      }
    }
  }
};

template <int NDIM, int T>
__global__ void __launch_bounds__(kSceneBlock)
knn_query_kernel(KnnArgs a) {
  __shared__ float4 s_pt[kSceneTile];                   // {x, y, z, the point index as bits}; x = NaN: invalid
  __shared__ int s_next[2][kSceneWaves];
  const long long qi = static_cast<long long>(blockIdx.x) * kSceneBlock + threadIdx.x;
  const bool exists = qi < a.m_cap;                     // (a lane without a query still takes every barrier)
  const int dead = T - a.k;
  float q[NDIM];
  const int mine = load_scene_query<NDIM>(a, qi, q);
  KnnList<T> best;
  best.clear(dead);
  int cur = -1;
  for (int it = 0;; ++it) {
    const int next = next_scene(mine, cur, it, s_next);
    if (next == INT_MAX) break;                         // the same LDS words for every lane: uniform
    cur = next;
    int beg, end;
    scene_range(a.offsets, a.n_cap, next, beg, end);
    const bool active = mine == next;
    for (int tile0 = beg; tile0 < end; tile0 += kSceneTile) {
      const int padded = stage_tile<NDIM>(a, tile0, end, s_pt);
      // kSceneAhead staged points at a time: their reads and distances are independent, a point that enters the list is
      // rare.  A wave none of whose lanes belongs to this scene skips the tile (a uniform branch); a lane of another
      // scene inside a busy wave never passes the gate.
      const bool wave_active = __ballot(active) != 0ull;
      for (int k0 = 0; k0 < padded && wave_active; k0 += kSceneAhead) {
        float4 p[kSceneAhead];
        float d2[kSceneAhead];
        const float gate = active ? best.worst_d2() : -1.f;          // (no d2 is <= -1: a lane of another scene)
        unsigned hits = 0u;
#pragma unroll
        for (int u = 0; u < kSceneAhead; ++u) p[u] = s_pt[k0 + u];
#pragma unroll
        for (int u = 0; u < kSceneAhead; ++u) {
          float d[NDIM];
          d[0] = p[u].x - q[0];
          d[1] = p[u].y - q[1];
          if (NDIM == 3) d[NDIM - 1] = p[u].z - q[NDIM - 1];
          d2[u] = dist2<NDIM>(d);
          hits |= d2[u] <= gate ? 1u << u : 0u;         // (false for an invalid point: its d2 is NaN)
        }
        // one copy of the insertion: a lane takes its own candidates one by one (selects over the eight, no indexed
        // register), and the wave runs it as often as its busiest lane needs, not once per staged point
        while (hits != 0u) {
          const int u = __builtin_ctz(hits);
          hits &= hits - 1u;
          uint32_t hi = __float_as_uint(d2[0]), lo = __float_as_uint(p[0].w);
#pragma unroll
          for (int v = 1; v < kSceneAhead; ++v) {
            hi = u == v ? __float_as_uint(d2[v]) : hi;
            lo = u == v ? __float_as_uint(p[v].w) : lo;
          }
          best.insert((static_cast<u64>(hi) << 32) | lo, dead);       // (a key not below the worst one changes nothing)
        }
      }
      __syncthreads();                                  // the tile is read to its end before the next one is staged
    }
  }
  if (!exists) return;
  // slot s of the result is list slot dead + s.  First pass: the count, slot 0 and the norm of the weights, added in
  // ascending slot; second pass: the tables.
  int cnt = 0;
  u64 first = kEmpty;
  float norm = 0.f;
#pragma unroll
  for (int i = 0; i < T; ++i) {
    if (i < dead || best.a[i] == kEmpty) continue;
    if (cnt == 0) first = best.a[i];
    ++cnt;
    if (a.weights) {
      const float r = 1.f / (sqrtf(__uint_as_float(static_cast<uint32_t>(best.a[i] >> 32))) + a.eps);
      norm = cnt == 1 ? r : norm + r;
    }
    __builtin_amdgcn_sched_barrier(0);                  // (one slot at a time: T square roots in flight spill)
  }
  const bool pad = (a.flags & kFlagPadFirst) && cnt > 0;
  const long long base = qi * a.width;
  int32_t *ro = a.rows + base;
  float *d2o = a.dist2 ? a.dist2 + base : nullptr;
  float *wo = a.weights ? a.weights + base : nullptr;
  float *oo = a.out_offsets ? a.out_offsets + base * NDIM : nullptr;
#pragma unroll
  for (int i = 0; i < T; ++i) {
    const int s = i - dead;
    if (s < 0) continue;
    const bool live = s < cnt;
    const u64 key = live ? best.a[i] : first;
    const bool has = live || pad;
    const int pi = has ? static_cast<int>(static_cast<uint32_t>(key)) : -1;
    const float d2 = has ? __uint_as_float(static_cast<uint32_t>(key >> 32)) : 0.f;
    ro[s] = pi;
    if (d2o) d2o[s] = d2;
    if (wo) wo[s] = live ? (1.f / (sqrtf(d2) + a.eps)) / norm : 0.f;
    if (oo) {
#pragma unroll
      for (int j = 0; j < NDIM; ++j)
        oo[s * NDIM + j] = has ? a.points[static_cast<size_t>(pi) * a.nfeat + j] - q[j] : 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);                  // (one slot's loads at a time)
  }
  for (int s = a.k; s < a.width; ++s) {
    ro[s] = -1;
    if (d2o) d2o[s] = 0.f;
    if (wo) wo[s] = 0.f;
    if (oo) {
#pragma unroll
      for (int j = 0; j < NDIM; ++j) oo[s * NDIM + j] = 0.f;
    }
  }
  a.count[qi] = cnt;
}

template <int NDIM> void launch_knn(const KnnArgs &a, dim3 grid, hipStream_t s) {
  if (a.k <= 4)
    hipLaunchKernelGGL((knn_query_kernel<NDIM, 4>), grid, dim3(kSceneBlock), 0, s, a);
  else if (a.k <= 16)
    hipLaunchKernelGGL((knn_query_kernel<NDIM, 16>), grid, dim3(kSceneBlock), 0, s, a);
  else
    hipLaunchKernelGGL((knn_query_kernel<NDIM, 64>), grid, dim3(kSceneBlock), 0, s, a);
}

}  // namespace
}  // namespace spx

extern "C" {

int spx_knn_max_k(void) { return spx::kKnnMaxK; }

int spx_knn_query(const float *queries, int q_nfeat, const int32_t *q_batch_ids, int m_cap, const int32_t *n_queries_dev,
                  const float *points, int nfeat, int n_cap, int ndim, const int32_t *offsets, const int32_t *list,
                  int batch, int k, int width, float eps, int flags, int32_t *rows, int32_t *count, float *dist2,
                  float *weights, float *out_offsets, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(k >= 1 && k <= kKnnMaxK, "k must be in 1 .. %d, got %d", kKnnMaxK, k);
  SPX_CHECK(width >= k, "width must be >= k, got %d < %d", width, k);
  SPX_CHECK(eps >= 0.f && eps < __builtin_huge_valf(), "eps must be finite and >= 0");
  const KnnArgs a = {{queries, q_nfeat, q_batch_ids, m_cap, n_queries_dev, points, nfeat, n_cap, offsets, list, batch},
                     k, width, eps, flags, rows, count, dist2, weights, out_offsets};
  if (int rc = check_scene_query(a, ndim, width, flags, rows, count, {dist2, weights, out_offsets})) return rc;
  if (m_cap == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((static_cast<long long>(m_cap) + kSceneBlock - 1) / kSceneBlock));
  if (ndim == 3)
    launch_knn<3>(a, grid, s);
  else
    launch_knn<2>(a, grid, s);
  SPX_LAUNCH_CHECK();
  spx::count(kSampleKnnQuery);
  return 0;
}

}  // extern "C"
