// Farthest-point sampling, its sectorised form and ball query over raw points (spx_fps, spx_sector_ids, spx_fps_quota,
// spx_fps_segments, spx_ball_query): the keypoint stage of the
// point-voxel detectors (PV-RCNN, PV-RCNN++, the raw-point source of Voxel R-CNN's set abstraction) -- the
// furthest_point_sample / ball_query extensions of pointnet2_stack.  The rows of a ball query are what spx_group_fwd /
// spx_group_bwd (query.hip) gather and transpose, with the points standing where a level's rows do.
//
//   scenes    the points of scene b are list[offsets[b] .. offsets[b + 1]) of spx_point_groups over the batch ids: any
//             input order, ascending point index inside a scene.  A point with a coordinate that is not finite is
//             INVALID: never a sample, never a hit.
//   fps       one workgroup of 1024 lanes per scene, sequential in the K samples.  Every valid point keeps t (+inf at
//             first); a step folds the squared distance to the last sample into t and picks the candidate with the
//             largest t, ties to the lowest point index; a chosen point stops being a candidate.  The argmax is one
//             64-bit key per lane -- the bits of t (a non-negative float: its bits order as an integer) above the
//             inverted scene position -- reduced over the wave by DPP moves and readlane; every wave's winner goes to
//             LDS WITH its coordinates, in slots alternated by step parity, and every lane reads the 16 slots behind
//             ONE barrier per step.  A scene of up to kResident points keeps coordinates and t in registers (no global load in a
//             step); a larger one streams {x, y, z, t} records staged in ws, each lane its own.  The tier is a uniform
//             branch on the scene's own count.  No workgroup waits for another.
//   ball      one lane per query, workgroups of 256 consecutive queries, on the scene walk of scenes.h (with the
//             distance, the validity of a point and the host checks, shared with knn.hip).  The workgroup walks the
//             scenes of its valid queries in ascending order (scene-contiguous queries: at most two), stages tiles of
//             that scene's points in LDS, and every lane of the scene tests the staged point all lanes read together (a
//             broadcast), appending while it has room.  The workgroup leaves a scene once none of its lanes has room.
//   sectors   sectorised sampling (spx_sector_ids, spx_fps_quota, spx_fps_segments; PV-RCNN++'s
//             sectorized_proposal_centric_sampling, pointnet2_stack's stack_farthest_point_sample): a SEGMENT id per point
//             -- scene * S + azimuth sector, -1 for a point in no scene or turned down by the RoI filter (one lane per
//             point; the filter on the scene walk with the roles turned, as roi.hip: a scene's boxes staged in LDS, the
//             nearest centre decides) --, spx_point_groups over it, a quota per segment in proportion to its points (a
//             wave per scene), and fps_scene with K read per segment: a workgroup per segment writing into its slots of
//             the scene's packed row.  B * S workgroups on B * S CUs; none waits for another.
// Every barrier sits in control flow that is uniform over the workgroup: trip counts come from values every lane reads
// from the same LDS words or from the scene's offsets.  The distances are fp32 with every operation rounded on its
// own, so a host loop reproduces every output bit for bit.
#include <math.h>

#include "common.h"
#include "fill.h"
#include "scenes.h"

// no multiply-add pair of this unit may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kFpsBlock = 1024, kFpsWaves = kFpsBlock / kWave;
constexpr int kFpsPer = 16;                          // points per lane of the register tier
constexpr int kFpsResident = kFpsBlock * kFpsPer;
constexpr int kFpsAhead = 6;                         // records of a batch of the streamed tier; a lane keeps two batches
constexpr int kMaxSamples = 1 << 16;
constexpr int kMaxSample = 128;

struct __attribute__((aligned(16))) FpsRec {
  float x, y, z, t;
};

// -------------------------------------------------------------------------------------------- farthest-point sampling

// A lane's best candidate: its t (< 0: none), scene position and coordinates.  A lane meets its positions in ascending
// order, so the strict compare keeps the LOWEST position of equal t.
template <int NDIM> struct Best {
  float t;
  int pos;
  float c[NDIM];
  __device__ __forceinline__ void clear() {
    t = -1.f;
    pos = 0;
#pragma unroll
    for (int j = 0; j < NDIM; ++j) c[j] = 0.f;
  }
  // bits(t) << 32 | ~position: a non-negative float orders as its bits, equal t by the lower position; 0: none
  __device__ __forceinline__ u64 key() const {
    return t >= 0.f ? (static_cast<u64>(__float_as_uint(t)) << 32) | static_cast<uint32_t>(~pos) : 0ull;
  }
};

// t < 0 marks a point that is no candidate (invalid, absent or chosen)
template <int NDIM>
__device__ __forceinline__ void consider(Best<NDIM> &best, float t, int pos, const float (&p)[NDIM]) {
  const bool take = t > best.t;                       // (selects: a branch per point would split every step)
  best.t = take ? t : best.t;
  best.pos = take ? pos : best.pos;
#pragma unroll
  for (int j = 0; j < NDIM; ++j) best.c[j] = take ? p[j] : best.c[j];
}

template <int NDIM> __device__ __forceinline__ float fold(float t, const float (&p)[NDIM], const float (&c)[NDIM]) {
  float d[NDIM];
#pragma unroll
  for (int j = 0; j < NDIM; ++j) d[j] = p[j] - c[j];
  const float d2 = dist2<NDIM>(d);
  return d2 < t ? d2 : t;                             // (false for t < 0: a non-candidate stays one)
}

// The register tier: lane `tid` holds positions tid + 1024 j, j < 16.  Every loop is unrolled with constant bounds (the
// arrays live in registers); the test against n is uniform.
template <int NDIM> struct ResidentPoints {
  float p[kFpsPer][NDIM], t[kFpsPer];
  __device__ __forceinline__ int init(const float *points, int nfeat, int n_cap, const int32_t *list_b, int n, int tid,
                                      FpsRec *, Best<NDIM> &best) {
    int valid = 0;
#pragma unroll
    for (int j = 0; j < kFpsPer; ++j) {
      const int pos = tid + j * kFpsBlock;
      t[j] = -1.f;
#pragma unroll
      for (int k = 0; k < NDIM; ++k) p[j][k] = 0.f;
      if (j * kFpsBlock < n) {
        int pi;
        if (pos < n && load_point<NDIM>(points, nfeat, n_cap, list_b, pos, p[j], pi)) {
          t[j] = __builtin_huge_valf();
          ++valid;
        }
        consider<NDIM>(best, t[j], pos, p[j]);
      }
      __builtin_amdgcn_sched_barrier(0);                // (one point's loads at a time: sixteen in flight spill)
    }
    return valid;
  }
  __device__ __forceinline__ void step(const float (&c)[NDIM], int chosen, int n, int tid, Best<NDIM> &best) {
#pragma unroll
    for (int j = 0; j < kFpsPer; ++j) {
      const int pos = tid + j * kFpsBlock;
      if (j * kFpsBlock < n) {
        t[j] = pos == chosen ? -1.f : fold<NDIM>(t[j], p[j], c);
        consider<NDIM>(best, t[j], pos, p[j]);
      }
      if (j % 4 == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }
};

// The streamed tier: lane `tid` owns the records of positions tid + 1024 j of its scene, in scene order.
template <int NDIM> struct StreamedPoints {
  FpsRec *rec;
  __device__ __forceinline__ int init(const float *points, int nfeat, int n_cap, const int32_t *list_b, int n, int tid,
                                      FpsRec *recs, Best<NDIM> &best) {
    rec = recs;
    int valid = 0;
    for (int pos = tid; pos < n; pos += kFpsBlock) {
      float p[NDIM];
      int pi;
      const bool ok = load_point<NDIM>(points, nfeat, n_cap, list_b, pos, p, pi);
      const float t = ok ? __builtin_huge_valf() : -1.f;
      FpsRec r = {p[0], p[1], NDIM == 3 ? p[NDIM - 1] : 0.f, t};
      rec[pos] = r;
      valid += ok ? 1 : 0;
      consider<NDIM>(best, t, pos, p);
    }
    return valid;
  }
  // the records of positions base + 1024 u, u < kFpsAhead (t = -1 beyond the scene): their loads in flight together
  __device__ __forceinline__ void load(FpsRec (&r)[kFpsAhead], int base, int n) const {
#pragma unroll
    for (int u = 0; u < kFpsAhead; ++u) {
      const int pos = base + u * kFpsBlock;
      r[u].x = r[u].y = r[u].z = 0.f;
      r[u].t = -1.f;
      if (pos < n) r[u] = rec[pos];
    }
  }
  // Two batches deep: the loads of the next batch are issued BEFORE the stores of this one, so waiting for them does not
  // wait for the stores' acknowledgements (loads and stores share one counter).  Worth 2 % of a step at 75 000 points
  // (profiles/sample_probe.json; DESIGN.md section 3.30 says what a step of this tier costs).
  __device__ __forceinline__ void step(const float (&c)[NDIM], int chosen, int n, int tid, Best<NDIM> &best) {
    FpsRec r[kFpsAhead];
    load(r, tid, n);
    for (int base = tid; base < n; base += kFpsAhead * kFpsBlock) {
      FpsRec ahead[kFpsAhead];
      load(ahead, base + kFpsAhead * kFpsBlock, n);
#pragma unroll
      for (int u = 0; u < kFpsAhead; ++u) {             // (ascending position)
        const int pos = base + u * kFpsBlock;
        float p[NDIM];
        p[0] = r[u].x;
        p[1] = r[u].y;
        if (NDIM == 3) p[NDIM - 1] = r[u].z;
        const float t = pos == chosen ? -1.f : fold<NDIM>(r[u].t, p, c);
        if (pos < n) rec[pos].t = t;
        consider<NDIM>(best, t, pos, p);
      }
#pragma unroll
      for (int u = 0; u < kFpsAhead; ++u) r[u] = ahead[u];
    }
  }
};

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

struct FpsShared {
  u64 key[2][kFpsWaves];
  float4 pt[2][kFpsWaves];
  int valid[kFpsWaves];
};

// One scene of n >= 1 points, all 1024 lanes inside.  out: the scene's row of idx.
template <int NDIM, typename Points>
__device__ __forceinline__ void fps_scene(FpsShared &sh, const float *points, int nfeat, int n_cap, const int32_t *list_b,
                                          int n, int K, FpsRec *recs, int32_t *out, int32_t *count_b) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  Points pts;
  Best<NDIM> best;
  best.clear();
  int valid = pts.init(points, nfeat, n_cap, list_b, n, tid, recs, best);
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) valid += __shfl_xor(valid, m, kWave);
  if (lane == 0) sh.valid[wave] = valid;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < kFpsWaves; ++w) total += sh.valid[w];
  const int trips = total < K ? total : K;              // the same LDS words for every lane: uniform
  for (int s = 0; s < trips; ++s) {
    const int par = s & 1;
    const u64 mine = best.key();
    const u64 wmax = wave_max(mine);
    if (wmax != 0ull ? mine == wmax : lane == 0) {  // (keys are unique: one lane)
      sh.key[par][wave] = wmax;
      sh.pt[par][wave] = make_float4(best.c[0], best.c[1], NDIM == 3 ? best.c[NDIM - 1] : 0.f, 0.f);
    }
    __syncthreads();
    u64 win = 0ull;
    int slot = 0;
#pragma unroll
    for (int h = 0; h < kFpsWaves; h += 8) {            // (two batches of reads: sixteen keys in flight would not fit)
#pragma unroll
      for (int w = h; w < h + 8; ++w) {
        const u64 k = sh.key[par][w];
        if (k > win) {
          win = k;
          slot = w;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // every lane holds the same winner: kept in scalar registers for the pass over the lane's points
    slot = __builtin_amdgcn_readfirstlane(slot);
    const float4 cw = sh.pt[par][slot];
    const int chosen = __builtin_amdgcn_readfirstlane(static_cast<int>(~static_cast<uint32_t>(win)));
    if (tid == 0) out[s] = chosen;                      // (the scene position; turned into the point index below)
    if (s + 1 < trips) {
      float c[NDIM];
      c[0] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(cw.x)));
      c[1] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(cw.y)));
      if (NDIM == 3) c[NDIM - 1] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(cw.z)));
      best.clear();
      pts.step(c, chosen, n, tid, best);
    }
  }
  __syncthreads();                                      // lane 0's positions are visible to the workgroup
  for (int s = tid; s < K; s += kFpsBlock) {
    int v = -1;
    if (s < trips) {
      const int pos = out[s];
      v = static_cast<unsigned>(pos) < static_cast<unsigned>(n) ? list_b[pos] : -1;
    }
    out[s] = v;
  }
  if (tid == 0) *count_b = trips;
}

template <int NDIM>
__global__ void __launch_bounds__(kFpsBlock)
fps_kernel(const float *__restrict__ points, int nfeat, int n_cap, const int32_t *__restrict__ offsets,
           const int32_t *__restrict__ list, int K, int32_t *idx, int32_t *__restrict__ count, FpsRec *recs) {
  __shared__ FpsShared sh;
  const int b = blockIdx.x;
  int beg, end;
  scene_range(offsets, n_cap, b, beg, end);
  const int n = end - beg;                              // uniform: the scene's own count
  int32_t *out = idx + static_cast<long long>(b) * K;
  if (n == 0) {                                         // before the first barrier
    for (int s = threadIdx.x; s < K; s += kFpsBlock) out[s] = -1;
    if (threadIdx.x == 0) count[b] = 0;
    return;
  }
  if (n <= kFpsResident || recs == nullptr)             // (the host refuses n_cap > kFpsResident without scratch)
    fps_scene<NDIM, ResidentPoints<NDIM>>(sh, points, nfeat, n_cap, list + beg, min(n, kFpsResident), K, nullptr, out,
                                          count + b);
  else
    fps_scene<NDIM, StreamedPoints<NDIM>>(sh, points, nfeat, n_cap, list + beg, n, K, recs + beg, out, count + b);
}

// -------------------------------------------------------------------------------------------- ball query

struct BallArgs : SceneArgs {
  int nsample;
  float r2;
  int flags;
  int32_t *rows, *count;
  float *out_offsets;
};

template <int NDIM>
__global__ void __launch_bounds__(kSceneBlock)
ball_query_kernel(BallArgs a) {
  __shared__ float4 s_pt[kSceneTile];                   // {x, y, z, the point index as bits}; x = NaN: invalid
  __shared__ int s_next[2][kSceneWaves];
  const long long qi = static_cast<long long>(blockIdx.x) * kSceneBlock + threadIdx.x;
  const bool exists = qi < a.m_cap;                     // (a lane without a query still takes every barrier)
  // load_scene_query with a NaN-only test of the coordinates, kept here: the finite test gives the same results (an
  // infinite coordinate makes every d2 +inf or NaN, never < r2) but cost 0.6 % of a call (see scenes.h)
  const int nq = a.n_queries ? min(*a.n_queries, a.m_cap) : a.m_cap;
  bool valid = qi < nq;
  int b = -1;
  float q[NDIM];
#pragma unroll
  for (int j = 0; j < NDIM; ++j) q[j] = 0.f;
  if (valid) {
    b = a.q_batch_ids ? a.q_batch_ids[qi] : 0;
    valid = b >= 0 && b < a.batch;
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < NDIM; ++j) {
      q[j] = a.queries[static_cast<size_t>(qi) * a.q_nfeat + j];
      valid = valid && q[j] == q[j];
    }
  }
  const int mine = valid ? b : INT_MAX;
  int32_t *ro = a.rows + qi * a.nsample;
  float *oo = a.out_offsets ? a.out_offsets + qi * a.nsample * NDIM : nullptr;
  int cnt = 0, first_row = -1;
  float first_off[NDIM] = {};
  int cur = -1;
  for (int it = 0;; ++it) {
    const int next = next_scene(mine, cur, it, s_next);
    if (next == INT_MAX) break;                         // the same LDS words for every lane: uniform
    cur = next;
    int beg, end;
    scene_range(a.offsets, a.n_cap, next, beg, end);
    bool active = mine == next;
    for (int tile0 = beg; tile0 < end; tile0 += kSceneTile) {
      const int padded = stage_tile<NDIM>(a, tile0, end, s_pt);
      // kSceneAhead staged points at a time: their reads and distances are independent, a hit is rare
      for (int k0 = 0; k0 < padded && active; k0 += kSceneAhead) {
        float4 p[kSceneAhead];
        float d[kSceneAhead][NDIM];
        unsigned hits = 0u;
#pragma unroll
        for (int u = 0; u < kSceneAhead; ++u) p[u] = s_pt[k0 + u];
#pragma unroll
        for (int u = 0; u < kSceneAhead; ++u) {
          d[u][0] = p[u].x - q[0];
          d[u][1] = p[u].y - q[1];
          if (NDIM == 3) d[u][NDIM - 1] = p[u].z - q[NDIM - 1];
          hits |= dist2<NDIM>(d[u]) < a.r2 ? 1u << u : 0u;   // (false for an invalid point: its d2 is NaN)
        }
        if (hits == 0u) continue;
#pragma unroll
        for (int u = 0; u < kSceneAhead; ++u) {              // (ascending point index)
          if (!(hits >> u & 1u) || cnt >= a.nsample) continue;
          const int pi = __float_as_int(p[u].w);
          ro[cnt] = pi;
          if (oo) {
#pragma unroll
            for (int j = 0; j < NDIM; ++j) oo[cnt * NDIM + j] = d[u][j];
          }
          if (cnt == 0) {
            first_row = pi;
#pragma unroll
            for (int j = 0; j < NDIM; ++j) first_off[j] = d[u][j];
          }
          ++cnt;
        }
        active = cnt < a.nsample;
      }
      if (!__syncthreads_or(active ? 1 : 0)) break;     // no lane of this scene has room: uniform
    }
  }
  if (exists) {
    const bool pad = (a.flags & kFlagPadFirst) && cnt > 0;
    for (int s = cnt; s < a.nsample; ++s) {
      ro[s] = pad ? first_row : -1;
      if (oo) {
#pragma unroll
        for (int j = 0; j < NDIM; ++j) oo[s * NDIM + j] = pad ? first_off[j] : 0.f;
      }
    }
    a.count[qi] = cnt;
  }
}


// -------------------------------------------------------------------------------------------- sectors

constexpr int kMaxSectors = 64;
constexpr int kSectorBoxTile = 128;                  // boxes staged per tile of the RoI filter
static_assert(kSectorBoxTile <= kSceneBlock, "one lane stages one box");
static_assert(kMaxSectors <= kWave, "a wave holds a scene's segments, one per lane");

// the boundary directions (cos, sin)(2 pi k / S), built by the host (sector_table): a kernel argument, read with
// uniform indices
struct SectorTable {
  float c[kMaxSectors], s[kMaxSectors];
};

// The scene walk with the roles turned (as roi.hip): queries / m_cap / n_queries are the POINTS, points / nfeat /
// n_cap / offsets / list the boxes and the scene list over the box batch ids.
struct SectorArgs : SceneArgs {
  int sectors;
  float cx, cy, radius;
  SectorTable tab;
  int32_t *seg;
};

// The azimuth sector of (x, y) about (cx, cy): the boundaries at or past which the direction (a, b) = -(x - cx, y - cy)
// lies, counted by half turn and the sign of one cross product each.  No transcendental function.
__device__ __forceinline__ int sector_of(const SectorTable &tab, int S, float x, float y, float cx, float cy) {
  const float a = -(x - cx), b = -(y - cy);
  if (a == 0.f && b == 0.f) return 0;
  const int half = (b > 0.f || (b == 0.f && a > 0.f)) ? 0 : 1;
  int past = 0;
  for (int k = 0; k < S; ++k) {                         // (uniform: the table is read into scalar registers)
    const int hk = 2 * k >= S ? 1 : 0;
    const float cross = tab.c[k] * b - tab.s[k] * a;
    past += (half > hk || (half == hk && cross >= 0.f)) ? 1 : 0;
  }
  return max(past - 1, 0);                              // (0 boundaries: only with a cross product that is NaN)
}

// One lane per point.  ROI: the point is kept when it lies nearer to the NEAREST valid box centre of its scene than that
// box's half diagonal plus the radius; the boxes of a scene are staged as {centre, squared half diagonal}, x = NaN for an
// invalid one (its d2 is NaN: never the nearest).
template <int NDIM, bool ROI>
__global__ void __launch_bounds__(kSceneBlock)
sector_ids_kernel(SectorArgs a) {
  const long long qi = static_cast<long long>(blockIdx.x) * kSceneBlock + threadIdx.x;
  float q[NDIM];
  const int mine = load_scene_query<NDIM>(a, qi, q);    // (a lane without a valid point still takes every barrier)
  bool keep = mine != INT_MAX;
  if constexpr (ROI) {
    __shared__ float4 s_box[kSectorBoxTile];
    __shared__ int s_next[2][kSceneWaves];
    float best = __builtin_huge_valf(), best_r2 = 0.f;
    bool found = false;
    int cur = -1;
    for (int it = 0;; ++it) {
      const int next = next_scene(mine, cur, it, s_next);
      if (next == INT_MAX) break;                       // the same LDS words for every lane: uniform
      cur = next;
      int beg, end;
      scene_range(a.offsets, a.n_cap, next, beg, end);
      for (int tile0 = beg; tile0 < end; tile0 += kSectorBoxTile) {
        const int tn = min(kSectorBoxTile, end - tile0);
        if (static_cast<int>(threadIdx.x) < tn) {
          const int bi = a.list[tile0 + threadIdx.x];
          float v[7];
          bool ok = static_cast<unsigned>(bi) < static_cast<unsigned>(a.n_cap);
#pragma unroll
          for (int j = 0; j < 7; ++j) {
            v[j] = ok ? a.points[static_cast<size_t>(bi) * a.nfeat + j] : 0.f;
            ok = ok && finite(v[j]);
          }
          ok = ok && v[3] > 0.f && v[4] > 0.f && v[5] > 0.f;   // (the rule of box_frames_kernel, roi.hip)
          const float h[3] = {0.5f * v[3], 0.5f * v[4], 0.5f * v[5]};
          s_box[threadIdx.x] = make_float4(ok ? v[0] : __builtin_nanf(""), v[1], v[2], dist2<3>(h));
        }
        __syncthreads();
        if (mine == next) {
          for (int k = 0; k < tn; ++k) {                // (ascending box index: the strict compare keeps the lowest)
            const float4 bx = s_box[k];
            const float d[3] = {bx.x - q[0], bx.y - q[1], bx.z - q[NDIM - 1]};
            const float d2 = dist2<3>(d);
            const bool take = d2 < best;
            best = take ? d2 : best;
            best_r2 = take ? bx.w : best_r2;
            found = found || take;
          }
        }
        __syncthreads();                                // the tile is read before the next one is staged
      }
    }
    keep = keep && found && sqrtf(best) < sqrtf(best_r2) + a.radius;
  }
  if (qi < a.m_cap) a.seg[qi] = keep ? mine * a.sectors + sector_of(a.tab, a.sectors, q[0], q[1], a.cx, a.cy) : -1;
}

// -------------------------------------------------------------------------------------------- quotas

// One wave per scene, lane k its segment k: the segment's share of K in proportion to its points, rounded up, the
// exclusive prefix of the shares inside the scene and their sum.
__global__ void __launch_bounds__(kWave)
fps_quota_kernel(const int32_t *__restrict__ offsets, int n_cap, int S, int K, int32_t *__restrict__ quota,
                 int32_t *__restrict__ slot, int32_t *__restrict__ count) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long g = static_cast<long long>(b) * S + lane;
  long long nk = 0;
  if (lane < S) {
    int beg, end;
    scene_range(offsets, n_cap, static_cast<int>(g), beg, end);
    nk = end - beg;
  }
  long long n = nk;
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) n += __shfl_xor(n, m, kWave);
  long long share = 0;
  if (n > 0) {
    share = (nk * K + n - 1) / n;
    share = share < nk ? share : nk;
  }
  const unsigned q = static_cast<unsigned>(share);
  unsigned inc = q;                                     // (unsigned: offsets that overlap may wrap, never trap)
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const unsigned v = __shfl_up(inc, d, kWave);
    inc += lane >= d ? v : 0u;
  }
  if (lane < S) {
    quota[g] = static_cast<int32_t>(q);
    slot[g] = static_cast<int32_t>(inc - q);
  }
  if (lane == kWave - 1) count[b] = static_cast<int32_t>(inc);
}

// -------------------------------------------------------------------------------------------- segmented sampling

// fps_kernel with K read per segment: segment g samples min(quota[g], its valid points) points into its row at slot[g].
// Both device values are clamped to what the row holds, so no store leaves idx whatever they are.  An instantiation of
// its own: fps_kernel keeps its registers.
template <int NDIM>
__global__ void __launch_bounds__(kFpsBlock)
fps_segments_kernel(const float *__restrict__ points, int nfeat, int n_cap, const int32_t *__restrict__ offsets,
                    const int32_t *__restrict__ list, const int32_t *__restrict__ quota, const int32_t *__restrict__ slot,
                    int per_row, int row_stride, int max_quota, int32_t *idx, int32_t *__restrict__ count, FpsRec *recs) {
  __shared__ FpsShared sh;
  const int g = blockIdx.x;
  int beg, end;
  scene_range(offsets, n_cap, g, beg, end);
  const int n = end - beg;                              // uniform: the segment's own count
  const int at = slot ? min(max(slot[g], 0), row_stride) : 0;
  const int K = min(min(max(quota[g], 0), max_quota), row_stride - at);   // uniform loads
  if (n == 0 || K == 0) {                               // before the first barrier (idx holds -1 already)
    if (threadIdx.x == 0) count[g] = 0;
    return;
  }
  int32_t *out = idx + static_cast<long long>(g / per_row) * row_stride + at;
  if (n <= kFpsResident || recs == nullptr)             // (the host refuses n_cap > kFpsResident without scratch)
    fps_scene<NDIM, ResidentPoints<NDIM>>(sh, points, nfeat, n_cap, list + beg, min(n, kFpsResident), K, nullptr, out,
                                          count + g);
  else
    fps_scene<NDIM, StreamedPoints<NDIM>>(sh, points, nfeat, n_cap, list + beg, n, K, recs + beg, out, count + g);
}

// (cos, sin)(2 pi k / S) in float64 rounded to float32; the multiples of a quarter turn exactly
void sector_table(int S, SectorTable &tab) {
  static const float kAxis[4][2] = {{1.f, 0.f}, {0.f, 1.f}, {-1.f, 0.f}, {0.f, -1.f}};
  for (int k = 0; k < kMaxSectors; ++k) tab.c[k] = tab.s[k] = 0.f;
  for (int k = 0; k < S; ++k) {
    if (4 * k % S == 0) {
      tab.c[k] = kAxis[4 * k / S][0];
      tab.s[k] = kAxis[4 * k / S][1];
    } else {
      const double t = 2.0 * M_PI * static_cast<double>(k) / static_cast<double>(S);
      tab.c[k] = static_cast<float>(cos(t));
      tab.s[k] = static_cast<float>(sin(t));
    }
  }
}

// 0 = ok: the scratch of a sampling call over a cloud of n_cap points (ws set to nullptr where none is needed)
int check_fps_ws(int n_cap, int batch, int ndim, void *&ws, size_t ws_bytes) {
  if (n_cap > kFpsResident) {                           // a scene may need the streamed tier
    SPX_CHECK(ws && ws_bytes >= spx_fps_ws_bytes(n_cap, batch, ndim), "workspace too small: %zu < %zu", ws_bytes,
              spx_fps_ws_bytes(n_cap, batch, ndim));
    SPX_CHECK(aligned_to(ws, 16), "workspace not aligned to 16 bytes");
  } else {
    ws = nullptr;
  }
  return 0;
}

}  // namespace
}  // namespace spx

// -------------------------------------------------------------------------------------------- host side

extern "C" {

int spx_fps_resident_points(void) { return spx::kFpsResident; }

size_t spx_fps_ws_bytes(int n_cap, int batch, int ndim) {
  if ((ndim != 2 && ndim != 3) || n_cap < 0 || batch < 1) return 0;
  return spx::align_up(static_cast<size_t>(n_cap) * sizeof(spx::FpsRec), 256);
}

int spx_fps(const float *points, int nfeat, int n_cap, int ndim, const int32_t *offsets, const int32_t *list, int batch,
            int num_samples, int32_t *idx, int32_t *count, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_scenes(ndim, nfeat, n_cap, batch)) return rc;
  SPX_CHECK(num_samples >= 1 && num_samples <= kMaxSamples, "num_samples must be in 1 .. %d, got %d", kMaxSamples,
            num_samples);
  SPX_CHECK(static_cast<long long>(batch) * num_samples < 0x80000000LL, "batch * num_samples must stay below 2^31, got %d x %d",
            batch, num_samples);
  SPX_CHECK(offsets && idx && count && (n_cap == 0 || (points && list)), "points / offsets / list / idx / count is NULL");
  SPX_CHECK(aligned_to(points, 4) && aligned_to(offsets, 4) && aligned_to(list, 4) && aligned_to(idx, 4) &&
                aligned_to(count, 4), "pointer not aligned to its elements");
  if (int rc = check_fps_ws(n_cap, batch, ndim, ws, ws_bytes)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  FpsRec *recs = static_cast<FpsRec *>(ws);
  if (ndim == 3)
    hipLaunchKernelGGL((fps_kernel<3>), dim3(batch), dim3(kFpsBlock), 0, s, points, nfeat, n_cap, offsets, list, num_samples,
                       idx, count, recs);
  else
    hipLaunchKernelGGL((fps_kernel<2>), dim3(batch), dim3(kFpsBlock), 0, s, points, nfeat, n_cap, offsets, list, num_samples,
                       idx, count, recs);
  SPX_LAUNCH_CHECK();
  spx::count(kSampleFps);
  return 0;
}

int spx_sector_max(void) { return spx::kMaxSectors; }
int spx_sector_box_tile(void) { return spx::kSectorBoxTile; }

int spx_sector_table(int num_sectors, float *table_h) {
  using namespace spx;
  SPX_CHECK(num_sectors >= 1 && num_sectors <= kMaxSectors, "num_sectors must be in 1 .. %d, got %d", kMaxSectors,
            num_sectors);
  SPX_CHECK(table_h, "table is NULL");
  SectorTable tab;
  sector_table(num_sectors, tab);
  for (int k = 0; k < num_sectors; ++k) {
    table_h[2 * k] = tab.c[k];
    table_h[2 * k + 1] = tab.s[k];
  }
  return 0;
}

int spx_sector_ids(const float *points, int nfeat, const int32_t *batch_ids, int n_cap, const int32_t *n_points_dev,
                   int ndim, int batch, int num_sectors, float cx, float cy, int roi_filter, const float *boxes,
                   int box_nfeat, int m_cap, const int32_t *box_offsets, const int32_t *box_list, float radius,
                   int32_t *seg, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_scenes(ndim, nfeat, n_cap, batch)) return rc;
  SPX_CHECK(num_sectors >= 1 && num_sectors <= kMaxSectors, "num_sectors must be in 1 .. %d, got %d", kMaxSectors,
            num_sectors);
  SPX_CHECK(static_cast<long long>(batch) * num_sectors < 0x7fffffffLL, "batch * num_sectors must stay below 2^31 - 1, got %d x %d",
            batch, num_sectors);
  SPX_CHECK(isfinite(cx) && isfinite(cy), "the centre must be finite");
  SPX_CHECK(roi_filter == 0 || roi_filter == 1, "roi_filter must be 0 or 1, got %d", roi_filter);
  if (roi_filter) {
    SPX_CHECK(ndim == 3, "the RoI filter needs ndim 3, got %d", ndim);
    SPX_CHECK(m_cap >= 0, "bad box counts %d", m_cap);
    SPX_CHECK(box_nfeat >= 7, "boxes need at least 7 columns (x, y, z, dx, dy, dz, heading), got %d", box_nfeat);
    SPX_CHECK(radius >= 0.f && isfinite(radius), "the radius must be finite and >= 0 (and no NaN)");
  }
  if (n_cap == 0) return 0;
  SPX_CHECK(points && seg, "points / seg is NULL");
  SPX_CHECK(aligned_to(points, 4) && aligned_to(batch_ids, 4) && aligned_to(n_points_dev, 4) && aligned_to(seg, 4),
            "pointer not aligned to its elements");
  SectorArgs a = {};
  a.queries = points, a.q_nfeat = nfeat, a.q_batch_ids = batch_ids, a.m_cap = n_cap, a.n_queries = n_points_dev;
  a.batch = batch, a.sectors = num_sectors, a.cx = cx, a.cy = cy, a.seg = seg;
  sector_table(num_sectors, a.tab);
  if (roi_filter) {
    SPX_CHECK(box_offsets && (m_cap == 0 || (boxes && box_list)), "boxes / box_offsets / box_list is NULL");
    SPX_CHECK(aligned_to(boxes, 4) && aligned_to(box_offsets, 4) && aligned_to(box_list, 4),
              "pointer not aligned to its elements");
    a.points = boxes, a.nfeat = box_nfeat, a.n_cap = m_cap, a.offsets = box_offsets, a.list = box_list, a.radius = radius;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((static_cast<long long>(n_cap) + kSceneBlock - 1) / kSceneBlock));
  if (roi_filter)
    hipLaunchKernelGGL((sector_ids_kernel<3, true>), grid, dim3(kSceneBlock), 0, s, a);
  else if (ndim == 3)
    hipLaunchKernelGGL((sector_ids_kernel<3, false>), grid, dim3(kSceneBlock), 0, s, a);
  else
    hipLaunchKernelGGL((sector_ids_kernel<2, false>), grid, dim3(kSceneBlock), 0, s, a);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_fps_quota(const int32_t *offsets, int n_cap, int batch, int num_sectors, int num_samples, int32_t *quota,
                  int32_t *slot, int32_t *count, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(n_cap >= 0, "bad point counts %d", n_cap);
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  SPX_CHECK(num_sectors >= 1 && num_sectors <= kMaxSectors, "num_sectors must be in 1 .. %d, got %d", kMaxSectors,
            num_sectors);
  SPX_CHECK(num_samples >= 1 && num_samples <= kMaxSamples, "num_samples must be in 1 .. %d, got %d", kMaxSamples,
            num_samples);
  SPX_CHECK(static_cast<long long>(batch) * num_sectors < 0x7fffffffLL, "batch * num_sectors must stay below 2^31 - 1, got %d x %d",
            batch, num_sectors);
  SPX_CHECK(offsets && quota && slot && count, "offsets / quota / slot / count is NULL");
  SPX_CHECK(aligned_to(offsets, 4) && aligned_to(quota, 4) && aligned_to(slot, 4) && aligned_to(count, 4),
            "pointer not aligned to its elements");
  hipLaunchKernelGGL(fps_quota_kernel, dim3(batch), dim3(kWave), 0, static_cast<hipStream_t>(stream), offsets, n_cap,
                     num_sectors, num_samples, quota, slot, count);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_fps_segments(const float *points, int nfeat, int n_cap, int ndim, const int32_t *offsets, const int32_t *list,
                     int groups, const int32_t *quota, const int32_t *slot, int groups_per_row, int row_stride,
                     int max_quota, int32_t *idx, int32_t *count, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(groups >= 1, "groups must be >= 1, got %d", groups);
  if (int rc = check_scenes(ndim, nfeat, n_cap, groups)) return rc;
  SPX_CHECK(groups_per_row >= 1 && groups % groups_per_row == 0, "groups (%d) must be a multiple of groups_per_row (%d >= 1)",
            groups, groups_per_row);
  SPX_CHECK(max_quota >= 1 && max_quota <= kMaxSamples, "max_quota must be in 1 .. %d, got %d", kMaxSamples, max_quota);
  SPX_CHECK(row_stride >= 1, "row_stride must be >= 1, got %d", row_stride);
  const long long rows = groups / groups_per_row;
  SPX_CHECK(rows * row_stride < 0x80000000LL, "rows * row_stride must stay below 2^31, got %lld x %d", rows, row_stride);
  SPX_CHECK(offsets && quota && idx && count && (n_cap == 0 || (points && list)),
            "points / offsets / list / quota / idx / count is NULL");
  SPX_CHECK(aligned_to(points, 4) && aligned_to(offsets, 4) && aligned_to(list, 4) && aligned_to(quota, 4) &&
                aligned_to(slot, 4) && aligned_to(idx, 4) && aligned_to(count, 4), "pointer not aligned to its elements");
  if (int rc = check_fps_ws(n_cap, groups, ndim, ws, ws_bytes)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  FillList fills;                                       // the slots no segment writes hold -1
  fills.add(idx, static_cast<size_t>(rows * row_stride) * 4, 0xffffffffu);
  SPX_HIP(fills.launch(s));
  FpsRec *recs = static_cast<FpsRec *>(ws);
  if (ndim == 3)
    hipLaunchKernelGGL((fps_segments_kernel<3>), dim3(groups), dim3(kFpsBlock), 0, s, points, nfeat, n_cap, offsets, list,
                       quota, slot, groups_per_row, row_stride, max_quota, idx, count, recs);
  else
    hipLaunchKernelGGL((fps_segments_kernel<2>), dim3(groups), dim3(kFpsBlock), 0, s, points, nfeat, n_cap, offsets, list,
                       quota, slot, groups_per_row, row_stride, max_quota, idx, count, recs);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_ball_query(const float *queries, int q_nfeat, const int32_t *q_batch_ids, int m_cap, const int32_t *n_queries_dev,
                   const float *points, int nfeat, int n_cap, int ndim, const int32_t *offsets, const int32_t *list,
                   int batch, int nsample, float r2, int flags, int32_t *rows, int32_t *count, float *out_offsets,
                   spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(nsample >= 1 && nsample <= kMaxSample, "nsample must be in 1 .. %d, got %d", kMaxSample, nsample);
  SPX_CHECK(r2 >= 0.f, "the squared radius must be >= 0 (and no NaN)");
  const BallArgs a = {{queries, q_nfeat, q_batch_ids, m_cap, n_queries_dev, points, nfeat, n_cap, offsets, list, batch},
                      nsample, r2, flags, rows, count, out_offsets};
  if (int rc = check_scene_query(a, ndim, nsample, flags, rows, count, {out_offsets})) return rc;
  if (m_cap == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((static_cast<long long>(m_cap) + kSceneBlock - 1) / kSceneBlock));
  if (ndim == 3)
    hipLaunchKernelGGL((ball_query_kernel<3>), grid, dim3(kSceneBlock), 0, s, a);
  else
    hipLaunchKernelGGL((ball_query_kernel<2>), grid, dim3(kSceneBlock), 0, s, a);
  SPX_LAUNCH_CHECK();
  spx::count(kSampleBallQuery);
  return 0;
}

}  // extern "C"
