// What the units over raw points share (sample.hip, knn.hip; the distance and the pad flag also query.hip): the
// squared distance, the validity of a coordinate and of a point, and the SCENE WALK of the one-lane-per-query kernels
// (ball_query_kernel, knn_query_kernel) -- workgroups of 256 consecutive queries walk the scenes of their valid queries
// in ascending order and stage each scene's points in LDS, tiles of 1024 {x, y, z, index} records padded to a multiple of
// the eight a lane tests together -- with the host checks of such a call.  A query is VALID when it lies below
// min(*n_queries, m_cap), its batch id is in [0, batch) and its first ndim coordinates are finite (load_scene_query).
// ball_query_kernel keeps its own copy of that load with a NaN-only test of the coordinates: its results are the same
// (an infinite query coordinate makes every d2 +inf or NaN, neither of which is < r2 even for r2 = +inf: count 0 either
// way), and with the finite test its code moved enough to cost 0.6 % of a call (profiles/scene_walk_refactor_probe.json).
// The tile loop and what consumes a batch of eight stay in each kernel: the ball query leaves a scene early, the k-NN
// gates on its worst kept key and skips tiles per wave; a walker over a callback would branch on its caller.  next_scene
// and stage_tile hold a barrier each: call them from control flow uniform over the workgroup.  Internal linkage.
#pragma once
#include <limits.h>

#include "common.h"
#include "piece.h"

// no multiply-add pair of this header may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kSceneBlock = 256, kSceneWaves = kSceneBlock / kWave, kSceneTile = 1024;
constexpr int kSceneAhead = 8;                       // staged points a lane tests together
static_assert(kSceneTile % kSceneAhead == 0, "a padded tile stays inside the staged array");
constexpr int kFlagPadFirst = 2;

typedef unsigned long long u64;

template <int NDIM> __device__ __forceinline__ float dist2(const float (&d)[NDIM]) {
  float s = d[0] * d[0] + d[1] * d[1];
  if (NDIM == 3) s = s + d[NDIM - 1] * d[NDIM - 1];
  return s;
}

__device__ __forceinline__ bool finite(float v) { return fabsf(v) < __builtin_huge_valf(); }      // (false for NaN)

// Position `pos` of a scene (its list starts at list_b): the point's coordinates; false for an index outside the
// points and for a coordinate that is not finite.
template <int NDIM>
__device__ __forceinline__ bool load_point(const float *__restrict__ points, int nfeat, int n_cap,
                                           const int32_t *__restrict__ list_b, int pos, float (&p)[NDIM], int &pi) {
  pi = list_b[pos];
  bool ok = static_cast<unsigned>(pi) < static_cast<unsigned>(n_cap);
#pragma unroll
  for (int j = 0; j < NDIM; ++j) {
    p[j] = ok ? points[static_cast<size_t>(pi) * nfeat + j] : 0.f;
    ok = ok && finite(p[j]);
  }
  return ok;
}

// the positions [beg, end) of scene b in the list: offsets checked, not trusted
__device__ __forceinline__ void scene_range(const int32_t *__restrict__ offsets, int n_cap, int b, int &beg, int &end) {
  beg = offsets[b];
  end = offsets[b + 1];
  beg = min(max(beg, 0), n_cap);
  end = min(max(end, beg), n_cap);
}

// The head of the arguments of a kernel that walks scenes (BallArgs, KnnArgs).
struct SceneArgs {
  const float *queries;
  int q_nfeat;
  const int32_t *q_batch_ids;
  int m_cap;
  const int32_t *n_queries;
  const float *points;
  int nfeat, n_cap;
  const int32_t *offsets, *list;
  int batch;
};

// Query qi, the lane's: its scene, or INT_MAX for a lane without a valid query (the rule above); q: its coordinates.
template <int NDIM> __device__ __forceinline__ int load_scene_query(const SceneArgs &a, long long qi, float (&q)[NDIM]) {
  const int nq = a.n_queries ? min(*a.n_queries, a.m_cap) : a.m_cap;
  bool valid = qi < nq;
  int b = -1;
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
      valid = valid && finite(q[j]);
    }
  }
  return valid ? b : INT_MAX;
}

// The lowest scene above `cur` among the workgroup's queries (`mine`: the lane's), INT_MAX once there is none: the same
// LDS words for every lane, so the answer is uniform.  One barrier; trip `it` uses the words of its parity, so a lane
// still reading the last answer is not overtaken.
__device__ __forceinline__ int next_scene(int mine, int cur, int it, int (&s_next)[2][kSceneWaves]) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int cand = mine > cur ? mine : INT_MAX;
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) cand = min(cand, __shfl_xor(cand, m, kWave));
  if (lane == 0) s_next[it & 1][wave] = cand;
  __syncthreads();
  int next = INT_MAX;
#pragma unroll
  for (int w = 0; w < kSceneWaves; ++w) next = min(next, s_next[it & 1][w]);
  return next;
}

// Stages positions [tile0, min(tile0 + kSceneTile, end)) of the list as {x, y, z, the point index as bits}, x = NaN for
// an invalid point and for the padding, and takes the barrier behind the stores.  Returns the staged count: the tile's,
// rounded up to a multiple of kSceneAhead.
template <int NDIM>
__device__ __forceinline__ int stage_tile(const SceneArgs &a, int tile0, int end, float4 (&s_pt)[kSceneTile]) {
  const int tn = min(kSceneTile, end - tile0);
  const int padded = (tn + kSceneAhead - 1) / kSceneAhead * kSceneAhead;        // (the tile is a multiple of kSceneAhead)
  for (int k = threadIdx.x; k < padded; k += kSceneBlock) {
    float p[NDIM] = {};
    int pi = -1;
    const bool ok = k < tn && load_point<NDIM>(a.points, a.nfeat, a.n_cap, a.list + tile0, k, p, pi);
    s_pt[k] = make_float4(ok ? p[0] : __builtin_nanf(""), p[1], NDIM == 3 ? p[NDIM - 1] : 0.f, __int_as_float(pi));
  }
  __syncthreads();
  return padded;
}

// -------------------------------------------------------------------------------------------- host side

// 0 = ok: the checks of a scene list that need no pointer
inline int check_scenes(int ndim, int nfeat, int n_cap, int batch) {
  SPX_CHECK(ndim == 2 || ndim == 3, "ndim must be 2 or 3, got %d", ndim);
  SPX_CHECK(n_cap >= 0, "bad point counts %d", n_cap);
  SPX_CHECK(nfeat >= ndim, "points need at least %d columns, got %d", ndim, nfeat);
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  return 0;
}

// 0 = ok: the checks of m_cap queries over a scene list with `entries` slots each, every one that needs no pointer
// before any pointer is looked at; a call without queries is done before that (it launches nothing).  `tables`: the
// fp32 outputs a caller may leave out.
inline int check_scene_query(const SceneArgs &a, int ndim, int entries, int flags, const int32_t *rows,
                             const int32_t *count, std::initializer_list<const float *> tables) {
  if (int rc = check_scenes(ndim, a.nfeat, a.n_cap, a.batch)) return rc;
  SPX_CHECK(a.m_cap >= 0, "bad query counts %d", a.m_cap);
  SPX_CHECK(a.q_nfeat >= ndim, "queries need at least %d columns, got %d", ndim, a.q_nfeat);
  SPX_CHECK(static_cast<long long>(a.m_cap) * entries < 0x80000000LL,
            "m_cap * entries per query must stay below 2^31, got %d x %d", a.m_cap, entries);
  SPX_CHECK((flags & ~kFlagPadFirst) == 0, "flags must be 0 or pad first (2), got %d", flags);
  if (a.m_cap == 0) return 0;
  SPX_CHECK(a.queries && rows && count && a.offsets && (a.n_cap == 0 || (a.points && a.list)),
            "queries / points / offsets / list / rows / count is NULL");
  bool aligned = aligned_to(a.queries, 4) && aligned_to(a.points, 4) && aligned_to(a.offsets, 4) && aligned_to(a.list, 4) &&
                 aligned_to(rows, 4) && aligned_to(count, 4);
  for (const float *t : tables) aligned = aligned && aligned_to(t, 4);
  SPX_CHECK(aligned, "pointer not aligned to its elements");
  return 0;
}

}  // namespace
}  // namespace spx
