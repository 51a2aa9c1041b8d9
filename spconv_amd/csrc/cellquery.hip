// Ball query and radius-limited k-nearest neighbours over the CELL INDEX of a point cloud (spx_cell_records,
// spx_ball_query_cells, spx_knn_query_cells): what spx_ball_query and spx_knn_query return, bit for bit, from
// O(points in 27 cells) records per query instead of O(points in the scene).  The index is cellrec.h's: cells of edge
// radius * (1 + 2^-6) in key order, the points as 16-byte records in cell order; a point within the radius of a query
// lies at most one cell from the query's on every axis (DESIGN.md sections 3.43 and 3.44, the second for a query
// outside the range).
//
//   group     a query belongs to 16 lanes: 4 queries per wave, 16 per workgroup of 256.  Every loop is WAVE-UNIFORM: it
//             runs while any group of the wave has work and idle groups are predicated off, so no ballot and no LDS fence
//             sits in divergent flow.  There is no workgroup barrier in the kernel.
//   cell      floorf((q - lo) / vsize) per axis, the voxeliser's operations, clamped in float to [-1, grid]: a query may
//             lie anywhere; one more than a cell outside the grid meets only points its distance test turns down.
//   lines     lanes 0 .. 8 of the group resolve one (dz, dy) line of the 3 x 3 x 3 stencil each: its up to three cells
//             are consecutive keys, hence ONE run [beg, end) of records (line_run: two rank-map lookups, two offsets),
//             clamped into the records that exist.  The non-empty runs are handed round the group by shuffles.
//   walk      16 records of the current run per step, one 16-byte load per lane (256 contiguous bytes per group);
//             d = p - q, d2 = (d0 * d0 + d1 * d1) + d2 * d2, hit = d2 < r2: spx_ball_query's predicate.
//   keys      a hit is a KEY -- the point index (ball query: the first nsample in ascending index are the nsample
//             smallest keys) or d2 bits << 32 | index (k-NN: spx_knn_query's total order).  It takes its slot in the
//             INCOMING half of the group's LDS buffer from the group's share of a wave ballot and a prefix popcount.
//   compact   when an incoming half cannot take 16 more keys, and once at the end: every key of both halves is ranked by
//             counting the smaller keys (keys are distinct: ranks are unique), keys of rank < nsample move to slot `rank`
//             of the KEPT half -- selection and sort in one pass, no atomics, no dependence on visiting order.  A lane
//             holds its 2 .. 16 keys and their ranks in registers (the tier follows the wave's longest buffer) while one
//             pass over the buffer reads every key once.  Once the kept half is full its largest key gates the hit test.
//   output    the last compaction leaves the result in slot order: rows, count, offsets p - q re-read from the point
//             (the same float32 operation: the same bits), dist2 and pointnet2's weights for the k-NN.
// Every index read from a table is range-checked before it addresses anything.
#include <math.h>

#include "cellrec.h"
#include "common.h"
#include "rankmap.h"
#include "scenes.h"

// the predicate is spx_ball_query's: no multiply-add pair of this unit may be contracted into an FMA
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kCqBlock = 256;
constexpr int kCqLanes = 16;                          // lanes of a query's group
constexpr int kCqGroups = kCqBlock / kCqLanes;        // queries of a workgroup
constexpr int kCqHalf = 128;                          // keys of a half: the largest nsample
constexpr int kCqMaxK = 64;
static_assert(kWave % kCqLanes == 0 && 2 * kCqHalf / kCqLanes == 16, "a lane ranks at most 16 keys");

// -------------------------------------------------------------------------------------------- records

struct CellRecordArgs {
  const float *points;
  int nfeat, n_cap;
  const int32_t *n_points, *batch_ids;
  int batch;
  float lo[3], hi[3];
  const int32_t *cell_rows, *cell_offsets, *cell_list;
  ClRec *recs;
};

// one lane per position of cell_list: cluster_records_kernel without labels, mask and parents
__global__ void __launch_bounds__(kCqBlock)
cell_records_kernel(CellRecordArgs a) {
  const long long pos = static_cast<long long>(blockIdx.x) * kCqBlock + threadIdx.x;
  if (pos >= a.n_cap) return;
  const int total = min(max(a.cell_offsets[a.n_cap], 0), a.n_cap);      // points that have a cell
  ClRec r = {__builtin_nanf(""), 0.f, 0.f, -1};
  if (pos < total) {
    const int i = a.cell_list[pos];
    const int np = a.n_points ? min(*a.n_points, a.n_cap) : a.n_cap;
    if (i >= 0 && i < np) {
      const int b = a.batch_ids ? a.batch_ids[i] : 0;
      const float *p = a.points + static_cast<size_t>(i) * a.nfeat;
      const float x = p[0], y = p[1], z = p[2];
      bool ok = b >= 0 && b < a.batch;
      ok = ok && x >= a.lo[0] && x < a.hi[0] && y >= a.lo[1] && y < a.hi[1] && z >= a.lo[2] && z < a.hi[2];   // (false for NaN)
      const int v = a.cell_rows[i];
      if (ok && v >= 0 && v < a.n_cap) r = {x, y, z, i};
    }
  }
  a.recs[pos] = r;
}

// -------------------------------------------------------------------------------------------- query

struct CellQueryArgs : CellLookup {
  const float *queries;
  int q_nfeat;
  const int32_t *q_batch_ids;
  int m_cap;
  const int32_t *n_queries;
  const float *points;
  int nfeat;
  const ClRec *recs;
  float lo[3], vsize, r2;
  int nsample, width, flags;
  float eps;
  int32_t *rows, *count;
  float *dist2, *weights, *out_offsets;
};

template <bool KNN> struct CqKey {
  typedef uint32_t T;
  static constexpr T kMax = 0xffffffffu;
};
template <> struct CqKey<true> {
  typedef u64 T;
  static constexpr T kMax = ~0ull;
};

// the LDS traffic of the lanes of a wave, ordered for the compiler (the hardware runs a wave's LDS operations in order)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// where key e of a group's n_kept + n_in keys lives: the kept half from 0, the incoming half from kCqHalf
__device__ __forceinline__ int key_slot(int e, int n_kept) { return e < n_kept ? e : kCqHalf + (e - n_kept); }

// One compaction with M keys per lane (16 M >= wave_total, the longest buffer of the wave: a uniform bound).
template <int M, typename K>
__device__ __forceinline__ void compact_keys(K *buf, int sub, int n_kept, int n_in, int nsample, int wave_total, K none) {
  const int total = n_kept + n_in;
  K mine[M];
  int rank[M];
#pragma unroll
  for (int u = 0; u < M; ++u) {
    const int e = sub + u * kCqLanes;
    mine[u] = e < total ? buf[key_slot(e, n_kept)] : none;
    rank[u] = 0;
  }
  for (int j = 0; j < wave_total; ++j) {              // (every lane of the group reads the same word: a broadcast)
    const K kj = j < total ? buf[key_slot(j, n_kept)] : none;
#pragma unroll
    for (int u = 0; u < M; ++u) rank[u] += kj < mine[u] ? 1 : 0;
  }
  wave_lds_fence();                                   // every key is read before the kept half is written
#pragma unroll
  for (int u = 0; u < M; ++u)
    if (sub + u * kCqLanes < total && rank[u] < nsample) buf[rank[u]] = mine[u];
  wave_lds_fence();
}

template <bool KNN>
__global__ void __launch_bounds__(kCqBlock)
cell_query_kernel(CellQueryArgs a) {
  typedef typename CqKey<KNN>::T K;
  constexpr K kNone = CqKey<KNN>::kMax;
  __shared__ K s_keys[kCqGroups][2 * kCqHalf];
  const int sub = threadIdx.x & (kCqLanes - 1), group = threadIdx.x / kCqLanes;
  const int gbase = (threadIdx.x & (kWave - 1)) & ~(kCqLanes - 1);
  K *buf = s_keys[group];
  const long long qi = static_cast<long long>(blockIdx.x) * kCqGroups + group;

  // the query: spx_ball_query turns down NaN coordinates only, spx_knn_query takes finite ones only
  const int nq = a.n_queries ? min(*a.n_queries, a.m_cap) : a.m_cap;
  bool valid = qi < nq;
  int b = 0;
  float q[3] = {0.f, 0.f, 0.f};
  if (valid) {
    b = a.q_batch_ids ? a.q_batch_ids[qi] : 0;
    valid = b >= 0 && b < a.batch;
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      q[j] = a.queries[static_cast<size_t>(qi) * a.q_nfeat + j];
      valid = valid && (KNN ? finite(q[j]) : q[j] == q[j]);
    }
  }
  int c[3];                                           // the query's cell by point column (x, y, z), in [-1, grid]
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float cell = floorf((q[j] - a.lo[j]) / a.vsize);
    c[j] = static_cast<int>(fminf(fmaxf(cell, -1.f), static_cast<float>(a.dims[2 - j])));
  }

  // lanes 0 .. 8: the run of one (dz, dy) line each
  int beg = 0, end = 0;
  if (valid && sub < 9) {
    const int zz = c[2] + sub / 3 - 1, yy = c[1] + sub % 3 - 1;
    const int x0 = max(c[0] - 1, 0), x1 = min(c[0] + 1, a.dims[2] - 1);
    if (static_cast<unsigned>(zz) < static_cast<unsigned>(a.dims[0]) &&
        static_cast<unsigned>(yy) < static_cast<unsigned>(a.dims[1]) && x0 <= x1) {
      line_run(a, b, zz, yy, x0, x1, beg, end);
      const int total = min(max(a.cell_offsets[a.n_cap], 0), a.n_cap);
      beg = min(max(beg, 0), total);
      end = min(max(end, beg), total);
    }
  }
  unsigned lines = static_cast<unsigned>(__ballot(end > beg) >> gbase) & 0x1ffu;     // the group's runs with records

  int n_kept = 0, n_in = 0;
  K gate = kNone;                                     // once the kept half is full: its largest key

  // ranks and moves the keys of every group of the wave; called from uniform flow
  auto compact = [&]() {
    int wave_total = n_kept + n_in;
    wave_total = max(wave_total, __shfl_xor(wave_total, 16, kWave));
    wave_total = max(wave_total, __shfl_xor(wave_total, 32, kWave));
    wave_total = __builtin_amdgcn_readfirstlane(wave_total);
    wave_lds_fence();                                 // the appended keys are in LDS
    if (wave_total <= 2 * kCqLanes)
      compact_keys<2, K>(buf, sub, n_kept, n_in, a.nsample, wave_total, kNone);
    else if (wave_total <= 4 * kCqLanes)
      compact_keys<4, K>(buf, sub, n_kept, n_in, a.nsample, wave_total, kNone);
    else if (wave_total <= 8 * kCqLanes)
      compact_keys<8, K>(buf, sub, n_kept, n_in, a.nsample, wave_total, kNone);
    else
      compact_keys<16, K>(buf, sub, n_kept, n_in, a.nsample, wave_total, kNone);
    n_kept = min(n_kept + n_in, a.nsample);
    n_in = 0;
    if (n_kept == a.nsample) gate = buf[a.nsample - 1];
  };

  int cur = 0, cur_end = 0;
  for (;;) {
    // a group whose run is spent takes its next one (every lane takes part in the shuffles)
    const int line = lines ? __ffs(lines) - 1 : 0;
    const int nb = __shfl(beg, gbase + line, kWave), ne = __shfl(end, gbase + line, kWave);
    if (cur >= cur_end && lines) {
      lines &= lines - 1u;
      cur = nb;
      cur_end = ne;
    }
    if (__ballot(cur < cur_end) == 0ull) break;       // no group of the wave has records left: uniform
    const int pos = cur + sub;
    bool hit = false;
    K key = kNone;
    if (pos < cur_end) {
      const ClRec p = a.recs[pos];
      float d[3];
      d[0] = p.x - q[0];
      d[1] = p.y - q[1];
      d[2] = p.z - q[2];
      const float d2 = dist2<3>(d);
      key = KNN ? static_cast<K>((static_cast<u64>(__float_as_uint(d2)) << 32) | static_cast<uint32_t>(p.idx))
                : static_cast<K>(static_cast<uint32_t>(p.idx));
      hit = d2 < a.r2 && static_cast<unsigned>(p.idx) < static_cast<unsigned>(a.n_cap) && key < gate;   // (NaN: no hit)
    }
    cur += kCqLanes;
    const unsigned hits = static_cast<unsigned>(__ballot(hit) >> gbase) & 0xffffu;
    if (hit) buf[kCqHalf + n_in + __popc(hits & ((1u << sub) - 1u))] = key;
    n_in += __popc(hits);
    if (__ballot(n_in > kCqHalf - kCqLanes) != 0ull) compact();      // some incoming half cannot take a step more
  }
  compact();

  if (qi >= a.m_cap) return;
  const int cnt = n_kept;
  const bool pad = (a.flags & kFlagPadFirst) && cnt > 0;
  const K first = cnt > 0 ? buf[0] : K(0);
  float norm = 1.f;
  if (KNN && a.weights) {                             // r_0 + r_1 + ... in ascending slot, by every lane of the group
    for (int s = 0; s < cnt; ++s) {
      const float r = 1.f / (sqrtf(__uint_as_float(static_cast<uint32_t>(static_cast<u64>(buf[s]) >> 32))) + a.eps);
      norm = s == 0 ? r : norm + r;
    }
  }
  const long long base = qi * a.width;
  for (int s = sub; s < a.width; s += kCqLanes) {
    const bool live = s < cnt, has = live || (pad && s < a.nsample);
    const K key = live ? buf[s] : first;
    const int pi = has ? static_cast<int>(static_cast<uint32_t>(key)) : -1;
    a.rows[base + s] = pi;
    if (KNN) {
      const float d2 = has ? __uint_as_float(static_cast<uint32_t>(static_cast<u64>(key) >> 32)) : 0.f;
      if (a.dist2) a.dist2[base + s] = d2;
      if (a.weights) a.weights[base + s] = live ? (1.f / (sqrtf(d2) + a.eps)) / norm : 0.f;
    }
    if (a.out_offsets) {
      const bool at = has && static_cast<unsigned>(pi) < static_cast<unsigned>(a.n_cap);
#pragma unroll
      for (int j = 0; j < 3; ++j)
        a.out_offsets[(base + s) * 3 + j] = at ? a.points[static_cast<size_t>(pi) * a.nfeat + j] - q[j] : 0.f;
    }
  }
  if (sub == 0) a.count[qi] = cnt;
}

// -------------------------------------------------------------------------------------------- host side

int check_cell_grid(int n_cap, int batch, const int *grid_zyx_h) {
  SPX_CHECK(n_cap >= 0 && n_cap <= kCellMaxPoints, "n_cap must be in 0 .. %d, got %d", kCellMaxPoints, n_cap);
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  SPX_CHECK(grid_zyx_h, "the grid is NULL");
  for (int j = 0; j < 3; ++j)
    SPX_CHECK(grid_zyx_h[j] >= 1 && grid_zyx_h[j] <= kCellMaxAxis, "grid axis %d must hold 1 .. %d cells, got %d", j,
              kCellMaxAxis, grid_zyx_h[j]);
  return 0;
}

// The checks and the launch of both queries; k-NN: knn = true, nsample = k.
int cell_query(bool knn, const float *queries, int q_nfeat, const int32_t *q_batch_ids, int m_cap,
               const int32_t *n_queries_dev, const float *points, int nfeat, int n_cap, int batch, const int *grid_zyx_h,
               const float *lo_xyz_h, float vsize, const int32_t *cell_offsets, const void *rankmap, size_t rankmap_bytes,
               const void *records, int nsample, int width, float r2, float eps, int flags, int32_t *rows, int32_t *count,
               float *dist2, float *weights, float *out_offsets, spx_stream_t stream) {
  if (int rc = check_cell_grid(n_cap, batch, grid_zyx_h)) return rc;
  SPX_CHECK(m_cap >= 0, "bad query counts %d", m_cap);
  SPX_CHECK(q_nfeat >= 3 && nfeat >= 3, "queries and points need at least 3 columns, got %d and %d", q_nfeat, nfeat);
  if (knn)
    SPX_CHECK(nsample >= 1 && nsample <= kCqMaxK, "k must be in 1 .. %d, got %d", kCqMaxK, nsample);
  else
    SPX_CHECK(nsample >= 1 && nsample <= kCqHalf, "nsample must be in 1 .. %d, got %d", kCqHalf, nsample);
  SPX_CHECK(width >= nsample, "width must be >= k, got %d < %d", width, nsample);
  SPX_CHECK(static_cast<long long>(m_cap) * width < 0x80000000LL, "m_cap * entries per query must stay below 2^31, got %d x %d",
            m_cap, width);
  SPX_CHECK(eps >= 0.f && eps < __builtin_huge_valf(), "eps must be finite and >= 0");
  SPX_CHECK((flags & ~kFlagPadFirst) == 0, "flags must be 0 or pad first (2), got %d", flags);
  SPX_CHECK(lo_xyz_h && isfinite(lo_xyz_h[0]) && isfinite(lo_xyz_h[1]) && isfinite(lo_xyz_h[2]), "the lows of the range are not finite");
  SPX_CHECK(vsize > 0.f && vsize < __builtin_huge_valf(), "the cell edge must be finite and > 0");
  SPX_CHECK(r2 >= 0.f && r2 < vsize * vsize, "the squared radius must be >= 0 and below the squared cell edge of the index");
  const size_t W = rank_words(3, batch, grid_zyx_h);
  SPX_CHECK(W > 0, "batch x grid has no rank map (beyond 2^31 cells)");
  SPX_CHECK(rankmap_bytes >= rank_bytes(W), "rank map too small for this grid (%zu words)", W);
  if (m_cap == 0) return 0;
  SPX_CHECK(queries && rows && count && cell_offsets && rankmap && (n_cap == 0 || (points && records)),
            "queries / points / cell_offsets / rankmap / records / rows / count is NULL");
  SPX_CHECK(aligned_to(queries, 4) && aligned_to(q_batch_ids, 4) && aligned_to(n_queries_dev, 4) && aligned_to(points, 4) &&
                aligned_to(cell_offsets, 4) && aligned_to(rankmap, 8) && aligned_to(records, 16) && aligned_to(rows, 4) &&
                aligned_to(count, 4) && aligned_to(dist2, 4) && aligned_to(weights, 4) && aligned_to(out_offsets, 4),
            "pointer not aligned to its elements");
  void *rm = const_cast<void *>(rankmap);
  CellQueryArgs a = {{n_cap, batch, {grid_zyx_h[0], grid_zyx_h[1], grid_zyx_h[2]}, static_cast<const uint2 *>(rm),
                      rank_blockoff(rm, W), cell_offsets},
                     queries, q_nfeat, q_batch_ids, m_cap, n_queries_dev, points, nfeat, static_cast<const ClRec *>(records),
                     {lo_xyz_h[0], lo_xyz_h[1], lo_xyz_h[2]}, vsize, r2, nsample, width, flags, eps, rows, count, dist2,
                     weights, out_offsets};
  const dim3 grid(static_cast<unsigned>((static_cast<long long>(m_cap) + kCqGroups - 1) / kCqGroups));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (knn)
    hipLaunchKernelGGL(cell_query_kernel<true>, grid, dim3(kCqBlock), 0, s, a);
  else
    hipLaunchKernelGGL(cell_query_kernel<false>, grid, dim3(kCqBlock), 0, s, a);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace spx

extern "C" {

int spx_cell_records(const float *points, int nfeat, const int32_t *batch_ids, int n_cap, const int32_t *n_points_dev,
                     int batch, const float *range_xyz_h, const int32_t *cell_rows, const int32_t *cell_offsets,
                     const int32_t *cell_list, void *records, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(n_cap >= 0 && n_cap <= kCellMaxPoints, "n_cap must be in 0 .. %d, got %d", kCellMaxPoints, n_cap);
  SPX_CHECK(nfeat >= 3, "points need at least 3 columns, got %d", nfeat);
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  SPX_CHECK(range_xyz_h, "the range is NULL");
  for (int j = 0; j < 3; ++j)
    SPX_CHECK(isfinite(range_xyz_h[j]) && isfinite(range_xyz_h[3 + j]) && range_xyz_h[j] < range_xyz_h[3 + j],
              "the range of axis %d must be finite and not empty", j);
  if (n_cap == 0) return 0;
  SPX_CHECK(points && cell_rows && cell_offsets && cell_list && records, "points / cell groups / records is NULL");
  SPX_CHECK(aligned_to(points, 4) && aligned_to(batch_ids, 4) && aligned_to(n_points_dev, 4) && aligned_to(cell_rows, 4) &&
                aligned_to(cell_offsets, 4) && aligned_to(cell_list, 4) && aligned_to(records, 16),
            "pointer not aligned to its elements");
  CellRecordArgs a = {points, nfeat, n_cap, n_points_dev, batch_ids, batch,
                      {range_xyz_h[0], range_xyz_h[1], range_xyz_h[2]}, {range_xyz_h[3], range_xyz_h[4], range_xyz_h[5]},
                      cell_rows, cell_offsets, cell_list, static_cast<ClRec *>(records)};
  hipLaunchKernelGGL(cell_records_kernel, dim3(static_cast<unsigned>((static_cast<long long>(n_cap) + kCqBlock - 1) / kCqBlock)),
                     dim3(kCqBlock), 0, static_cast<hipStream_t>(stream), a);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_ball_query_cells(const float *queries, int q_nfeat, const int32_t *q_batch_ids, int m_cap,
                         const int32_t *n_queries_dev, const float *points, int nfeat, int n_cap, int batch,
                         const int *grid_zyx_h, const float *lo_xyz_h, float vsize, const int32_t *cell_offsets,
                         const void *rankmap, size_t rankmap_bytes, const void *records, int nsample, float r2, int flags,
                         int32_t *rows, int32_t *count, float *out_offsets, spx_stream_t stream) {
  return spx::cell_query(false, queries, q_nfeat, q_batch_ids, m_cap, n_queries_dev, points, nfeat, n_cap, batch, grid_zyx_h,
                         lo_xyz_h, vsize, cell_offsets, rankmap, rankmap_bytes, records, nsample, nsample, r2, 0.f, flags,
                         rows, count, nullptr, nullptr, out_offsets, stream);
}

int spx_knn_query_cells(const float *queries, int q_nfeat, const int32_t *q_batch_ids, int m_cap,
                        const int32_t *n_queries_dev, const float *points, int nfeat, int n_cap, int batch,
                        const int *grid_zyx_h, const float *lo_xyz_h, float vsize, const int32_t *cell_offsets,
                        const void *rankmap, size_t rankmap_bytes, const void *records, int k, int width, float r2, float eps,
                        int flags, int32_t *rows, int32_t *count, float *dist2, float *weights, float *out_offsets,
                        spx_stream_t stream) {
  return spx::cell_query(true, queries, q_nfeat, q_batch_ids, m_cap, n_queries_dev, points, nfeat, n_cap, batch, grid_zyx_h,
                         lo_xyz_h, vsize, cell_offsets, rankmap, rankmap_bytes, records, k, width, r2, eps, flags, rows, count,
                         dist2, weights, out_offsets, stream);
}

}  // extern "C"
