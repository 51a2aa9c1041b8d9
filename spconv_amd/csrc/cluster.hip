// Instance clustering: the connected components of the radius graph of a point cloud (spx_cluster_records,
// spx_cluster_link, spx_cluster_roots, spx_cluster_number) -- the grouping stage of the bottom-up instance-segmentation
// networks (PointGroup, HAIS, SoftGroup: ballquery_batch_p + bfs_cluster, the second of which runs on the CPU there).
// Two points that take part are linked when they share a scene and a label and d2 < r2 under spx_ball_query's float32
// predicate; a cluster is a connected component with enough points.
//
//   index     made by the caller from existing pieces: the static voxeliser in key order over cells of edge
//             radius * (1 + 2^-6) (indices, the level's rank map) and spx_point_groups over its pc_voxel_id (cell_rows,
//             cell_offsets, cell_list).  The widened edge keeps two linked points at most one cell apart on every axis
//             (DESIGN.md section 3.43 has the argument and the bound of 2^14 cells per axis it needs).
//   records   one lane per position of cell_list: the point as a 16-byte record {x, y, z, index} in CELL ORDER, x = NaN for
//             a point that takes no part (its d2 is NaN: never below r2), the cell's row beside it; parent[i] = i for a
//             point that takes part, -1 (a fill in front) for every other.
//   link      one lane per record, workgroups of 256 consecutive records (the same or adjacent cells: their candidate
//             runs overlap in L1).  A lane walks a HALF stencil -- the four (dz, dy) lines in front of its own with
//             three cells each, and on its own line the cell before its own and the records before its own in its cell:
//             13 neighbours + itself, every edge met once.  The cells of a line are consecutive keys, so in a key-ordered
//             level their rows are consecutive and their records ONE contiguous run offsets[first] .. offsets[last + 1]:
//             two rank-map lookups per line, none per cell.  A pair that passes is united in parent[] by lock-free
//             hooking: the larger root is attached to the smaller by atomicCAS, find halves paths with atomicMin.
//             parent[x] <= x holds at every instant, so every walk goes strictly downwards; a walk over a unite call
//             never restarts from the top, which bounds its steps by 2 n + 8 -- the explicit budget every loop carries.
//             A budget that runs out, a parent above its child or a table entry out of range sets a bit of the status
//             word and leaves the loop.  Vector atomics in plain C++ only.
//   roots     root[i] = find(i), in place over parent (a stored root is an ancestor like any other: concurrent walks stay
//             correct); -1 for a point that takes no part.  The root of a component is its smallest point index.
//   number    sizes come from spx_point_groups over the roots (offsets[r + 1] - offsets[r]: no atomics); the flags
//             `is a root and large enough` are counted per block, scanned by one block (block_scan_loop), and numbered:
//             kept components 0, 1, ... by ascending root; a last pass gives every point its root's number.
// No kernel of this unit holds a barrier in divergent control flow (only the numbering passes hold barriers, in uniform
// loops).  Every index read from a table is range-checked before it addresses anything.
#include <math.h>

#include "cellrec.h"
#include "common.h"
#include "fill.h"
#include "piece.h"
#include "rankmap.h"
#include "scan.h"

// the predicate is spx_ball_query's: no multiply-add pair of this unit may be contracted into an FMA
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kClBlock = 256;
constexpr int kClItems = 2048;                       // points of a numbering block
constexpr int kClMaxAxis = kCellMaxAxis;
constexpr int kClMaxPoints = kCellMaxPoints;         // 2 n + 8 steps fit a 32-bit budget
static_assert(kClBlock == kScanThreads, "block_rank and block_scan_loop are kScanThreads wide");
static_assert(kClItems % kClBlock == 0, "a numbering block is whole rounds");

enum : int { kStFind = 1, kStHook = 2, kStParent = 4, kStTable = 8 };

struct ClWs {
  ClRec *recs;
  int32_t *rec_cell, *blockcount, *blockoff;
  int nblk;
  size_t bytes;
  ClWs(void *ws, int n_cap) {
    Carver c(ws);
    const size_t n = static_cast<size_t>(n_cap > 0 ? n_cap : 0);
    nblk = static_cast<int>((n + kClItems - 1) / kClItems);
    recs = c.take<ClRec>(n ? n : 1);
    rec_cell = c.take<int32_t>(n ? n : 1);
    blockcount = c.take<int32_t>(nblk ? nblk : 1);
    blockoff = c.take<int32_t>(nblk ? nblk : 1);
    bytes = c.off;
  }
};

// -------------------------------------------------------------------------------------------- records

struct RecordArgs {
  const float *points;
  int nfeat, n_cap;
  const int32_t *n_points, *batch_ids;
  int batch;
  const int32_t *labels;
  const uint8_t *valid;
  float lo[3], hi[3];
  const int32_t *cell_rows, *cell_offsets, *cell_list;
  ClRec *recs;
  int32_t *rec_cell, *parent;
};

__global__ void __launch_bounds__(kClBlock)
cluster_records_kernel(RecordArgs a) {
  const long long pos = static_cast<long long>(blockIdx.x) * kClBlock + threadIdx.x;
  if (pos >= a.n_cap) return;
  const int total = min(max(a.cell_offsets[a.n_cap], 0), a.n_cap);      // points that have a cell
  ClRec r = {__builtin_nanf(""), 0.f, 0.f, -1};
  int cell = -1;
  if (pos < total) {
    const int i = a.cell_list[pos];
    const int np = a.n_points ? min(*a.n_points, a.n_cap) : a.n_cap;
    if (i >= 0 && i < np) {
      const int b = a.batch_ids ? a.batch_ids[i] : 0;
      const float *p = a.points + static_cast<size_t>(i) * a.nfeat;
      const float x = p[0], y = p[1], z = p[2];
      bool ok = b >= 0 && b < a.batch;
      ok = ok && x >= a.lo[0] && x < a.hi[0] && y >= a.lo[1] && y < a.hi[1] && z >= a.lo[2] && z < a.hi[2];   // (false for NaN)
      ok = ok && (!a.valid || a.valid[i] != 0) && (!a.labels || a.labels[i] >= 0);
      const int v = a.cell_rows[i];
      if (ok && v >= 0 && v < a.n_cap) {
        r = {x, y, z, i};
        cell = v;
        a.parent[i] = i;
      }
    }
  }
  a.recs[pos] = r;
  a.rec_cell[pos] = cell;
}

// -------------------------------------------------------------------------------------------- union-find

__device__ __forceinline__ int ld_parent(const int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x, halving the path on the way; -1 once the budget is spent or a parent lies above its child (a status
// bit is set).  Every step moves x strictly downwards.
__device__ __forceinline__ int find_root(int32_t *parent, int x, int &budget, int32_t *status) {
  for (;;) {
    const int p = ld_parent(parent + x);
    if (p == x) return x;
    if (static_cast<unsigned>(p) > static_cast<unsigned>(x)) {          // (p < 0 included)
      atomicOr(status, kStParent);
      return -1;
    }
    const int gp = ld_parent(parent + p);
    if (gp == p) return p;
    if (static_cast<unsigned>(gp) > static_cast<unsigned>(p)) {
      atomicOr(status, kStParent);
      return -1;
    }
    atomicMin(parent + x, gp);
    x = gp;
    if (--budget < 0) {
      atomicOr(status, kStFind);
      return -1;
    }
  }
}

// Unites the sets of a and b: the larger root is hooked onto the smaller.  A failed CAS means someone hooked that root
// first: the walk goes on from what it was hooked to, below it.  a and b only ever move downwards, so one call takes at
// most a + b + O(1) steps: `budget` = 2 n + 8 is never spent by a sound parent array.
__device__ __forceinline__ void unite(int32_t *parent, int a, int b, int budget, int32_t *status) {
  for (;;) {
    a = find_root(parent, a, budget, status);
    b = find_root(parent, b, budget, status);
    if (a < 0 || b < 0 || a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicCAS(parent + a, a, b);
    if (old == a) return;
    if (static_cast<unsigned>(old) >= static_cast<unsigned>(a)) {
      atomicOr(status, kStParent);
      return;
    }
    a = old;
    if (--budget < 0) {
      atomicOr(status, kStHook);
      return;
    }
  }
}

// -------------------------------------------------------------------------------------------- link

struct LinkArgs : CellLookup {                        // (cellrec.h: the grid, the rank map, the cells' offsets)
  const int4 *indices;                                // {batch, z, y, x} of every cell row
  const int32_t *labels;
  float r2;
  const ClRec *recs;
  const int32_t *rec_cell;
  int32_t *parent, *status;
};

__global__ void __launch_bounds__(kClBlock)
cluster_link_kernel(LinkArgs a) {
  const long long pos = static_cast<long long>(blockIdx.x) * kClBlock + threadIdx.x;
  if (pos >= a.n_cap) return;
  const int v = a.rec_cell[pos];
  if (v < 0 || v >= a.n_cap) return;                  // no part: nothing to link (no barrier below)
  const ClRec me = a.recs[pos];
  if (static_cast<unsigned>(me.idx) >= static_cast<unsigned>(a.n_cap)) return;
  const int4 c = a.indices[v];
  if (static_cast<unsigned>(c.x) >= static_cast<unsigned>(a.batch) || static_cast<unsigned>(c.y) >= static_cast<unsigned>(a.dims[0]) ||
      static_cast<unsigned>(c.z) >= static_cast<unsigned>(a.dims[1]) || static_cast<unsigned>(c.w) >= static_cast<unsigned>(a.dims[2])) {
    atomicOr(a.status, kStTable);
    return;
  }
  const int total = min(max(a.cell_offsets[a.n_cap], 0), a.n_cap);
  const int my_label = a.labels ? a.labels[me.idx] : 0;
  const int budget = 2 * a.n_cap + 8;
#pragma unroll 1
  for (int line = 0; line < 5; ++line) {              // (dz, dy) = (-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 0)
    const int dz = line < 3 ? -1 : 0, dy = line < 3 ? line - 1 : line - 4;
    const int zz = c.y + dz, yy = c.z + dy;
    if (zz < 0 || yy < 0 || yy >= a.dims[1]) continue;
    int beg, end;
    if (line == 4) {                                  // the cell before mine, then the records before me in my cell
      bool occ;
      const unsigned long long base =
          ((static_cast<unsigned long long>(c.x) * a.dims[0] + zz) * a.dims[1] + yy) * static_cast<unsigned long long>(a.dims[2]);
      beg = cell_offset(a, c.w > 0 ? rank_lower(a, base + c.w - 1, occ) : v);
      end = static_cast<int>(pos);
    } else {
      line_run(a, c.x, zz, yy, max(c.w - 1, 0), min(c.w + 1, a.dims[2] - 1), beg, end);
    }
    beg = min(max(beg, 0), total);
    end = min(max(end, beg), total);
    for (int k = beg; k < end; ++k) {
      const ClRec q = a.recs[k];
      const float d0 = q.x - me.x, d1 = q.y - me.y, d2 = q.z - me.z;
      float s = d0 * d0 + d1 * d1;                    // dist2<3> of scenes.h, operation by operation
      s = s + d2 * d2;
      if (!(s < a.r2)) continue;                      // (a record that takes no part has x = NaN)
      if (static_cast<unsigned>(q.idx) >= static_cast<unsigned>(a.n_cap)) continue;
      if (a.labels && a.labels[q.idx] != my_label) continue;
      unite(a.parent, me.idx, q.idx, budget, a.status);
    }
  }
}

// -------------------------------------------------------------------------------------------- roots

__global__ void __launch_bounds__(kClBlock)
cluster_roots_kernel(int32_t *parent, int n_cap, int32_t *status) {
  const long long i = static_cast<long long>(blockIdx.x) * kClBlock + threadIdx.x;
  if (i >= n_cap) return;
  if (ld_parent(parent + i) < 0) return;              // takes no part: stays -1
  int budget = n_cap + 8;
  const int r = find_root(parent, static_cast<int>(i), budget, status);
  __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// -------------------------------------------------------------------------------------------- numbering

struct NumberArgs {
  int n_cap, cap;
  const int32_t *root, *size_offsets, *labels;
  int min_points;
  const float *min_table;                             // per label, or null: min_points
  int num_labels;
};

// is i the root of a component that is kept?
__device__ __forceinline__ bool kept_root(const NumberArgs &a, int i) {
  if (i >= a.n_cap || a.root[i] != i) return false;
  const int lo = a.size_offsets[i], hi = a.size_offsets[i + 1];
  const int size = min(max(hi - lo, 0), a.n_cap);
  if (!a.min_table) return size >= a.min_points;
  const int lab = a.labels[i];
  return static_cast<unsigned>(lab) < static_cast<unsigned>(a.num_labels) && static_cast<float>(size) >= a.min_table[lab];
}

__global__ void __launch_bounds__(kClBlock)
cluster_count_kernel(NumberArgs a, int32_t *__restrict__ blockcount) {
  __shared__ int lds_wave[kClBlock / 64];
  const int begin = blockIdx.x * kClItems;
  int cnt = 0;
#pragma unroll
  for (int it = 0; it < kClItems / kClBlock; ++it)
    cnt += __popcll(__ballot(kept_root(a, begin + it * kClBlock + threadIdx.x)));
  if ((threadIdx.x & 63) == 0) lds_wave[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < kClBlock / 64; ++w) sum += lds_wave[w];
    blockcount[blockIdx.x] = sum;
  }
}

__global__ void __launch_bounds__(kClBlock)
cluster_totals_kernel(const int32_t *__restrict__ blockcount, int32_t *__restrict__ blockoff, int nblk, int cap,
                      int32_t *__restrict__ count) {
  __shared__ int lds_wave[kClBlock / 64];
  const int total = block_scan_loop(blockcount, blockoff, nblk, lds_wave);
  if (threadIdx.x == 0) *count = min(total, cap);
}

// cluster_of_point[i] = the number of the kept component i is the root of, -1 for every other i
__global__ void __launch_bounds__(kClBlock)
cluster_number_kernel(NumberArgs a, const int32_t *__restrict__ blockoff, int32_t *__restrict__ cluster_of_point) {
  __shared__ int lds_wave[kClBlock / 64];
  const int begin = blockIdx.x * kClItems;
  int running = blockoff[blockIdx.x];
  for (int it = 0; it < kClItems / kClBlock; ++it) {   // (uniform: block_rank holds barriers)
    const int i = begin + it * kClBlock + threadIdx.x;
    const bool keep = kept_root(a, i);
    int total;
    const int num = running + block_rank(keep, total, lds_wave);
    if (i < a.n_cap) cluster_of_point[i] = keep && num < a.cap ? num : -1;
    running += total;
  }
}

// every other point takes its root's number (a root's entry is written by the pass in front only)
__global__ void __launch_bounds__(kClBlock)
cluster_assign_kernel(const int32_t *__restrict__ root, int n_cap, int32_t *cluster_of_point) {
  const long long i = static_cast<long long>(blockIdx.x) * kClBlock + threadIdx.x;
  if (i >= n_cap) return;
  const int r = root[i];
  if (r == i || static_cast<unsigned>(r) >= static_cast<unsigned>(n_cap)) return;
  cluster_of_point[i] = cluster_of_point[r];
}

int check_cloud_size(int n_cap) {
  SPX_CHECK(n_cap >= 0 && n_cap <= kClMaxPoints, "n_cap must be in 0 .. %d, got %d", kClMaxPoints, n_cap);
  return 0;
}

int check_cluster_ws(int n_cap, const void *ws, size_t ws_bytes) {
  SPX_CHECK(ws && ws_bytes >= spx_cluster_ws_bytes(n_cap), "workspace too small: %zu < %zu", ws_bytes,
            spx_cluster_ws_bytes(n_cap));
  SPX_CHECK(aligned_to(ws, 16), "workspace not aligned to 16 bytes");
  return 0;
}

dim3 point_grid(int n_cap) { return dim3(static_cast<unsigned>((static_cast<long long>(n_cap) + kClBlock - 1) / kClBlock)); }

}  // namespace
}  // namespace spx

// -------------------------------------------------------------------------------------------- host side

extern "C" {

int spx_cluster_max_axis_cells(void) { return spx::kClMaxAxis; }

size_t spx_cluster_ws_bytes(int n_cap) {
  if (n_cap < 0 || n_cap > spx::kClMaxPoints) return 0;
  return spx::ClWs(nullptr, n_cap).bytes;
}

int spx_cluster_records(const float *points, int nfeat, const int32_t *batch_ids, int n_cap, const int32_t *n_points_dev,
                        int batch, const int32_t *labels, const void *valid, const float *range_xyz_h,
                        const int32_t *cell_rows, const int32_t *cell_offsets, const int32_t *cell_list, int32_t *root,
                        int32_t *status, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_cloud_size(n_cap)) return rc;
  SPX_CHECK(nfeat >= 3, "points need at least 3 columns, got %d", nfeat);
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  SPX_CHECK(range_xyz_h, "the range is NULL");
  for (int j = 0; j < 3; ++j)
    SPX_CHECK(isfinite(range_xyz_h[j]) && isfinite(range_xyz_h[3 + j]) && range_xyz_h[j] < range_xyz_h[3 + j],
              "the range of axis %d must be finite and not empty", j);
  SPX_CHECK(status, "status is NULL");
  SPX_CHECK(aligned_to(status, 4), "pointer not aligned to its elements");
  hipStream_t s = static_cast<hipStream_t>(stream);
  FillList fills;                                       // nobody takes part until the records pass says so
  fills.add(status, 4, 0u);
  if (n_cap > 0) {
    SPX_CHECK(points && cell_rows && cell_offsets && cell_list && root, "points / cell groups / root is NULL");
    SPX_CHECK(aligned_to(points, 4) && aligned_to(batch_ids, 4) && aligned_to(n_points_dev, 4) && aligned_to(labels, 4) &&
                  aligned_to(cell_rows, 4) && aligned_to(cell_offsets, 4) && aligned_to(cell_list, 4) && aligned_to(root, 4),
              "pointer not aligned to its elements");
    if (int rc = check_cluster_ws(n_cap, ws, ws_bytes)) return rc;
    fills.add(root, static_cast<size_t>(n_cap) * 4, 0xffffffffu);
  }
  SPX_HIP(fills.launch(s));
  if (n_cap == 0) return 0;
  const ClWs w(ws, n_cap);
  RecordArgs a = {points, nfeat, n_cap, n_points_dev, batch_ids, batch, labels, static_cast<const uint8_t *>(valid),
                  {range_xyz_h[0], range_xyz_h[1], range_xyz_h[2]}, {range_xyz_h[3], range_xyz_h[4], range_xyz_h[5]},
                  cell_rows, cell_offsets, cell_list, w.recs, w.rec_cell, root};
  hipLaunchKernelGGL(cluster_records_kernel, point_grid(n_cap), dim3(kClBlock), 0, s, a);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_cluster_link(int n_cap, int batch, const int *grid_zyx_h, const int32_t *indices, const int32_t *cell_offsets,
                     const void *rankmap, size_t rankmap_bytes, const int32_t *labels, float r2, int32_t *root,
                     int32_t *status, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_cloud_size(n_cap)) return rc;
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  SPX_CHECK(grid_zyx_h, "the grid is NULL");
  for (int j = 0; j < 3; ++j)
    SPX_CHECK(grid_zyx_h[j] >= 1 && grid_zyx_h[j] <= kClMaxAxis, "grid axis %d must hold 1 .. %d cells, got %d", j,
              kClMaxAxis, grid_zyx_h[j]);
  SPX_CHECK(r2 >= 0.f, "the squared radius must be >= 0 (and no NaN)");
  const size_t W = rank_words(3, batch, grid_zyx_h);
  SPX_CHECK(W > 0, "batch x grid has no rank map (beyond 2^31 cells)");
  SPX_CHECK(rankmap_bytes >= rank_bytes(W), "rank map too small for this grid (%zu words)", W);
  if (n_cap == 0) return 0;
  SPX_CHECK(indices && cell_offsets && rankmap && root && status, "indices / cell_offsets / rankmap / root / status is NULL");
  SPX_CHECK(aligned_to(indices, 16) && aligned_to(rankmap, 8) && aligned_to(cell_offsets, 4) && aligned_to(labels, 4) &&
                aligned_to(root, 4) && aligned_to(status, 4), "pointer not aligned to its elements");
  if (int rc = check_cluster_ws(n_cap, ws, ws_bytes)) return rc;
  const ClWs w(ws, n_cap);
  void *rm = const_cast<void *>(rankmap);
  LinkArgs a = {{n_cap, batch, {grid_zyx_h[0], grid_zyx_h[1], grid_zyx_h[2]}, static_cast<const uint2 *>(rm),
                 rank_blockoff(rm, W), cell_offsets},
                reinterpret_cast<const int4 *>(indices), labels, r2, w.recs, w.rec_cell, root, status};
  hipLaunchKernelGGL(cluster_link_kernel, point_grid(n_cap), dim3(kClBlock), 0, static_cast<hipStream_t>(stream), a);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_cluster_roots(int n_cap, int32_t *root, int32_t *status, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_cloud_size(n_cap)) return rc;
  if (n_cap == 0) return 0;
  SPX_CHECK(root && status, "root / status is NULL");
  SPX_CHECK(aligned_to(root, 4) && aligned_to(status, 4), "pointer not aligned to its elements");
  hipLaunchKernelGGL(cluster_roots_kernel, point_grid(n_cap), dim3(kClBlock), 0, static_cast<hipStream_t>(stream), root,
                     n_cap, status);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_cluster_number(int n_cap, const int32_t *root, const int32_t *size_offsets, const int32_t *labels, int min_points,
                       const float *min_table, int num_labels, int cap, int32_t *cluster_of_point, int32_t *count,
                       void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_cloud_size(n_cap)) return rc;
  SPX_CHECK(cap >= 1, "cap must be >= 1, got %d", cap);
  SPX_CHECK(min_table ? num_labels >= 1 : min_points >= 1, "min_points (or the labels of its table) must be >= 1");
  SPX_CHECK(!min_table || labels, "a min_points table is indexed by the labels, which are NULL");
  SPX_CHECK(count, "count is NULL");
  SPX_CHECK(aligned_to(count, 4) && aligned_to(min_table, 4), "pointer not aligned to its elements");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_cap == 0) {
    FillList fills;
    fills.add(count, 4, 0u);
    SPX_HIP(fills.launch(s));
    return 0;
  }
  SPX_CHECK(root && size_offsets && cluster_of_point, "root / size_offsets / cluster_of_point is NULL");
  SPX_CHECK(aligned_to(root, 4) && aligned_to(size_offsets, 4) && aligned_to(labels, 4) && aligned_to(cluster_of_point, 4),
            "pointer not aligned to its elements");
  if (int rc = check_cluster_ws(n_cap, ws, ws_bytes)) return rc;
  const ClWs w(ws, n_cap);
  const NumberArgs a = {n_cap, cap, root, size_offsets, labels, min_points, min_table, num_labels};
  hipLaunchKernelGGL(cluster_count_kernel, dim3(w.nblk), dim3(kClBlock), 0, s, a, w.blockcount);
  hipLaunchKernelGGL(cluster_totals_kernel, dim3(1), dim3(kClBlock), 0, s, w.blockcount, w.blockoff, w.nblk, cap, count);
  hipLaunchKernelGGL(cluster_number_kernel, dim3(w.nblk), dim3(kClBlock), 0, s, a, w.blockoff, cluster_of_point);
  hipLaunchKernelGGL(cluster_assign_kernel, point_grid(n_cap), dim3(kClBlock), 0, s, root, n_cap, cluster_of_point);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
