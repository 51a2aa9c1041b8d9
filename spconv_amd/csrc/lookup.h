// A LEVEL AS SOMETHING POINTS LOOK CELLS UP IN: a point's own cell (the geometry by point column, the voxeliser's
// expression, the batch / count test), a cell's linear key -> a live row of the level (one load of the rank map,
// rankmap.h, for a key-ordered level; a probe of the builders' hash table, table.h, built here from the level's rows,
// for rows in any order), and the host side: the pointer-free checks of a level, the hash form's scratch and build.
// Shared by the units whose kernels start from a point (interp.hip, query.hip); every definition has internal linkage.
#pragma once
#include "common.h"
#include "rankmap.h"
#include "table.h"

// A point's cell promises float32 results a host reproduces bit for bit, and the contraction mode is that of where an
// expression is DEFINED (see pointvoxel.hip): no multiply-add pair written here may be contracted into an FMA.
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kPointDims = 3;         // a level that points look cells up in has 2 or 3 axes
constexpr int kMaxRows = 1 << 30;     // rows of a level: table_capacity(n) = 2^31 slots still fits its 32-bit mask
constexpr int kInsertThreads = 256;

// -------------------------------------------------------------------------------------------- a point's own cell

struct PointGeom {
  LevelGeom level;                              // batch and grid extents, index-column (zyx) order
  float vsize[kPointDims], lo[kPointDims];      // by POINT COLUMN (x, y, z): entry j belongs to grid axis ndim - 1 - j
  // the host arrays are zyx: point column j is axis ndim - 1 - j
  PointGeom(int ndim, int batch, const int *spatial_h, const float *vsize_zyx, const float *coors_range_zyx)
      : level(ndim, batch, spatial_h) {
    for (int j = 0; j < kPointDims; ++j) {
      vsize[j] = j < ndim ? vsize_zyx[ndim - 1 - j] : 1.f;
      lo[j] = j < ndim ? coors_range_zyx[ndim - 1 - j] : 0.f;
    }
  }
};

// Does point i exist for the level?  Not at or beyond *n_points (null: n_cap), nor with a batch id outside it.
// b: its batch (batch_ids null: 0), meaningful for a point that exists.
template <typename I>                 // (the caller's index type: an int index keeps its 32-bit compare)
__device__ __forceinline__ bool point_batch(const PointGeom &g, const int32_t *batch_ids, int n_cap,
                                            const int32_t *n_points, I i, int &b) {
  const int np = n_points ? *n_points : n_cap;
  b = i < np ? (batch_ids ? batch_ids[i] : 0) : -1;
  return b >= 0 && b < g.level.batch;
}

// Coordinate pj of point column j in cells: t = (pj - lo) / vsize, the voxeliser's own expression (voxelize.hip),
// returned, and the point's cell floorf(t) along that column's axis.  `valid` stays true only for a cell inside the
// extent (a NaN coordinate clears it).
template <int NDIM>
__device__ __forceinline__ float point_cell(const PointGeom &g, int j, float pj, float &cell, bool &valid) {
  const float t = (pj - g.lo[j]) / g.vsize[j];
  cell = floorf(t);
  valid = valid && cell >= 0.f && cell < static_cast<float>(g.level.dims[NDIM - 1 - j]);      // (false for NaN)
  return t;
}

// -------------------------------------------------------------------------------------------- key -> row

// What a kernel finds the rows of a level with: the view of its rank map (rankmap.h: cells[w] = {occupancy bits of
// cells 32 w .. 32 w + 31, occupied cells before them inside the block}, blockoff[w >> 11] = occupied cells before
// the 2048-word block; null: the level carries no map) or the table, and the level's row count.
struct LevelLookup {
  const uint2 *cells;
  const int32_t *blockoff;
  Table table;
  int n;
  const int32_t *n_live;              // device count of the live rows (null: all n)
  __device__ __forceinline__ int live() const { return n_live ? min(*n_live, n) : n; }
};

// key -> row, or -1: no row there, or one at or beyond the live rows.  RANKED: rank_of over the map, else a probe of
// the table.
template <bool RANKED> struct RowFinder {
  const LevelLookup &look;
  int live;
  __device__ __forceinline__ explicit RowFinder(const LevelLookup &l) : look(l), live(l.live()) {}
  __device__ __forceinline__ int operator()(long long key) const {
    const int r = RANKED ? rank_of(look.cells, look.blockoff, static_cast<unsigned long long>(key))
                         : table_find(look.table, key);
    return static_cast<unsigned>(r) < static_cast<unsigned>(live) ? r : -1;
  }
};

// the live rows of the level into the table, by their linear key (level_key of rankmap.h over all axes)
__global__ void __launch_bounds__(kInsertThreads)
level_insert_kernel(const int32_t *__restrict__ idx, int n, const int32_t *__restrict__ n_live, LevelGeom g, Table t) {
  const int i = blockIdx.x * kInsertThreads + threadIdx.x;
  if (i >= n || (n_live && i >= *n_live)) return;
  const long long key = level_key(idx + static_cast<size_t>(i) * (g.ndim + 1), g, kAllAxes);
  if (key >= 0) table_insert_min(t, key, i);      // (a duplicate coordinate: the lowest row stays)
}

// -------------------------------------------------------------------------------------------- host side

// 0 = ok: the checks of a level that points (`noun`: what the caller calls them) look cells up in, none of which
// needs a device pointer; `look` receives the row counts and the view of the rank map (rankmap: the caller's buffer,
// or null for the hash form, whose table build_level_table places).
int check_level(const char *noun, int ndim, int nfeat, int n, const int32_t *n_live, int batch, const int *spatial_h,
                const float *vsize, const float *coors_range, const void *rankmap, size_t rankmap_bytes,
                LevelLookup *look) {
  SPX_CHECK(ndim == 2 || ndim == 3, "ndim must be 2 or 3, got %d", ndim);
  SPX_CHECK(n <= kMaxRows, "at most 2^30 voxel rows (the table holds two slots per row), got %d", n);
  SPX_CHECK(nfeat >= ndim, "%s need at least %d columns, got %d", noun, ndim, nfeat);
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  SPX_CHECK(vsize && coors_range && spatial_h, "vsize / coors_range / spatial shape is NULL");
  unsigned long long cells_total = static_cast<unsigned long long>(batch);
  for (int d = 0; d < ndim; ++d) {
    SPX_CHECK(spatial_h[d] >= 1, "empty grid axis %d", d);
    SPX_CHECK(vsize[d] > 0.f, "voxel size of axis %d must be positive", d);
    SPX_CHECK(cells_total <= (0x7fffffffffffffffULL / static_cast<unsigned long long>(spatial_h[d])),
              "the key space of batch x grid does not fit 63 bits");
    cells_total *= static_cast<unsigned long long>(spatial_h[d]);
  }
  const size_t W = rankmap ? rank_words(ndim, batch, spatial_h) : 0;      // (the pointer's value, not its target)
  SPX_CHECK(!rankmap || (W > 0 && rankmap_bytes >= rank_bytes(W)), "rank map too small for this level (%zu words)", W);
  void *rm = const_cast<void *>(rankmap);
  *look = {static_cast<const uint2 *>(rm), rankmap ? rank_blockoff(rm, W) : nullptr, Table{}, n, n_live};
  return 0;
}

// scratch of a hash-form lookup: the table (room for the wide form, 12 bytes per slot)
struct LevelTableWs {
  hkey_t *keys;
  int32_t *vals;
  uint32_t cap;
  size_t bytes;
  LevelTableWs(void *ws, int n) {
    Carver c(ws);
    cap = table_capacity(static_cast<size_t>(n > 0 ? n : 0));
    keys = c.take<hkey_t>(cap);
    vals = c.take<int32_t>(cap);
    bytes = c.off;
  }
};

// How a level's rows become a lookup table: placed in the caller's scratch (packed slots when batch x grid fits 32
// bits), emptied, the live rows inserted.  0 = ok.
int build_level_table(void *ws, size_t ws_bytes, const int32_t *indices, int n, const int32_t *n_live, const LevelGeom &g,
                      Table *t, hipStream_t s) {
  LevelTableWs w(ws, n);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  table_place(*t, w.keys, w.vals, w.cap, keys_fit_u32(g.batch, g.dims, kMaxNdim));
  FillList fills;
  table_fill(fills, *t);
  SPX_HIP(fills.launch(s));
  if (n > 0) {
    hipLaunchKernelGGL(level_insert_kernel, dim3(div_up(n, kInsertThreads)), dim3(kInsertThreads), 0, s, indices, n, n_live,
                       g, *t);
    SPX_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
}  // namespace spx
