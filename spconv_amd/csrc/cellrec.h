// THE CELL INDEX OF A POINT CLOUD as its readers see it (cluster.hip, cellquery.hip): the points as 16-byte records in
// cell order, and the lookup that turns a line of cells into ONE contiguous run of records.  The index is made from
// existing pieces -- the static voxeliser in key order over cells of edge radius * (1 + 2^-6) (cell rows, the level's
// rank map) and spx_point_groups over its pc_voxel_id (cell_offsets, cell_list); DESIGN.md section 3.43 has the
// argument that two points within the radius lie at most one cell apart on every axis.  Internal linkage.
#pragma once
#include "common.h"

namespace spx {
namespace {

constexpr int kCellMaxAxis = 1 << 14;                // cells per axis the widened edge is proven for
constexpr int kCellMaxPoints = (1 << 30) - 8;

// A point in cell order; x = NaN for a point that takes no part (its d2 is NaN: never below r2).
struct __attribute__((aligned(16))) ClRec {
  float x, y, z;
  int32_t idx;
};
static_assert(sizeof(ClRec) == 16, "one 16-byte load per candidate");

// What a kernel walks the index with: the grid (z, y, x), the words of the rank map and the offsets of the cells' records.
struct CellLookup {
  int n_cap, batch;
  int dims[3];
  const uint2 *cells;
  const int32_t *blockoff;
  const int32_t *cell_offsets;
};

// occupied cells with a key below `key` (the row `key` has, or would have), and whether `key` is occupied
__device__ __forceinline__ int rank_lower(const CellLookup &a, unsigned long long key, bool &occupied) {
  const uint2 cell = a.cells[key >> 5];
  const uint32_t bit = 1u << (key & 31);
  occupied = (cell.x & bit) != 0u;
  return a.blockoff[key >> 16] + static_cast<int>(cell.y) + __popc(cell.x & (bit - 1u));
}

// the offset of cell row `row`, the row clamped into the table
__device__ __forceinline__ int cell_offset(const CellLookup &a, int row) { return a.cell_offsets[min(max(row, 0), a.n_cap)]; }

// The records of cells x0 .. x1 (0 <= x0 <= x1 < dims[2]) of line (b, zz, yy), which lies inside the grid: consecutive
// keys, so in a key-ordered level consecutive rows and one run [beg, end) -- two rank-map lookups, none per cell.  The
// caller clamps the run into the records that exist.
__device__ __forceinline__ void line_run(const CellLookup &a, int b, int zz, int yy, int x0, int x1, int &beg, int &end) {
  const unsigned long long base =
      ((static_cast<unsigned long long>(b) * a.dims[0] + zz) * a.dims[1] + yy) * static_cast<unsigned long long>(a.dims[2]);
  bool occ;
  const int first = rank_lower(a, base + x0, occ);
  const int last = rank_lower(a, base + x1, occ) + (occ ? 1 : 0);
  beg = cell_offset(a, first);
  end = cell_offset(a, last);
}

}  // namespace
}  // namespace spx
