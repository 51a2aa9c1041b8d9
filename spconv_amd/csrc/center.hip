// Training targets of the centre heads (spx_box_centers, spx_center_heatmap, spx_center_nearest,
// spx_center_heatmap_sparse): the Gaussian heatmaps of CenterPoint's assign_target_of_single_head and of VoxelNeXt's
// sparse twin, which OpenPCDet builds in a Python loop over the ground-truth boxes.  The header says what each entry
// computes; tests/refcenter.py restates it in numpy float32.
//
//   record    a box in the heat kernels is its RECORD: cell, radius and class plane (and, on a sparse level, the float
//             centre and the nearest row).  One lane per box writes it; the slot of a box -- its position among the
//             boxes of its scene -- is a bisection in the scene list, which is ascending in box index.  One lane per
//             entry of the [batch, max_objs] tables writes that entry from the box the list names there: every element
//             has one owner, no element is written twice, nothing is filled first.
//   dense     the gather form of points_in_boxes: a workgroup owns a 16 x 16 patch of one class plane, a lane a cell.  A
//             scene's records are staged 128 at a time and COMPACTED to the boxes of this class whose windows meet the
//             patch (a ballot and the popcount of the lanes below: ascending box index); every lane then walks the kept
//             ones as LDS broadcasts with its maximum in a register and stores it once.  No atomics, no zero fill; a
//             maximum of floats does not depend on the order of its operands.
//   nearest   a box to a wave over the rows of its scene, keys (bits of d2) << 32 | row reduced across the wave.
//   sparse    one lane per row on the scene walk of scenes.h with the roles turned: the rows are the walk's queries,
//             the records of a scene's boxes what a tile stages.  A lane keeps eight class maxima in registers (selected
//             by an unrolled compare, never indexed); more than eight classes walk again per group of eight, a box
//             being evaluated only in the pass of its class.
// Every barrier sits in control flow that is uniform over the workgroup.  Every float operation is rounded on its own.
#include "scenes.h"

// no multiply-add pair of this unit may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kCenterTile = 128;               // records staged per tile
constexpr int kCenterPatch = 16;               // a dense workgroup owns kCenterPatch x kCenterPatch cells
constexpr int kCenterChunk = 8;                // class maxima a lane of the sparse kernel keeps
constexpr int kCenterWaves = 4;                // boxes (waves) of a workgroup of the nearest-row kernel
constexpr int kCenterMaxClasses = SPX_CENTER_MAX_CLASSES, kCenterMaxExtent = 1 << 23, kCenterMaxRadius = 1 << 20;
constexpr int kAnchorCenter = SPX_CENTER_ANCHOR_CENTER, kAnchorNearest = SPX_CENTER_ANCHOR_NEAREST;
constexpr int kCutoffNone = SPX_CENTER_CUTOFF_NONE, kCutoffWindow = SPX_CENTER_CUTOFF_WINDOW;
static_assert(kCenterTile <= kSceneBlock, "one lane stages one record");
static_assert(kCenterPatch * kCenterPatch == kSceneBlock, "one lane per cell of a patch");

// expf(-d2 / (2 sigma^2)) with sigma = (2 r + 1) / 6: the division stays per element, as the Python loop has it
__device__ __forceinline__ float gauss(float d2, int r) {
  const float sigma = static_cast<float>(2 * r + 1) / 6.f;
  const float arg = -d2 / ((2.f * sigma) * sigma);
  return expf(arg);
}

__device__ __forceinline__ float sq_cells(int ddx, int ddy) {
  return static_cast<float>(static_cast<long long>(ddx) * ddx + static_cast<long long>(ddy) * ddy);
}

// -------------------------------------------------------------------------------------------- records

struct CenterArgs {
  const float *boxes;
  int nfeat;
  const int32_t *b_batch_ids;
  const void *class_ids;
  int class_bytes, m_cap;
  const int32_t *n_boxes, *offsets, *list;
  int batch, W, H;
  float vx, vy, x0, y0, stride;
  int C, max_objs;
  float ov;
  int min_radius;
  float *center;
  int32_t *cell, *radius, *cls, *slot, *box_index, *mask, *inds;
};

struct Record {
  float cx, cy;
  int ix, iy, r;
  int cls;          // the class plane of a box with a valid geometry, scene and class; else -1
  int b;            // its scene, -1 for none
};

// the smaller of two numbers, NaN when either is (fminf would drop the NaN)
__device__ __forceinline__ float min_nan(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }

__device__ __forceinline__ float clamp_cell(float v, int extent) {
  v = v < 0.f ? 0.f : v;
  const float hi = static_cast<float>(extent) - 0.5f;
  return v > hi ? hi : v;
}

// Box i < m_cap without its slot.  A box without a valid geometry -- at or beyond the device count, a number that is not
// finite, a size <= 0, a radius that is not finite or not below 2^20 -- is all zeros with class -1.
__device__ __forceinline__ Record box_record(const CenterArgs &a, int i) {
  Record rec = {0.f, 0.f, 0, 0, 0, -1, -1};
  const int live = a.n_boxes ? min(*a.n_boxes, a.m_cap) : a.m_cap;
  if (i >= live) return rec;
  const int b = a.b_batch_ids ? a.b_batch_ids[i] : 0;
  rec.b = b >= 0 && b < a.batch ? b : -1;
  float v[7];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    v[j] = a.boxes[static_cast<size_t>(i) * a.nfeat + j];
    ok = ok && finite(v[j]);
  }
  ok = ok && v[3] > 0.f && v[4] > 0.f && v[5] > 0.f;
  if (!ok) return rec;
  const float cx = clamp_cell(((v[0] - a.x0) / a.vx) / a.stride, a.W);
  const float cy = clamp_cell(((v[1] - a.y0) / a.vy) / a.stride, a.H);
  const float w = (v[3] / a.vx) / a.stride, h = (v[4] / a.vy) / a.stride, ov = a.ov;
  // CornerNet's gaussian_radius(h, w, ov) as every code base carries it
  const float b1 = h + w, c1 = ((w * h) * (1.f - ov)) / (1.f + ov);
  const float r1 = (b1 + sqrtf(b1 * b1 - 4.f * c1)) / 2.f;
  const float b2 = 2.f * (h + w), c2 = ((1.f - ov) * w) * h;
  const float r2 = (b2 + sqrtf(b2 * b2 - 16.f * c2)) / 2.f;
  const float a3 = 4.f * ov, b3 = (-2.f * ov) * (h + w), c3 = ((ov - 1.f) * w) * h;
  const float r3 = (b3 + sqrtf(b3 * b3 - (4.f * a3) * c3)) / 2.f;
  const float ret = min_nan(min_nan(r1, r2), r3);
  const float lim = static_cast<float>(kCenterMaxRadius);
  if (!(ret > -lim && ret < lim)) return rec;           // (false for NaN)
  long long cl = 0;
  if (a.class_ids)
    cl = a.class_bytes == 8 ? static_cast<const long long *>(a.class_ids)[i] : static_cast<const int32_t *>(a.class_ids)[i];
  rec.cx = cx, rec.cy = cy;
  rec.ix = static_cast<int>(cx), rec.iy = static_cast<int>(cy);
  rec.r = max(static_cast<int>(ret), a.min_radius);
  rec.cls = rec.b >= 0 && cl >= 0 && cl < a.C ? static_cast<int>(cl) : -1;
  return rec;
}

__global__ void __launch_bounds__(256)
box_centers_kernel(CenterArgs a) {
  const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (e < a.m_cap) {                                    // the lane of box e
    const int i = static_cast<int>(e);
    const Record rec = box_record(a, i);
    int slot = -1;
    if (rec.b >= 0) {                                   // the list of a scene is ascending in box index: a bisection
      int beg, end;
      scene_range(a.offsets, a.m_cap, rec.b, beg, end);
      int lo = beg, hi = end;
      while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (a.list[mid] < i) lo = mid + 1; else hi = mid;
      }
      if (lo < end && a.list[lo] == i && lo - beg < a.max_objs) slot = lo - beg;
    }
    a.center[2 * e] = rec.cx, a.center[2 * e + 1] = rec.cy;
    a.cell[2 * e] = rec.ix, a.cell[2 * e + 1] = rec.iy;
    a.radius[e] = rec.r;
    a.cls[e] = slot >= 0 ? rec.cls : -1;
    a.slot[e] = slot;
  }
  if (e < static_cast<long long>(a.batch) * a.max_objs) {    // the lane of entry e of the scene tables
    const int b = static_cast<int>(e / a.max_objs), s = static_cast<int>(e - static_cast<long long>(b) * a.max_objs);
    int beg, end;
    scene_range(a.offsets, a.m_cap, b, beg, end);
    int bi = -1, on = 0, ind = 0;
    if (s < end - beg) {
      const int i = a.list[beg + s];
      if (static_cast<unsigned>(i) < static_cast<unsigned>(a.m_cap)) {
        const Record rec = box_record(a, i);
        if (rec.b == b) {
          bi = i;
          on = rec.cls >= 0 ? 1 : 0;
          ind = on ? rec.iy * a.W + rec.ix : 0;
        }
      }
    }
    a.box_index[e] = bi, a.mask[e] = on, a.inds[e] = ind;
  }
}

// -------------------------------------------------------------------------------------------- dense

struct HeatArgs {
  const int32_t *cell, *radius, *cls;
  int m_cap;
  const int32_t *offsets, *list;
  int W, H, C, tiles_x;
  float *heat;
};

__global__ void __launch_bounds__(kSceneBlock)
center_heatmap_kernel(HeatArgs a) {
  __shared__ int s_ix[kCenterTile], s_iy[kCenterTile], s_r[kCenterTile];
  __shared__ int s_cnt[kSceneWaves];
  const int b = blockIdx.z, c = blockIdx.y;
  const int px0 = static_cast<int>(blockIdx.x % a.tiles_x) * kCenterPatch;
  const int py0 = static_cast<int>(blockIdx.x / a.tiles_x) * kCenterPatch;
  const int x = px0 + (threadIdx.x & (kCenterPatch - 1)), y = py0 + static_cast<int>(threadIdx.x) / kCenterPatch;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const u64 below = (1ull << lane) - 1ull;
  int beg, end;
  scene_range(a.offsets, a.m_cap, b, beg, end);         // (the same for every lane: the loop is uniform)
  float best = 0.f;
  for (int tile0 = beg; tile0 < end; tile0 += kCenterTile) {
    const int tn = min(kCenterTile, end - tile0);
    bool keep = false;
    int ix = 0, iy = 0, r = 0;
    if (static_cast<int>(threadIdx.x) < tn) {
      const int bi = a.list[tile0 + threadIdx.x];
      if (static_cast<unsigned>(bi) < static_cast<unsigned>(a.m_cap) && a.cls[bi] == c) {
        ix = a.cell[2 * static_cast<size_t>(bi)], iy = a.cell[2 * static_cast<size_t>(bi) + 1], r = a.radius[bi];
        const long long lr = r;
        keep = r >= 0 && r <= kCenterMaxRadius && ix + lr >= px0 && ix - lr < px0 + kCenterPatch && iy + lr >= py0 &&
               iy - lr < py0 + kCenterPatch;
      }
    }
    const u64 word = __ballot(keep);
    if (lane == 0) s_cnt[wave] = __builtin_popcountll(word);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSceneWaves; ++w) {
      base += w < wave ? s_cnt[w] : 0;
      total += s_cnt[w];
    }
    if (keep) {
      const int p = base + __builtin_popcountll(word & below);
      s_ix[p] = ix, s_iy[p] = iy, s_r[p] = r;
    }
    __syncthreads();
    for (int k = 0; k < total; ++k) {
      const int ddx = x - s_ix[k], ddy = y - s_iy[k], rk = s_r[k];
      if (abs(ddx) <= rk && abs(ddy) <= rk) {
        const float v = gauss(sq_cells(ddx, ddy), rk);
        best = v > best ? v : best;
      }
    }
    __syncthreads();                                    // (the next tile overwrites what this one read)
  }
  if (x < a.W && y < a.H) a.heat[((static_cast<size_t>(b) * a.C + c) * a.H + y) * a.W + x] = best;
}

// -------------------------------------------------------------------------------------------- nearest row

struct NearestArgs {
  const float *center;
  const int32_t *cls, *b_batch_ids;
  int m_cap;
  const int32_t *indices;
  int n_cap;
  const int32_t *n_live, *offsets, *list;
  int batch, W, H;
  const int32_t *box_index, *box_mask;
  int max_objs;
  int32_t *nearest, *inds, *mask;
};

// a live row's cell: row ri below `live`, of scene b, inside W x H
__device__ __forceinline__ bool live_cell(const int32_t *__restrict__ indices, int ri, int live, int b, int W, int H,
                                          int &vx, int &vy) {
  if (static_cast<unsigned>(ri) >= static_cast<unsigned>(max(live, 0))) return false;
  const int32_t *row = indices + static_cast<size_t>(ri) * 3;
  vy = row[1], vx = row[2];
  return row[0] == b && static_cast<unsigned>(vx) < static_cast<unsigned>(W) &&
         static_cast<unsigned>(vy) < static_cast<unsigned>(H);
}

__global__ void __launch_bounds__(kCenterWaves *kWave)
center_nearest_kernel(NearestArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int m = blockIdx.x * kCenterWaves + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave);
  if (m >= a.m_cap) return;                             // (the whole wave: no barrier in this kernel)
  const int b = a.b_batch_ids ? a.b_batch_ids[m] : 0;
  const bool valid = a.cls[m] >= 0 && b >= 0 && b < a.batch;
  int beg = 0, end = 0;
  if (valid) scene_range(a.offsets, a.n_cap, b, beg, end);
  const int live = a.n_live ? min(*a.n_live, a.n_cap) : a.n_cap;
  const float cx = a.center[2 * static_cast<size_t>(m)], cy = a.center[2 * static_cast<size_t>(m) + 1];
  u64 key = ~0ull;
  for (long long pos = static_cast<long long>(beg) + lane; pos < end; pos += kWave) {
    const int ri = a.list[pos];
    int vx, vy;
    if (live_cell(a.indices, ri, live, b, a.W, a.H, vx, vy)) {
      const float dx = static_cast<float>(vx) - cx, dy = static_cast<float>(vy) - cy;
      const float d2 = dx * dx + dy * dy;               // (>= +0 and finite or +inf: its bits order as the values do)
      const u64 k = (static_cast<u64>(__float_as_uint(d2)) << 32) | static_cast<unsigned>(ri);
      key = k < key ? k : key;
    }
  }
#pragma unroll
  for (int s = kWave / 2; s >= 1; s >>= 1) {
    const unsigned lo = __shfl_xor(static_cast<unsigned>(key), s, kWave);
    const unsigned hi = __shfl_xor(static_cast<unsigned>(key >> 32), s, kWave);
    const u64 other = (static_cast<u64>(hi) << 32) | lo;
    key = other < key ? other : key;
  }
  if (lane == 0) a.nearest[m] = key == ~0ull ? -1 : static_cast<int>(key & 0xffffffffu);
}

// One lane per entry of the scene tables, behind center_nearest_kernel: it reads what lanes of that launch stored.
__global__ void __launch_bounds__(256)
center_nearest_table_kernel(NearestArgs a) {
  const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= static_cast<long long>(a.batch) * a.max_objs) return;
  const int bi = a.box_index[e];
  int nr = -1;
  if (a.box_mask[e] != 0 && static_cast<unsigned>(bi) < static_cast<unsigned>(a.m_cap)) nr = a.nearest[bi];
  a.mask[e] = nr >= 0 ? 1 : 0;
  a.inds[e] = nr >= 0 ? nr : 0;
}

// -------------------------------------------------------------------------------------------- sparse

struct SparseHeatArgs {
  const float *center;
  const int32_t *cell, *radius, *cls, *nearest;
  int m_cap;
  const int32_t *offsets, *list, *indices;
  int n_cap;
  const int32_t *n_live;
  int batch, W, H, C, anchor, cutoff;
  float *heat;
};

__global__ void __launch_bounds__(kSceneBlock)
center_sparse_kernel(SparseHeatArgs a) {
  __shared__ float s_cx[kCenterTile], s_cy[kCenterTile];
  __shared__ int s_wx[kCenterTile], s_wy[kCenterTile], s_r[kCenterTile], s_cls[kCenterTile];
  __shared__ int s_next[2][kSceneWaves];
  const long long qi = static_cast<long long>(blockIdx.x) * kSceneBlock + threadIdx.x;
  const int live = a.n_live ? min(*a.n_live, a.n_cap) : a.n_cap;
  int mine = INT_MAX, x = 0, y = 0;                     // (a lane without a live row still takes every barrier)
  if (qi < live) {
    const int b = a.indices[static_cast<size_t>(qi) * 3];
    if (b >= 0 && b < a.batch && live_cell(a.indices, static_cast<int>(qi), live, b, a.W, a.H, x, y)) mine = b;
  }
  const float fx = static_cast<float>(x), fy = static_cast<float>(y);
  int it = 0;                                           // (runs on over the class groups: next_scene's parity rule)
  for (int c0 = 0; c0 < a.C; c0 += kCenterChunk) {
    float best[kCenterChunk];
#pragma unroll
    for (int j = 0; j < kCenterChunk; ++j) best[j] = 0.f;
    int cur = -1;
    for (;; ++it) {
      const int next = next_scene(mine, cur, it, s_next);
      if (next == INT_MAX) {                            // the same LDS words for every lane: uniform
        ++it;
        break;
      }
      cur = next;
      int beg, end;
      scene_range(a.offsets, a.m_cap, next, beg, end);
      for (int tile0 = beg; tile0 < end; tile0 += kCenterTile) {
        const int tn = min(kCenterTile, end - tile0);
        if (static_cast<int>(threadIdx.x) < tn) {
          const int bi = a.list[tile0 + threadIdx.x];
          int cj = -1, wx = 0, wy = 0, r = 0;
          float cx = 0.f, cy = 0.f;
          if (static_cast<unsigned>(bi) < static_cast<unsigned>(a.m_cap)) {
            cj = a.cls[bi] - c0;
            if (static_cast<unsigned>(cj) >= static_cast<unsigned>(kCenterChunk)) cj = -1;   // (another pass, or none)
          }
          if (cj >= 0) {
            r = a.radius[bi];
            cx = a.center[2 * static_cast<size_t>(bi)], cy = a.center[2 * static_cast<size_t>(bi) + 1];
            wx = a.cell[2 * static_cast<size_t>(bi)], wy = a.cell[2 * static_cast<size_t>(bi) + 1];
            if (r < 0 || r > kCenterMaxRadius) cj = -1;
            if (a.anchor == kAnchorNearest) {
              const int nr = a.nearest[bi];
              if (!live_cell(a.indices, nr, live, next, a.W, a.H, wx, wy)) cj = -1;   // no nearest row: draws nothing
            }
          }
          s_cx[threadIdx.x] = cx, s_cy[threadIdx.x] = cy;
          s_wx[threadIdx.x] = wx, s_wy[threadIdx.x] = wy;
          s_r[threadIdx.x] = r, s_cls[threadIdx.x] = cj;
        }
        __syncthreads();
        if (mine == next) {
          for (int k = 0; k < tn; ++k) {
            const int cj = s_cls[k];
            if (cj < 0) continue;
            const int ddx = x - s_wx[k], ddy = y - s_wy[k], rk = s_r[k];
            if (a.cutoff == kCutoffWindow && (abs(ddx) > rk || abs(ddy) > rk)) continue;
            float d2;
            if (a.anchor == kAnchorNearest) {
              d2 = sq_cells(ddx, ddy);
            } else {
              const float dx = fx - s_cx[k], dy = fy - s_cy[k];
              d2 = dx * dx + dy * dy;
            }
            const float v = gauss(d2, rk);
#pragma unroll
            for (int j = 0; j < kCenterChunk; ++j) best[j] = cj == j && v > best[j] ? v : best[j];
          }
        }
        __syncthreads();                                // (the next tile overwrites what this one read)
      }
    }
    if (qi < a.n_cap) {
#pragma unroll
      for (int j = 0; j < kCenterChunk; ++j)
        if (c0 + j < a.C) a.heat[static_cast<size_t>(qi) * a.C + c0 + j] = best[j];
    }
  }
}

// -------------------------------------------------------------------------------------------- host side

// 0 = ok: the checks of a map that need no pointer
int check_center_map(int m_cap, int batch, int W, int H, int C) {
  SPX_CHECK(m_cap >= 0, "bad box counts %d", m_cap);
  SPX_CHECK(batch >= 1 && batch <= 65535, "batch must be in 1 .. 65535, got %d", batch);
  SPX_CHECK(W >= 1 && H >= 1 && W <= kCenterMaxExtent && H <= kCenterMaxExtent,
            "grid_size must be two extents in 1 .. %d, got (%d, %d)", kCenterMaxExtent, W, H);
  SPX_CHECK(C >= 1 && C <= kCenterMaxClasses, "num_classes must be in 1 .. %d, got %d", kCenterMaxClasses, C);
  SPX_CHECK(static_cast<double>(batch) * C * H * W < 2147483648.0,
            "batch * num_classes * H * W must stay below 2^31, got %d x %d x %d x %d", batch, C, H, W);
  return 0;
}

int check_center_rows(int n_cap) {
  SPX_CHECK(n_cap >= 0, "bad row counts %d", n_cap);
  return 0;
}

bool positive(float v) { return v > 0.f && v < __builtin_huge_valf(); }

}  // namespace
}  // namespace spx

extern "C" {

int spx_center_tile(void) { return spx::kCenterTile; }
int spx_center_max_classes(void) { return spx::kCenterMaxClasses; }

int spx_box_centers(const float *boxes, int nfeat, const int32_t *b_batch_ids, const void *class_ids, int class_bytes,
                    int m_cap, const int32_t *n_boxes_dev, const int32_t *box_offsets, const int32_t *box_list, int batch,
                    int W, int H, float vx, float vy, float x0, float y0, float stride, int num_classes, int max_objs,
                    float min_overlap, int min_radius, float *center, int32_t *cell, int32_t *radius, int32_t *cls,
                    int32_t *slot, int32_t *box_index, int32_t *mask, int32_t *inds, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(positive(stride), "stride must be a positive finite float");
  SPX_CHECK(min_overlap > 0.f && min_overlap < 1.f, "min_overlap must lie inside (0, 1)");
  SPX_CHECK(min_radius >= 0 && min_radius <= kCenterMaxRadius, "min_radius must be in 0 .. %d, got %d", kCenterMaxRadius,
            min_radius);
  SPX_CHECK(max_objs >= 1, "max_objs must be >= 1, got %d", max_objs);
  if (int rc = check_center_map(m_cap, batch, W, H, num_classes)) return rc;
  SPX_CHECK(static_cast<long long>(batch) * max_objs < 0x80000000LL, "batch * max_objs must stay below 2^31, got %d x %d",
            batch, max_objs);
  SPX_CHECK(positive(vx) && positive(vy), "voxel_size must be two positive finite floats");
  SPX_CHECK(finite(x0) && finite(y0), "range_min must be two finite floats");
  SPX_CHECK(nfeat >= 7, "boxes need at least 7 columns (x, y, z, dx, dy, dz, heading), got %d", nfeat);
  SPX_CHECK(class_bytes == 4 || class_bytes == 8, "class ids are int32 or int64 (class_bytes 4 or 8), got %d", class_bytes);
  SPX_CHECK(box_offsets && box_index && mask && inds, "box_offsets / box_index / mask / inds is NULL");
  SPX_CHECK(m_cap == 0 || (boxes && box_list && center && cell && radius && cls && slot),
            "boxes / box_list / center / cell / radius / cls / slot is NULL");
  SPX_CHECK(aligned_to(boxes, 4) && aligned_to(b_batch_ids, 4) && aligned_to(class_ids, class_bytes) &&
                aligned_to(n_boxes_dev, 4) && aligned_to(box_offsets, 4) && aligned_to(box_list, 4) && aligned_to(center, 4) &&
                aligned_to(cell, 4) && aligned_to(radius, 4) && aligned_to(cls, 4) && aligned_to(slot, 4) &&
                aligned_to(box_index, 4) && aligned_to(mask, 4) && aligned_to(inds, 4), "pointer not aligned to its elements");
  const CenterArgs a = {boxes, nfeat, b_batch_ids, class_ids, class_bytes, m_cap, n_boxes_dev, box_offsets, box_list, batch,
                        W, H, vx, vy, x0, y0, stride, num_classes, max_objs, min_overlap, min_radius, center, cell, radius,
                        cls, slot, box_index, mask, inds};
  const long long lanes = std::max(static_cast<long long>(m_cap), static_cast<long long>(batch) * max_objs);
  hipLaunchKernelGGL(box_centers_kernel, dim3(static_cast<unsigned>((lanes + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_center_heatmap(const int32_t *cell, const int32_t *radius, const int32_t *cls, int m_cap,
                       const int32_t *box_offsets, const int32_t *box_list, int batch, int W, int H, int num_classes,
                       float *heat, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_center_map(m_cap, batch, W, H, num_classes)) return rc;
  const long long tiles_x = div_up(W, kCenterPatch), tiles_y = div_up(H, kCenterPatch);
  SPX_CHECK(tiles_x * tiles_y < 0x80000000LL, "the map has too many patches: %lld x %lld", tiles_x, tiles_y);
  SPX_CHECK(box_offsets && heat, "box_offsets / heat is NULL");
  SPX_CHECK(m_cap == 0 || (cell && radius && cls && box_list), "cell / radius / cls / box_list is NULL");
  SPX_CHECK(aligned_to(cell, 4) && aligned_to(radius, 4) && aligned_to(cls, 4) && aligned_to(box_offsets, 4) &&
                aligned_to(box_list, 4) && aligned_to(heat, 4), "pointer not aligned to its elements");
  const HeatArgs a = {cell, radius, cls, m_cap, box_offsets, box_list, W, H, num_classes, static_cast<int>(tiles_x), heat};
  const dim3 grid(static_cast<unsigned>(tiles_x * tiles_y), static_cast<unsigned>(num_classes), static_cast<unsigned>(batch));
  hipLaunchKernelGGL(center_heatmap_kernel, grid, dim3(kSceneBlock), 0, static_cast<hipStream_t>(stream), a);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_center_nearest(const float *center, const int32_t *cls, const int32_t *b_batch_ids, int m_cap,
                       const int32_t *indices, int n_cap, const int32_t *n_live_dev, const int32_t *row_offsets,
                       const int32_t *row_list, int batch, int W, int H, const int32_t *box_index, const int32_t *box_mask,
                       int max_objs, int32_t *nearest, int32_t *inds, int32_t *mask, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(max_objs >= 1, "max_objs must be >= 1, got %d", max_objs);
  if (int rc = check_center_map(m_cap, batch, W, H, 1)) return rc;
  if (int rc = check_center_rows(n_cap)) return rc;
  SPX_CHECK(static_cast<long long>(batch) * max_objs < 0x80000000LL, "batch * max_objs must stay below 2^31, got %d x %d",
            batch, max_objs);
  SPX_CHECK(row_offsets && box_index && box_mask && inds && mask, "row_offsets / box_index / box_mask / inds / mask is NULL");
  SPX_CHECK(m_cap == 0 || (center && cls && nearest), "center / cls / nearest is NULL");
  SPX_CHECK(n_cap == 0 || (indices && row_list), "indices / row_list is NULL");
  SPX_CHECK(aligned_to(center, 4) && aligned_to(cls, 4) && aligned_to(b_batch_ids, 4) && aligned_to(indices, 4) &&
                aligned_to(n_live_dev, 4) && aligned_to(row_offsets, 4) && aligned_to(row_list, 4) &&
                aligned_to(box_index, 4) && aligned_to(box_mask, 4) && aligned_to(nearest, 4) && aligned_to(inds, 4) &&
                aligned_to(mask, 4), "pointer not aligned to its elements");
  const NearestArgs a = {center, cls, b_batch_ids, m_cap, indices, n_cap, n_live_dev, row_offsets, row_list, batch, W, H,
                         box_index, box_mask, max_objs, nearest, inds, mask};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (m_cap > 0) {
    hipLaunchKernelGGL(center_nearest_kernel, dim3(div_up(m_cap, kCenterWaves)), dim3(kCenterWaves * kWave), 0, s, a);
    SPX_LAUNCH_CHECK();
  }
  const long long entries = static_cast<long long>(batch) * max_objs;
  hipLaunchKernelGGL(center_nearest_table_kernel, dim3(static_cast<unsigned>((entries + 255) / 256)), dim3(256), 0, s, a);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_center_heatmap_sparse(const float *center, const int32_t *cell, const int32_t *radius, const int32_t *cls,
                              const int32_t *nearest, int m_cap, const int32_t *box_offsets, const int32_t *box_list,
                              const int32_t *indices, int n_cap, const int32_t *n_live_dev, int batch, int W, int H,
                              int num_classes, int anchor, int cutoff, float *heat, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(anchor == kAnchorCenter || anchor == kAnchorNearest, "anchor must be centre (0) or nearest (1), got %d", anchor);
  SPX_CHECK(cutoff == kCutoffNone || cutoff == kCutoffWindow, "cutoff must be none (0) or window (1), got %d", cutoff);
  if (int rc = check_center_map(m_cap, batch, W, H, num_classes)) return rc;
  if (int rc = check_center_rows(n_cap)) return rc;
  SPX_CHECK(static_cast<long long>(n_cap) * num_classes < 0x80000000LL, "n_cap * num_classes must stay below 2^31, got %d x %d",
            n_cap, num_classes);
  if (n_cap == 0) return 0;
  SPX_CHECK(box_offsets && indices && heat, "box_offsets / indices / heat is NULL");
  SPX_CHECK(m_cap == 0 || (center && cell && radius && cls && box_list && (anchor == kAnchorCenter || nearest)),
            "center / cell / radius / cls / nearest / box_list is NULL");
  SPX_CHECK(aligned_to(center, 4) && aligned_to(cell, 4) && aligned_to(radius, 4) && aligned_to(cls, 4) &&
                aligned_to(nearest, 4) && aligned_to(box_offsets, 4) && aligned_to(box_list, 4) && aligned_to(indices, 4) &&
                aligned_to(n_live_dev, 4) && aligned_to(heat, 4), "pointer not aligned to its elements");
  const SparseHeatArgs a = {center, cell, radius, cls, nearest, m_cap, box_offsets, box_list, indices, n_cap, n_live_dev,
                            batch, W, H, num_classes, anchor, cutoff, heat};
  const dim3 grid(static_cast<unsigned>((static_cast<long long>(n_cap) + kSceneBlock - 1) / kSceneBlock));
  hipLaunchKernelGGL(center_sparse_kernel, grid, dim3(kSceneBlock), 0, static_cast<hipStream_t>(stream), a);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
