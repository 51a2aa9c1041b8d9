// Points in rotated boxes (spx_boxes_to_frames, spx_points_in_boxes, spx_box_query): the geometric test of the
// roiaware_pool3d / roipoint_pool3d extensions of OpenPCDet / mmdet3d (points_in_boxes_gpu, the point stage of
// roipoint_pool3d, the point-to-cell stage of roiaware_pool3d).  The header says what each entry computes;
// tests/refroi.py restates it in numpy float32.  The pooling itself is spx_group_fwd / spx_collapse_fwd over the tables
// written here.
//
//   frame     a box in a kernel is its FRAME: centre, enlarged half sizes, cosine and sine of the heading -- eight words,
//             two 16-byte loads; an invalid box is eight NaNs, which fail every comparison of the test: no branch.
//   point     one lane per point, workgroups of 256 consecutive points, on the scene walk of scenes.h with the roles
//             turned: the points are the walk's queries, the FRAMES of a scene's boxes are what a tile stages (128 of
//             them, read back as broadcasts).  A lane that has its box stops testing and keeps taking the barriers; a
//             scene's remaining tiles are skipped once no lane of the workgroup still looks.
//   box       few boxes, each against a whole scene: a box per WAVE, its 64 lanes testing consecutive entries of the
//             scene's point list, eight batches of 64 in flight and the list entries of the next eight requested
//             ahead.  A ballot and the popcount of the lanes below give every hit its slot: ascending point index, no
//             atomics, no per-lane list, no LDS, no barrier.  The walk goes on past nsample because hits is the total.
//   pad       slots at or beyond count that repeat a kept slot are written by a SECOND launch, one lane per slot: the
//             slot it copies was stored by another lane of the box's wave, and the end of a kernel is the one ordering
//             of those stores that needs no reasoning about caches.
// Every barrier sits in control flow that is uniform over the workgroup.  Every float operation is rounded on its own.
#include "fill.h"
#include "scenes.h"

// no multiply-add pair of this unit may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kRoiBoxTile = 128;               // frames staged per tile of the point-major kernel
constexpr int kRoiWaves = 4;                   // boxes (waves) of a box-major workgroup
constexpr int kRoiAhead = 8;                   // batches of 64 list entries a wave has in flight
constexpr int kRoiMaxSample = 16384, kRoiMaxGrid = 64;
constexpr int kPadFirst = SPX_ROI_PAD_FIRST, kPadCycle = SPX_ROI_PAD_CYCLE;
static_assert(kRoiBoxTile <= kSceneBlock, "one lane stages one frame");

struct Frame {
  float x, y, z, hx, hy, hz, c, s;
};

__device__ __forceinline__ Frame make_frame(const float4 &u, const float4 &v) {
  return Frame{u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
}

// the point in the frame of the box (lx, ly, lz) and whether the box contains it: inclusive in z, strict in the plane
// (check_pt_in_box3d).  False for a frame with a NaN.
__device__ __forceinline__ bool in_frame(const Frame &f, float px, float py, float pz, float &lx, float &ly, float &lz) {
  const float sx = px - f.x, sy = py - f.y;
  lz = pz - f.z;
  lx = sx * f.c + sy * f.s;
  ly = sy * f.c - sx * f.s;
  return fabsf(lz) <= f.hz && lx > -f.hx && lx < f.hx && ly > -f.hy && ly < f.hy;
}

// -------------------------------------------------------------------------------------------- frames

__global__ void __launch_bounds__(256)
box_frames_kernel(const float *__restrict__ boxes, int nfeat, int n, const int32_t *__restrict__ n_boxes, float ex,
                  float ey, float ez, float *__restrict__ frames) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int live = n_boxes ? min(*n_boxes, n) : n;
  float b[7];
  bool ok = i < live;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    b[j] = ok ? boxes[static_cast<size_t>(i) * nfeat + j] : 0.f;
    ok = ok && finite(b[j]);
  }
  ok = ok && b[3] > 0.f && b[4] > 0.f && b[5] > 0.f;      // (the rule of spx_boxes_to_corners, before enlargement)
  const float nan = __builtin_nanf("");
  const float c = cosf(b[6]), s = sinf(b[6]);
  const float hx = b[3] * 0.5f + ex, hy = b[4] * 0.5f + ey, hz = b[5] * 0.5f + ez;
  float4 *out = reinterpret_cast<float4 *>(frames + static_cast<size_t>(i) * 8);
  out[0] = ok ? make_float4(b[0], b[1], b[2], hx) : make_float4(nan, nan, nan, nan);
  out[1] = ok ? make_float4(hy, hz, c, s) : make_float4(nan, nan, nan, nan);
}

// -------------------------------------------------------------------------------------------- point major

// The scene walk with the roles turned: queries / m_cap / n_queries are the POINTS, points / n_cap / offsets / list
// the frame table and the scene list over the box batch ids.
struct InBoxArgs : SceneArgs {
  int32_t *out;
};

__global__ void __launch_bounds__(kSceneBlock)
points_in_boxes_kernel(InBoxArgs a) {
  __shared__ float4 s_frame[kRoiBoxTile][2];
  __shared__ int s_box[kRoiBoxTile];
  __shared__ int s_next[2][kSceneWaves];
  const long long qi = static_cast<long long>(blockIdx.x) * kSceneBlock + threadIdx.x;
  float q[3];
  const int mine = load_scene_query<3>(a, qi, q);       // (a lane without a valid point still takes every barrier)
  int found = -1, cur = -1;
  for (int it = 0;; ++it) {
    const int next = next_scene(mine, cur, it, s_next);
    if (next == INT_MAX) break;                         // the same LDS words for every lane: uniform
    cur = next;
    int beg, end;
    scene_range(a.offsets, a.n_cap, next, beg, end);
    for (int tile0 = beg; tile0 < end; tile0 += kRoiBoxTile) {
      const int tn = min(kRoiBoxTile, end - tile0);
      if (static_cast<int>(threadIdx.x) < tn) {
        const int bi = a.list[tile0 + threadIdx.x];
        const float nan = __builtin_nanf("");
        float4 u = make_float4(nan, nan, nan, nan), v = u;
        if (static_cast<unsigned>(bi) < static_cast<unsigned>(a.n_cap)) {
          u = *reinterpret_cast<const float4 *>(a.points + static_cast<size_t>(bi) * 8);
          v = *reinterpret_cast<const float4 *>(a.points + static_cast<size_t>(bi) * 8 + 4);
        }
        s_frame[threadIdx.x][0] = u;
        s_frame[threadIdx.x][1] = v;
        s_box[threadIdx.x] = bi;
      }
      __syncthreads();
      if (mine == next && found < 0) {
        for (int k = 0; k < tn; ++k) {                  // (ascending box index: the first hit is the lowest)
          const Frame f = make_frame(s_frame[k][0], s_frame[k][1]);
          float lx, ly, lz;
          if (in_frame(f, q[0], q[1], q[2], lx, ly, lz)) {
            found = s_box[k];
            break;
          }
        }
      }
      if (!__syncthreads_or(mine == next && found < 0 ? 1 : 0)) break;   // no lane of this scene still looks: uniform
    }
  }
  if (qi < a.m_cap) a.out[qi] = found;
}

// -------------------------------------------------------------------------------------------- box major

struct BoxQueryArgs {
  const float *frames;
  const int32_t *b_batch_ids;
  int m_cap;
  const int32_t *n_boxes;
  const float *points;
  int nfeat, n_cap;
  const int32_t *offsets, *list;
  int batch;
  int nsample, flags, ox, oy, oz;
  int32_t *rows, *count, *hits;
  float *local;
  int32_t *cells;
};

// entry base + k of a scene's list that ends at `end`, -1 beyond it (no point: load_point's rule for an index)
__device__ __forceinline__ int list_entry(const int32_t *__restrict__ list, long long base, int k, int end) {
  return base + k < end ? list[base + k] : -1;
}

__device__ __forceinline__ int cell_of(float l, float h, float w, int o) {
  return min(max(static_cast<int>((l + h) / w), 0), o - 1);
}

__global__ void __launch_bounds__(kRoiWaves *kWave)
box_query_kernel(BoxQueryArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int m = blockIdx.x * kRoiWaves + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave);
  if (m >= a.m_cap) return;                             // (the whole wave: no barrier in this kernel)
  const int live = a.n_boxes ? min(*a.n_boxes, a.m_cap) : a.m_cap;
  bool valid = m < live;
  int b = 0;
  if (valid) {
    b = a.b_batch_ids ? a.b_batch_ids[m] : 0;
    valid = b >= 0 && b < a.batch;
  }
  const float nan = __builtin_nanf("");
  Frame f = {nan, nan, nan, nan, nan, nan, nan, nan};
  if (valid) {
    f = make_frame(*reinterpret_cast<const float4 *>(a.frames + static_cast<size_t>(m) * 8),
                   *reinterpret_cast<const float4 *>(a.frames + static_cast<size_t>(m) * 8 + 4));
    valid = f.x == f.x;                                 // an invalid box's frame: nothing to walk
  }
  int beg = 0, end = 0;
  if (valid) scene_range(a.offsets, a.n_cap, b, beg, end);
  const size_t row0 = static_cast<size_t>(m) * a.nsample;
  int32_t *ro = a.rows + row0;
  float *lo = a.local ? a.local + row0 * 3 : nullptr;
  int32_t *co = a.cells ? a.cells + row0 : nullptr;
  float wx = 1.f, wy = 1.f, wz = 1.f;
  int cell0 = 0;
  if (co) {
    wx = (f.hx + f.hx) / static_cast<float>(a.ox);
    wy = (f.hy + f.hy) / static_cast<float>(a.oy);
    wz = (f.hz + f.hz) / static_cast<float>(a.oz);
    cell0 = m * (a.ox * a.oy * a.oz);
  }
  const u64 below = (1ull << lane) - 1ull;
  int total = 0;
  // The list entries of the NEXT trip are requested before the points of this one: the walk is two dependent loads deep
  // (entry, then point), and a wave per box has little else in flight.
  int pi[kRoiAhead];
#pragma unroll
  for (int u = 0; u < kRoiAhead; ++u) pi[u] = list_entry(a.list, beg, u * kWave + lane, end);
  for (long long base = beg; base < end; base += kWave * kRoiAhead) {
    float p[kRoiAhead][3];
    int ahead[kRoiAhead];
    bool ok[kRoiAhead];
#pragma unroll
    for (int u = 0; u < kRoiAhead; ++u) ahead[u] = list_entry(a.list, base + kWave * kRoiAhead, u * kWave + lane, end);
#pragma unroll
    for (int u = 0; u < kRoiAhead; ++u) {               // the loads of all batches first: they are independent
      ok[u] = static_cast<unsigned>(pi[u]) < static_cast<unsigned>(a.n_cap);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        p[u][j] = ok[u] ? a.points[static_cast<size_t>(pi[u]) * a.nfeat + j] : 0.f;
        ok[u] = ok[u] && finite(p[u][j]);
      }
    }
#pragma unroll
    for (int u = 0; u < kRoiAhead; ++u) {               // (ascending list position = ascending point index)
      float lx, ly, lz;
      const bool in = in_frame(f, p[u][0], p[u][1], p[u][2], lx, ly, lz) && ok[u];
      const u64 word = __ballot(in);
      const int slot = total + __builtin_popcountll(word & below);
      if (in && slot < a.nsample) {
        ro[slot] = pi[u];
        if (lo) lo[slot * 3] = lx, lo[slot * 3 + 1] = ly, lo[slot * 3 + 2] = lz;
        if (co)
          co[slot] = cell0 + (cell_of(lx, f.hx, wx, a.ox) * a.oy + cell_of(ly, f.hy, wy, a.oy)) * a.oz +
                     cell_of(lz, f.hz, wz, a.oz);
      }
      total += __builtin_popcountll(word);
      pi[u] = ahead[u];
    }
  }
  const int cnt = min(total, a.nsample);
  if (a.flags == 0 || cnt == 0) {                       // (else box_query_pad_kernel writes these slots)
    for (int s = cnt + lane; s < a.nsample; s += kWave) {
      ro[s] = -1;
      if (lo) lo[s * 3] = 0.f, lo[s * 3 + 1] = 0.f, lo[s * 3 + 2] = 0.f;
      if (co) co[s] = -1;
    }
  }
  if (lane == 0) {
    a.count[m] = cnt;
    a.hits[m] = total;
  }
}

// One lane per slot, behind box_query_kernel: a slot at or beyond a count > 0 copies slot 0 (pad first) or slot
// s % count (pad cycle).  It reads slots below count and writes slots at or beyond it: no lane reads what another writes.
__global__ void __launch_bounds__(256)
box_query_pad_kernel(BoxQueryArgs a) {
  const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= static_cast<long long>(a.m_cap) * a.nsample) return;
  const int m = static_cast<int>(e / a.nsample), s = static_cast<int>(e - static_cast<long long>(m) * a.nsample);
  const int cnt = min(a.count[m], a.nsample);
  if (cnt <= 0 || s < cnt) return;
  const int src = (a.flags & kPadCycle) ? s % cnt : 0;
  const size_t row0 = static_cast<size_t>(m) * a.nsample;
  a.rows[row0 + s] = a.rows[row0 + src];
  if (a.cells) a.cells[row0 + s] = a.cells[row0 + src];
  if (a.local) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a.local[(row0 + s) * 3 + j] = a.local[(row0 + src) * 3 + j];
  }
}

// -------------------------------------------------------------------------------------------- host side

// 0 = ok: the checks of a cloud of n_cap points and a table of m_cap boxes that need no pointer
int check_roi(int nfeat, int n_cap, int m_cap, int batch) {
  SPX_CHECK(n_cap >= 0, "bad point counts %d", n_cap);
  SPX_CHECK(m_cap >= 0, "bad box counts %d", m_cap);
  SPX_CHECK(nfeat >= 3, "points need at least 3 columns, got %d", nfeat);
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  return 0;
}

}  // namespace
}  // namespace spx

extern "C" {

int spx_box_query_max_nsample(void) { return spx::kRoiMaxSample; }
int spx_box_query_waves(void) { return spx::kRoiWaves; }
int spx_points_in_boxes_tile(void) { return spx::kRoiBoxTile; }

int spx_boxes_to_frames(const float *boxes, int nfeat, int n, const int32_t *n_boxes_dev, float ex, float ey, float ez,
                        float *frames, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(n >= 0, "bad box counts %d", n);
  SPX_CHECK(nfeat >= 7, "boxes need at least 7 columns (x, y, z, dx, dy, dz, heading), got %d", nfeat);
  SPX_CHECK(ex >= 0.f && ey >= 0.f && ez >= 0.f && ex < __builtin_huge_valf() && ey < __builtin_huge_valf() &&
                ez < __builtin_huge_valf(), "the extra widths must be finite and >= 0 (and no NaN)");
  if (n == 0) return 0;
  SPX_CHECK(boxes && frames, "boxes / frames is NULL");
  SPX_CHECK(aligned_to(boxes, 4) && aligned_to(frames, 16) && aligned_to(n_boxes_dev, 4),
            "pointer not aligned (frames 16 bytes)");
  hipLaunchKernelGGL(box_frames_kernel, dim3(div_up(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), boxes,
                     nfeat, n, n_boxes_dev, ex, ey, ez, frames);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_points_in_boxes(const float *points, int nfeat, const int32_t *p_batch_ids, int n_cap, const int32_t *n_points_dev,
                        const float *frames, int m_cap, const int32_t *box_offsets, const int32_t *box_list, int batch,
                        int32_t *out, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_roi(nfeat, n_cap, m_cap, batch)) return rc;
  if (n_cap == 0) return 0;
  SPX_CHECK(out && aligned_to(out, 4), "out is NULL or not aligned to its elements");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (m_cap == 0) {                                     // no boxes: no walk, every point is in none
    FillList fills;
    fills.add(out, static_cast<size_t>(n_cap) * 4, 0xffffffffu);
    SPX_HIP(fills.launch(s));
    return 0;
  }
  SPX_CHECK(points && frames && box_offsets && box_list, "points / frames / box_offsets / box_list is NULL");
  SPX_CHECK(aligned_to(points, 4) && aligned_to(p_batch_ids, 4) && aligned_to(n_points_dev, 4) && aligned_to(frames, 16) &&
                aligned_to(box_offsets, 4) && aligned_to(box_list, 4), "pointer not aligned (frames 16 bytes)");
  const InBoxArgs a = {{points, nfeat, p_batch_ids, n_cap, n_points_dev, frames, 8, m_cap, box_offsets, box_list, batch},
                       out};
  const dim3 grid(static_cast<unsigned>((static_cast<long long>(n_cap) + kSceneBlock - 1) / kSceneBlock));
  hipLaunchKernelGGL(points_in_boxes_kernel, grid, dim3(kSceneBlock), 0, s, a);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_box_query(const float *frames, const int32_t *b_batch_ids, int m_cap, const int32_t *n_boxes_dev,
                  const float *points, int nfeat, int n_cap, const int32_t *offsets, const int32_t *list, int batch,
                  int nsample, int flags, int ox, int oy, int oz, int32_t *rows, int32_t *count, int32_t *hits,
                  float *local, int32_t *cells, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(nsample >= 1 && nsample <= kRoiMaxSample, "nsample must be in 1 .. %d, got %d", kRoiMaxSample, nsample);
  SPX_CHECK(flags == 0 || flags == kPadFirst || flags == kPadCycle, "flags must be 0, pad first (2) or pad cycle (4), got %d",
            flags);
  const bool no_grid = ox == 0 && oy == 0 && oz == 0;
  SPX_CHECK(no_grid || (ox >= 1 && ox <= kRoiMaxGrid && oy >= 1 && oy <= kRoiMaxGrid && oz >= 1 && oz <= kRoiMaxGrid),
            "the grid must be (0, 0, 0) (none) or three sizes in 1 .. %d, got (%d, %d, %d)", kRoiMaxGrid, ox, oy, oz);
  if (int rc = check_roi(nfeat, n_cap, m_cap, batch)) return rc;
  SPX_CHECK(static_cast<long long>(m_cap) * nsample < 0x80000000LL, "m_cap * nsample must stay below 2^31, got %d x %d",
            m_cap, nsample);
  SPX_CHECK(no_grid || static_cast<long long>(m_cap) * (ox * oy * oz) < 0x80000000LL,
            "m_cap * cells per box must stay below 2^31, got %d x %d", m_cap, ox * oy * oz);
  if (m_cap == 0) return 0;
  SPX_CHECK(rows && count && hits, "rows / count / hits is NULL");
  SPX_CHECK((cells != nullptr) == !no_grid, "cells and a grid come together: cells is %s, the grid (%d, %d, %d)",
            cells ? "given" : "NULL", ox, oy, oz);
  SPX_CHECK(aligned_to(rows, 4) && aligned_to(count, 4) && aligned_to(hits, 4) && aligned_to(local, 4) &&
                aligned_to(cells, 4), "pointer not aligned to its elements");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t slots = static_cast<size_t>(m_cap) * nsample;
  if (n_cap == 0) {                                     // no points: no walk, every box is empty
    FillList fills;
    fills.add(rows, slots * 4, 0xffffffffu);
    fills.add(cells, slots * 4, 0xffffffffu);
    fills.add(count, static_cast<size_t>(m_cap) * 4, 0u);
    fills.add(hits, static_cast<size_t>(m_cap) * 4, 0u);
    fills.add(local, slots * 12, 0u);
    SPX_HIP(fills.launch(s));
    return 0;
  }
  SPX_CHECK(frames && points && offsets && list, "frames / points / offsets / list is NULL");
  SPX_CHECK(aligned_to(frames, 16) && aligned_to(b_batch_ids, 4) && aligned_to(n_boxes_dev, 4) && aligned_to(points, 4) &&
                aligned_to(offsets, 4) && aligned_to(list, 4), "pointer not aligned (frames 16 bytes)");
  const BoxQueryArgs a = {frames, b_batch_ids, m_cap, n_boxes_dev, points, nfeat, n_cap, offsets, list, batch,
                          nsample, flags, ox, oy, oz, rows, count, hits, local, cells};
  const dim3 grid(static_cast<unsigned>((static_cast<long long>(m_cap) + kRoiWaves - 1) / kRoiWaves));
  hipLaunchKernelGGL(box_query_kernel, grid, dim3(kRoiWaves * kWave), 0, s, a);
  SPX_LAUNCH_CHECK();
  if (flags != 0) {
    hipLaunchKernelGGL(box_query_pad_kernel, dim3(static_cast<unsigned>((slots + 255) / 256)), dim3(256), 0, s, a);
    SPX_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
