// Rotated boxes: corners, pairwise overlap / IoU and a non-maximum suppression that stays on the device -- the
// iou3d_nms extension of OpenPCDet / mmdet3d (boxes_iou_bev, boxes_iou3d_gpu, its aligned form, nms_gpu), which every
// detector head ends in and every two-stage head assigns targets through.  The header says what each entry computes;
// tests/refbox.py restates it in numpy float32.  (The record, its load and the clip live in box.h: boxgrad.hip, the
// gradient of aligned pairs, shares them.)
//
//   record    a box in a kernel is a BoxRec: its four bird's-eye corners walked COUNTER-CLOCKWISE (a quad whose signed
//             area is negative is reversed: 3, 2, 1, 0), its bounding rectangle, its area |a| * 0.5f (NaN: the box is
//             invalid), its z range and its class: 16 words, what a staged box is in LDS.
//   clip      Sutherland-Hodgman of the subject quad A against the four edges of B.  The clipped polygon has at most
//             eight vertices and a run-time length: a register array indexed at run time would go to scratch, so the two
//             polygon buffers are PER-LANE LDS SLOTS, s_pa / s_pb [8][lanes] of 8 bytes, slot-major so that the lanes of a
//             wave read consecutive words (no bank conflict).  A lane reads only what it wrote: no barrier.  A ninth vertex
//             (rounding alone can make one) is dropped.
//   pairs     lanes own consecutive COLUMNS (B, the clip edges, in registers: the row stores coalesce); the SUBJECTS of a
//             tile (16 rows; 64 ranks in the NMS mask) are staged as records in LDS once and read as broadcasts.  The
//             bounding-rectangle reject comes before the clip.
//   NMS       key -> spx_serialize (the rank order and the scenes' offsets) -> mask -> reduce, see the header.  In the
//             mask a wave's ballot over its 64 columns IS the word of a row; the reduce is one wave per scene.
// Every barrier sits in control flow that is uniform over the workgroup.  Every float operation is rounded on its own.
#include "common.h"
#include "piece.h"

// no multiply-add pair of this unit may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

#include "box.h"                               // the record, its load and the clip: shared with boxgrad.hip

namespace spx {
namespace {

typedef unsigned long long u64;

constexpr int kBoxBlock = 256;                 // lanes (columns) of a pairwise workgroup
constexpr int kBoxRows = 16;                   // subjects staged per pairwise workgroup
constexpr int kNmsMaxPre = 16384;
constexpr int kModeOverlap = SPX_BOX_OVERLAP_BEV, kModeIouBev = SPX_BOX_IOU_BEV, kModeIou3d = SPX_BOX_IOU_3D;

template <int MODE, int LANES>
__device__ __forceinline__ float pair_value(const BoxRec &A, const BoxRec &B, float2 (&pa)[kMaxPoly][LANES],
                                            float2 (&pb)[kMaxPoly][LANES]) {
  if (!valid(A) || !valid(B)) return 0.f;
  const float inter = overlap_bev<LANES>(A, B, pa, pb);
  if (MODE == kModeOverlap) return inter;
  if (MODE == kModeIouBev) return inter / fmaxf((A.area + B.area) - inter, 1e-8f);
  const float h = fmaxf(fminf(A.zmax, B.zmax) - fmaxf(A.zmin, B.zmin), 0.f);
  const float inter3 = inter * h;
  const float va = A.area * (A.zmax - A.zmin), vb = B.area * (B.zmax - B.zmin);
  return inter3 / fmaxf((va + vb) - inter3, 1e-6f);
}

// -------------------------------------------------------------------------------------------- corners

__global__ void __launch_bounds__(256)
box_corners_kernel(const float *__restrict__ boxes, int nfeat, int n, const int32_t *__restrict__ n_boxes,
                   float *__restrict__ bev, float *__restrict__ zrange) {
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
  ok = ok && b[3] > 0.f && b[4] > 0.f && b[5] > 0.f;
  const float nan = __builtin_nanf("");
  const float c = cosf(b[6]), s = sinf(b[6]);
  const float hx = b[3] * 0.5f, hy = b[4] * 0.5f, hz = b[5] * 0.5f;
  float o[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float lx = (k == 0 || k == 3) ? hx : -hx, ly = k < 2 ? hy : -hy;
    o[2 * k] = ok ? b[0] + (lx * c - ly * s) : nan;
    o[2 * k + 1] = ok ? b[1] + (lx * s + ly * c) : nan;
  }
  float4 *out = reinterpret_cast<float4 *>(bev + static_cast<size_t>(i) * 8);
  out[0] = make_float4(o[0], o[1], o[2], o[3]);
  out[1] = make_float4(o[4], o[5], o[6], o[7]);
  *reinterpret_cast<float2 *>(zrange + static_cast<size_t>(i) * 2) =
      ok ? make_float2(b[2] - hz, b[2] + hz) : make_float2(nan, nan);
}

// -------------------------------------------------------------------------------------------- pairs

struct PairArgs {
  const float *bev_a, *z_a;
  int m;
  const int32_t *n_a;
  const float *bev_b, *z_b;
  int n;
  const int32_t *n_b;
  float *out;
};

template <int MODE>
__global__ void __launch_bounds__(kBoxBlock)
box_pairs_kernel(PairArgs a) {
  __shared__ float2 s_pa[kMaxPoly][kBoxBlock], s_pb[kMaxPoly][kBoxBlock];
  __shared__ BoxRec s_row[kBoxRows];
  const int row0 = blockIdx.x * kBoxRows;
  const long long col = static_cast<long long>(blockIdx.y) * kBoxBlock + threadIdx.x;
  if (threadIdx.x < kBoxRows) {
    const int row = row0 + threadIdx.x;
    const int live = a.n_a ? min(*a.n_a, a.m) : a.m;
    s_row[threadIdx.x] = load_box(a.bev_a, MODE == kModeIou3d ? a.z_a : nullptr, row, row < live, 0);
  }
  const int live_b = a.n_b ? min(*a.n_b, a.n) : a.n;
  const BoxRec B = load_box(a.bev_b, MODE == kModeIou3d ? a.z_b : nullptr, col, col < live_b, 0);
  __syncthreads();
  const int rows = min(kBoxRows, a.m - row0);
  for (int r = 0; r < rows; ++r) {
    const BoxRec A = s_row[r];
    const float v = pair_value<MODE, kBoxBlock>(A, B, s_pa, s_pb);
    if (col < a.n) a.out[static_cast<size_t>(row0 + r) * a.n + col] = v;
  }
}

template <int MODE>
__global__ void __launch_bounds__(kBoxBlock)
box_aligned_kernel(PairArgs a) {
  __shared__ float2 s_pa[kMaxPoly][kBoxBlock], s_pb[kMaxPoly][kBoxBlock];
  const long long i = static_cast<long long>(blockIdx.x) * kBoxBlock + threadIdx.x;
  if (i >= a.n) return;
  const int live_a = a.n_a ? min(*a.n_a, a.n) : a.n, live_b = a.n_b ? min(*a.n_b, a.n) : a.n;
  const BoxRec A = load_box(a.bev_a, MODE == kModeIou3d ? a.z_a : nullptr, i, i < live_a, 0);
  const BoxRec B = load_box(a.bev_b, MODE == kModeIou3d ? a.z_b : nullptr, i, i < live_b, 0);
  a.out[i] = pair_value<MODE, kBoxBlock>(A, B, s_pa, s_pb);
}

// -------------------------------------------------------------------------------------------- NMS

struct NmsArgs {
  const float *bev, *scores;
  const int32_t *batch_ids, *class_ids;
  int n;
  const int32_t *n_boxes;
  int batch;
  float thresh, score_thresh;
  int use_score_thresh;
  int P, W;                 // ranks of a scene that take part: min(pre_max, n); words of a mask row: ceil(P / 64)
  int by_scene;             // mask row of (scene s, rank i): s * P + i, else the sorted position offsets[s] + i
  int post_max;
  u64 *keys;
  int32_t *order, *offsets;
  u64 *mask;
  int32_t *keep, *count;
};

// the sorted positions [beg, beg + c) of the ranks of scene s that take part: offsets checked, not trusted
__device__ __forceinline__ void scene_ranks(const NmsArgs &a, int s, int &beg, int &c) {
  const int lo = min(max(a.offsets[s], 0), a.n), hi = min(max(a.offsets[s + 1], lo), a.n);
  beg = lo;
  c = min(hi - lo, a.P);
}

__device__ __forceinline__ size_t mask_row(const NmsArgs &a, int s, int beg, int i) {
  return a.by_scene ? static_cast<size_t>(s) * a.P + i : static_cast<size_t>(beg) + i;
}

__global__ void __launch_bounds__(256)
nms_key_kernel(NmsArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int live = a.n_boxes ? min(*a.n_boxes, a.n) : a.n;
  u64 key = ~0ull;
  if (i < live) {
    const int b = a.batch_ids ? a.batch_ids[i] : 0;
    const float sc = a.scores[i];
    const float4 u = *reinterpret_cast<const float4 *>(a.bev + static_cast<size_t>(i) * 8);
    const float4 v = *reinterpret_cast<const float4 *>(a.bev + static_cast<size_t>(i) * 8 + 4);
    bool ok = finite(u.x) && finite(u.y) && finite(u.z) && finite(u.w) && finite(v.x) && finite(v.y) && finite(v.z) &&
              finite(v.w);
    ok = ok && b >= 0 && b < a.batch && sc == sc && (!a.use_score_thresh || sc > a.score_thresh);
    if (ok) {
      const uint32_t bits = __float_as_uint(sc);
      const uint32_t ord = bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
      key = (static_cast<u64>(static_cast<uint32_t>(b)) << 32) | static_cast<uint32_t>(~ord);
    }
  }
  a.keys[i] = key;
}

// Workgroup (rb, jb): rb numbers the 64-rank row blocks of all scenes in scene order (found by a walk over the
// offsets), jb is the column block.  Only jb >= ib of an existing row block computes.
__global__ void __launch_bounds__(kWave)
nms_mask_kernel(NmsArgs a) {
  __shared__ float2 s_pa[kMaxPoly][kWave], s_pb[kMaxPoly][kWave];
  __shared__ BoxRec s_row[kWave];
  const int lane = threadIdx.x, jb = blockIdx.y;
  long long rb = blockIdx.x;
  int s = 0, beg = 0, c = 0;
  for (; s < a.batch; ++s) {
    scene_ranks(a, s, beg, c);
    const int nb = (c + kWave - 1) / kWave;
    if (rb < nb) break;
    rb -= nb;
  }
  if (s == a.batch) return;
  const int ib = static_cast<int>(rb);
  if (jb < ib || jb * kWave >= c) return;
  const int i = ib * kWave + lane, j = jb * kWave + lane;
  {
    const int src = i < c ? a.order[beg + i] : -1;
    const bool ok = static_cast<unsigned>(src) < static_cast<unsigned>(a.n);
    s_row[lane] = load_box(a.bev, nullptr, ok ? src : 0, ok, ok && a.class_ids ? a.class_ids[src] : 0);
  }
  const int srcj = j < c ? a.order[beg + j] : -1;
  const bool okj = static_cast<unsigned>(srcj) < static_cast<unsigned>(a.n);
  const BoxRec B = load_box(a.bev, nullptr, okj ? srcj : 0, okj, okj && a.class_ids ? a.class_ids[srcj] : 0);
  __syncthreads();
  const int rows = min(kWave, c - ib * kWave);
  u64 mine = 0ull;
  for (int r = 0; r < rows; ++r) {
    const BoxRec A = s_row[r];
    bool bit = false;
    if (j > ib * kWave + r && A.cls == B.cls && valid(A) && valid(B)) {
      const float inter = overlap_bev<kWave>(A, B, s_pa, s_pb);
      bit = inter / fmaxf((A.area + B.area) - inter, 1e-8f) > a.thresh;
    }
    const u64 word = __ballot(bit);
    mine = lane == r ? word : mine;
  }
  if (i < c) a.mask[mask_row(a, s, beg, i) * a.W + jb] = mine;
}

__device__ __forceinline__ u64 lane_word(u64 v, int t) {            // t uniform
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(v)), t);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(v >> 32)), t);
  return (static_cast<u64>(hi) << 32) | lo;
}
__device__ __forceinline__ u64 uniform_word(u64 v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(v)));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(v >> 32)));
  return (static_cast<u64>(hi) << 32) | lo;
}

// One wave per scene.  Word w of the removed set lives in lane w % 64, slot w / 64 (WPL slots: up to 64 * 64 * WPL ranks).
template <int WPL>
__global__ void __launch_bounds__(kWave)
nms_reduce_kernel(NmsArgs a) {
  const int lane = threadIdx.x, s = blockIdx.x;
  int beg, c;
  scene_ranks(a, s, beg, c);
  const int nblk = (c + kWave - 1) / kWave;
  int32_t *keep = a.keep + static_cast<size_t>(s) * a.post_max;
  u64 rem[WPL];
#pragma unroll
  for (int k = 0; k < WPL; ++k) rem[k] = 0ull;
  int total = 0;
  for (int kb = 0; kb < nblk && total < a.post_max; ++kb) {
    u64 held = rem[0];
#pragma unroll
    for (int k = 1; k < WPL; ++k) held = (kb >> 6) == k ? rem[k] : held;
    u64 r = lane_word(held, kb & 63);
    const int i = kb * kWave + lane;
    const u64 diag = i < c ? a.mask[mask_row(a, s, beg, i) * a.W + kb] : 0ull;
    const int left = c - kb * kWave;
    const u64 exist = left >= kWave ? ~0ull : (1ull << left) - 1ull;
    u64 avail = uniform_word(~r & exist), kept = 0ull;
    const int before = total;
    while (avail != 0ull && total < a.post_max) {
      const int t = __builtin_ctzll(avail);
      kept |= 1ull << t;
      ++total;
      r |= lane_word(diag, t);
      avail = uniform_word(avail & ~r & ~(1ull << t));
    }
    if ((kept >> lane) & 1ull)
      keep[before + __builtin_popcountll(kept & ((1ull << lane) - 1ull))] = a.order[beg + i];
    // the rows of the kept ranks, words beyond this block only (the upper triangle is all that was written)
    for (u64 kk = kept; kk != 0ull; kk &= kk - 1ull) {
      const size_t row = mask_row(a, s, beg, kb * kWave + __builtin_ctzll(kk)) * a.W;
#pragma unroll
      for (int k = 0; k < WPL; ++k) {
        const int w = lane + kWave * k;
        if (w > kb && w < nblk) rem[k] |= a.mask[row + w];
      }
    }
  }
  for (int p = total + lane; p < a.post_max; p += kWave) keep[p] = -1;
  if (lane == 0) a.count[s] = total;
}

// -------------------------------------------------------------------------------------------- host side

int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

bool nms_geometry_ok(int n, int batch, int pre_max) {
  return n >= 0 && batch >= 1 && batch < (1 << 30) && pre_max >= 1 && pre_max <= kNmsMaxPre;
}

// the carve of an NMS workspace
struct NmsWs {
  u64 *keys, *mask;
  int32_t *order, *inverse, *offsets;
  void *sort;
  size_t sort_bytes, bytes;
  int P, W, by_scene;
  NmsWs(void *ws, int n, int batch, int pre_max) {
    Carver cv(ws);
    const size_t nn = n > 0 ? n : 1;
    P = n > 0 ? (pre_max < n ? pre_max : n) : 1;
    W = (P + kWave - 1) / kWave;
    const unsigned long long scene_rows = static_cast<unsigned long long>(batch) * P;
    by_scene = scene_rows < nn ? 1 : 0;
    const size_t rows = by_scene ? static_cast<size_t>(scene_rows) : nn;
    keys = cv.take<u64>(nn);
    order = cv.take<int32_t>(nn);
    inverse = cv.take<int32_t>(nn);
    offsets = cv.take<int32_t>(static_cast<size_t>(batch) + 1);
    sort_bytes = spx_serialize_ws_bytes(n, 1, 32 + bit_length(static_cast<unsigned>(batch)));
    sort = cv.take<char>(sort_bytes);
    mask = cv.take<u64>(rows * W);
    bytes = cv.off;
  }
};

int check_pairs(int m, int n, int mode) {
  SPX_CHECK(mode == kModeOverlap || mode == kModeIouBev || mode == kModeIou3d,
            "mode must be 0 (overlap), 1 (IoU in the plane) or 2 (IoU in space), got %d", mode);
  SPX_CHECK(m >= 0 && n >= 0, "bad box counts %d / %d", m, n);
  return 0;
}

int check_pair_pointers(const spx::PairArgs &a, int mode) {
  SPX_CHECK(a.bev_a && a.bev_b && a.out && (mode != kModeIou3d || (a.z_a && a.z_b)), "corners / zrange / out is NULL");
  SPX_CHECK(aligned_to(a.bev_a, 16) && aligned_to(a.bev_b, 16) && aligned_to(a.z_a, 8) && aligned_to(a.z_b, 8) &&
                aligned_to(a.out, 4) && aligned_to(a.n_a, 4) && aligned_to(a.n_b, 4),
            "pointer not aligned (corners 16 bytes, zrange 8)");
  return 0;
}

}  // namespace
}  // namespace spx

extern "C" {

int spx_boxes_to_corners(const float *boxes, int nfeat, int n, const int32_t *n_boxes_dev, float *bev, float *zrange,
                         spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(n >= 0, "bad box counts %d", n);
  SPX_CHECK(nfeat >= 7, "boxes need at least 7 columns (x, y, z, dx, dy, dz, heading), got %d", nfeat);
  if (n == 0) return 0;
  SPX_CHECK(boxes && bev && zrange, "boxes / bev / zrange is NULL");
  SPX_CHECK(aligned_to(boxes, 4) && aligned_to(bev, 16) && aligned_to(zrange, 8) && aligned_to(n_boxes_dev, 4),
            "pointer not aligned (corners 16 bytes, zrange 8)");
  hipLaunchKernelGGL(box_corners_kernel, dim3(div_up(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), boxes,
                     nfeat, n, n_boxes_dev, bev, zrange);
  SPX_LAUNCH_CHECK();
  spx::count(kBoxCorners);
  return 0;
}

int spx_boxes_overlap(const float *bev_a, const float *zrange_a, int m, const int32_t *n_a_dev, const float *bev_b,
                      const float *zrange_b, int n, const int32_t *n_b_dev, int mode, float *out, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_pairs(m, n, mode)) return rc;
  SPX_CHECK(static_cast<long long>(div_up(n, kBoxBlock)) <= 65535, "at most %d columns, got %d", 65535 * kBoxBlock, n);
  if (m == 0 || n == 0) return 0;
  const PairArgs a = {bev_a, zrange_a, m, n_a_dev, bev_b, zrange_b, n, n_b_dev, out};
  if (int rc = check_pair_pointers(a, mode)) return rc;
  const dim3 grid(div_up(m, kBoxRows), div_up(n, kBoxBlock));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == kModeOverlap)
    hipLaunchKernelGGL(box_pairs_kernel<kModeOverlap>, grid, dim3(kBoxBlock), 0, s, a);
  else if (mode == kModeIouBev)
    hipLaunchKernelGGL(box_pairs_kernel<kModeIouBev>, grid, dim3(kBoxBlock), 0, s, a);
  else
    hipLaunchKernelGGL(box_pairs_kernel<kModeIou3d>, grid, dim3(kBoxBlock), 0, s, a);
  SPX_LAUNCH_CHECK();
  spx::count(kBoxPairs);
  return 0;
}

int spx_boxes_overlap_aligned(const float *bev_a, const float *zrange_a, const int32_t *n_a_dev, const float *bev_b,
                              const float *zrange_b, const int32_t *n_b_dev, int n, int mode, float *out,
                              spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_pairs(n, n, mode)) return rc;
  if (n == 0) return 0;
  const PairArgs a = {bev_a, zrange_a, n, n_a_dev, bev_b, zrange_b, n, n_b_dev, out};
  if (int rc = check_pair_pointers(a, mode)) return rc;
  const dim3 grid(div_up(n, kBoxBlock));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == kModeOverlap)
    hipLaunchKernelGGL(box_aligned_kernel<kModeOverlap>, grid, dim3(kBoxBlock), 0, s, a);
  else if (mode == kModeIouBev)
    hipLaunchKernelGGL(box_aligned_kernel<kModeIouBev>, grid, dim3(kBoxBlock), 0, s, a);
  else
    hipLaunchKernelGGL(box_aligned_kernel<kModeIou3d>, grid, dim3(kBoxBlock), 0, s, a);
  SPX_LAUNCH_CHECK();
  spx::count(kBoxAligned);
  return 0;
}

int spx_nms_max_pre(void) { return spx::kNmsMaxPre; }

size_t spx_nms_ws_bytes(int n, int batch, int pre_max) {
  if (!spx::nms_geometry_ok(n, batch, pre_max)) return 0;
  return spx::NmsWs(nullptr, n, batch, pre_max).bytes;
}

int spx_nms_rotated(const float *bev, const float *scores, const int32_t *batch_ids, const int32_t *class_ids, int n,
                    const int32_t *n_boxes_dev, int batch, float thresh, int use_score_thresh, float score_thresh,
                    int pre_max, int post_max, int32_t *keep, int32_t *count, void *ws, size_t ws_bytes,
                    spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(n >= 0, "bad box counts %d", n);
  SPX_CHECK(batch >= 1 && batch < (1 << 30), "batch must be in 1 .. 2^30 - 1, got %d", batch);
  SPX_CHECK(pre_max >= 1 && pre_max <= kNmsMaxPre, "pre_max must be in 1 .. %d, got %d", kNmsMaxPre, pre_max);
  SPX_CHECK(post_max >= 1 && post_max <= pre_max, "post_max must be in 1 .. pre_max = %d, got %d", pre_max, post_max);
  SPX_CHECK(thresh == thresh, "thresh is NaN");
  SPX_CHECK(use_score_thresh == 0 || use_score_thresh == 1, "use_score_thresh must be 0 or 1, got %d", use_score_thresh);
  SPX_CHECK(!use_score_thresh || score_thresh == score_thresh, "score_thresh is NaN");
  SPX_CHECK(keep && count && (n == 0 || (bev && scores)), "bev / scores / keep / count is NULL");
  SPX_CHECK(aligned_to(bev, 16) && aligned_to(scores, 4) && aligned_to(batch_ids, 4) && aligned_to(class_ids, 4) &&
                aligned_to(n_boxes_dev, 4) && aligned_to(keep, 4) && aligned_to(count, 4) && aligned_to(ws, 256),
            "pointer not aligned (corners 16 bytes, workspace 256)");
  const NmsWs w(ws, n, batch, pre_max);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const NmsArgs a = {bev, scores, batch_ids, class_ids, n, n_boxes_dev, batch, thresh, score_thresh, use_score_thresh,
                     w.P, w.W, w.by_scene, post_max, w.keys, w.order, w.offsets, w.mask, keep, count};
  // SPX_TEST_NMS_STAGES = 1 | 2 | 3 stops behind the key / sort / mask launch: tools/box_probe.py times the prefixes of the
  // pipeline against each other.  Anything but the default leaves keep and count unwritten.
  const int stages = option_int("SPX_TEST_NMS_STAGES", 4);
  if (n > 0) {
    hipLaunchKernelGGL(nms_key_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, a);
    SPX_LAUNCH_CHECK();
    spx::count(kBoxKey);
  }
  if (stages == 1) return 0;
  // (n = 0: the bisection writes the offsets -- all 0 -- and touches neither keys nor order)
  if (int rc = spx_serialize(reinterpret_cast<const uint64_t *>(w.keys), n, 1, 32 + bit_length(static_cast<unsigned>(batch)),
                             batch, 32, w.order, w.inverse, w.offsets, w.sort, w.sort_bytes, stream))
    return rc;
  if (stages == 2) return 0;
  if (n > 0) {
    // row blocks of all scenes together: at most n / 64 + batch, and at most W per scene
    const long long by_n = static_cast<long long>(n) / kWave + batch, by_w = static_cast<long long>(batch) * w.W;
    const long long rbs = by_n < by_w ? by_n : by_w;
    SPX_CHECK(rbs < 0x7fffffffLL, "too many row blocks");
    hipLaunchKernelGGL(nms_mask_kernel, dim3(static_cast<unsigned>(rbs), w.W), dim3(kWave), 0, s, a);
    SPX_LAUNCH_CHECK();
    spx::count(kBoxMask);
  }
  if (stages == 3) return 0;
  if (w.W <= 64)
    hipLaunchKernelGGL(nms_reduce_kernel<1>, dim3(batch), dim3(kWave), 0, s, a);
  else if (w.W <= 128)
    hipLaunchKernelGGL(nms_reduce_kernel<2>, dim3(batch), dim3(kWave), 0, s, a);
  else
    hipLaunchKernelGGL(nms_reduce_kernel<4>, dim3(batch), dim3(kWave), 0, s, a);
  SPX_LAUNCH_CHECK();
  spx::count(kBoxReduce);
  return 0;
}

}  // extern "C"
