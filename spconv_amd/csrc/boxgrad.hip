// Differentiable rotated IoU: the value and the corner gradients of aligned (prediction, target) pairs, and the backward
// of the corners launch -- what a rotated-IoU regression loss (mmdet3d's RotatedIoU3DLoss over diff_iou_rotated_3d) and
// the IoU-aware / IoU-guided heads train through.  The header gives the order of operations; tests/refboxgrad.py
// restates it in numpy float32.
//
//   value     the forward's own arithmetic (box.h: the record, the rectangle reject, the Sutherland-Hodgman clip in per-lane
//             LDS slots), so that without a penalty the bits are those of spx_boxes_overlap_aligned.
//   gradient  NOT differentiated through the clip.  The gradient of the shared area with respect to the corners is a
//             boundary integral: every one of the eight edges is cut to [t0, t1] by the four half-planes of the other
//             quad, and hands its normal times (w0, w1) to its two corners.  Eight edges x four half-planes, fully
//             unrolled: nothing is indexed at run time, so there is no scratch, no atomic, and no LDS beyond the clip's.
//   lanes     one lane per pair; every table given is written in full by the lane that owns the row.
// Every float operation is rounded on its own.
#include "common.h"
#include "piece.h"

// no multiply-add pair of this unit may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

#include "box.h"

namespace spx {
namespace {

constexpr int kGradBlock = 256;

struct GradArgs {
  const float *bev_a, *z_a;
  const int32_t *n_a;
  const float *bev_b, *z_b;
  const int32_t *n_b;
  int n;
  const float *grad_out;
  float *value, *gbev_a, *gz_a, *gbev_b, *gz_b;
};

// the caller's corners of box idx run clockwise: load_box holds them reversed (its own sum, its own test)
__device__ __forceinline__ bool reversed(const float *__restrict__ bev, long long idx, bool exists) {
  if (!exists) return false;
  const float4 u = *reinterpret_cast<const float4 *>(bev + idx * 8);
  const float4 v = *reinterpret_cast<const float4 *>(bev + idx * 8 + 4);
  const float x[4] = {u.x, u.z, v.x, v.z}, y[4] = {u.y, u.w, v.y, v.w};
  float a = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) a = a + (x[k] * y[(k + 1) & 3] - x[(k + 1) & 3] * y[k]);
  return a < 0.f;
}

// the shoelace gradient of the area of a counter-clockwise quad
__device__ __forceinline__ void area_grad(const BoxRec &R, float (&gx)[4], float (&gy)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    gx[k] = (R.y[(k + 1) & 3] - R.y[(k + 3) & 3]) * 0.5f;
    gy[k] = (R.x[(k + 3) & 3] - R.x[(k + 1) & 3]) * 0.5f;
  }
}

// adds the parts of P's edges inside Q: the gradient of the shared area with respect to the corners of P
__device__ __forceinline__ void edge_integral(const BoxRec &P, const BoxRec &Q, float (&gx)[4], float (&gy)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = (k + 1) & 3;
    const float px = P.x[k], py = P.y[k], qx = P.x[j], qy = P.y[j];
    float t0 = 0.f, t1 = 1.f;
    bool dead = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ax = Q.x[e], ay = Q.y[e];
      const float ex = Q.x[(e + 1) & 3] - ax, ey = Q.y[(e + 1) & 3] - ay;
      const float dp = ex * (py - ay) - ey * (px - ax);
      const float dq = ex * (qy - ay) - ey * (qx - ax);
      const bool ip = dp >= 0.f, iq = dq >= 0.f;
      dead = dead || (!ip && !iq);
      if (ip != iq) {
        const float t = dp / (dp - dq);
        t0 = ip ? t0 : fmaxf(t0, t);
        t1 = ip ? fminf(t1, t) : t1;
      }
    }
    if (!dead && t0 < t1) {
      const float nx = qy - py, ny = px - qx;
      const float w1 = (t1 * t1 - t0 * t0) * 0.5f;
      const float w0 = (t1 - t0) - w1;
      gx[k] = gx[k] + nx * w0;
      gy[k] = gy[k] + ny * w0;
      gx[j] = gx[j] + nx * w1;
      gy[j] = gy[j] + ny * w1;
    }
  }
}

// to the corner of lowest index that attains `hi` + q, to the one that attains `lo` - q: A before B
__device__ __forceinline__ void extreme_grad(const float (&ca)[4], const float (&cb)[4], float lo, float hi, float q,
                                             float (&ga)[4], float (&gb)[4]) {
  bool found_hi = false, found_lo = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool at_hi = !found_hi && ca[k] == hi, at_lo = !found_lo && ca[k] == lo;
    if (at_hi) ga[k] = ga[k] + q;
    if (at_lo) ga[k] = ga[k] - q;
    found_hi = found_hi || at_hi, found_lo = found_lo || at_lo;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool at_hi = !found_hi && cb[k] == hi, at_lo = !found_lo && cb[k] == lo;
    if (at_hi) gb[k] = gb[k] + q;
    if (at_lo) gb[k] = gb[k] - q;
    found_hi = found_hi || at_hi, found_lo = found_lo || at_lo;
  }
}

// the corner gradients of a record at the caller's indices: [4, 2] of one row
__device__ __forceinline__ void store_corners(float *__restrict__ out, long long i, const float (&gx)[4],
                                              const float (&gy)[4], bool rev, bool ok) {
  float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
  if (ok) {
    u = rev ? make_float4(gx[3], gy[3], gx[2], gy[2]) : make_float4(gx[0], gy[0], gx[1], gy[1]);
    v = rev ? make_float4(gx[1], gy[1], gx[0], gy[0]) : make_float4(gx[2], gy[2], gx[3], gy[3]);
  }
  reinterpret_cast<float4 *>(out + i * 8)[0] = u;
  reinterpret_cast<float4 *>(out + i * 8)[1] = v;
}

template <bool SPACE, bool DIOU>
__global__ void __launch_bounds__(kGradBlock)
box_pair_grad_kernel(GradArgs a) {
  __shared__ float2 s_pa[kMaxPoly][kGradBlock], s_pb[kMaxPoly][kGradBlock];
  const long long i = static_cast<long long>(blockIdx.x) * kGradBlock + threadIdx.x;
  if (i >= a.n) return;
  const int live_a = a.n_a ? min(*a.n_a, a.n) : a.n, live_b = a.n_b ? min(*a.n_b, a.n) : a.n;
  const BoxRec A = load_box(a.bev_a, SPACE ? a.z_a : nullptr, i, i < live_a, 0);
  const BoxRec B = load_box(a.bev_b, SPACE ? a.z_b : nullptr, i, i < live_b, 0);
  const bool ok = valid(A) && valid(B);
  const bool want_grad = a.gbev_a || a.gz_a || a.gbev_b || a.gz_b;        // (uniform)
  const float aa = A.area, ab = B.area;

  // ---- inter and its gradient
  float gix_a[4] = {0.f, 0.f, 0.f, 0.f}, giy_a[4] = {0.f, 0.f, 0.f, 0.f};
  float gix_b[4] = {0.f, 0.f, 0.f, 0.f}, giy_b[4] = {0.f, 0.f, 0.f, 0.f};
  float gax_a[4], gay_a[4], gax_b[4], gay_b[4];
  area_grad(A, gax_a, gay_a);
  area_grad(B, gax_b, gay_b);
  const float small = fminf(aa, ab);
  float inter = 0.f;
  const bool apart = A.maxx < B.minx || B.maxx < A.minx || A.maxy < B.miny || B.maxy < A.miny;
  if (ok && !apart) {
    const float clip = clip_area<kGradBlock>(A, B, s_pa, s_pb);
    inter = fminf(clip, small);
    if (want_grad) {
      if (clip > small) {                       // the clamp binds: the smaller area, to that box alone (a tie: A)
        const bool to_a = aa <= ab;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          gix_a[k] = to_a ? gax_a[k] : 0.f, giy_a[k] = to_a ? gay_a[k] : 0.f;
          gix_b[k] = to_a ? 0.f : gax_b[k], giy_b[k] = to_a ? 0.f : gay_b[k];
        }
      } else {
        edge_integral(A, B, gix_a, giy_a);
        edge_integral(B, A, gix_b, giy_b);
      }
    }
  }

  // ---- the value, and the coefficients of d inter, d area, d h and d height
  float hraw = 1.f, h = 1.f, ha = 1.f, hb = 1.f, i3 = inter, sa = aa, sb = ab;
  if (SPACE) {
    hraw = fminf(A.zmax, B.zmax) - fmaxf(A.zmin, B.zmin);
    h = fmaxf(hraw, 0.f);
    ha = A.zmax - A.zmin, hb = B.zmax - B.zmin;
    i3 = inter * h;
    sa = aa * ha, sb = ab * hb;
  }
  const float floor_u = SPACE ? 1e-6f : 1e-8f;
  const float s = sa + sb;
  const float uraw = s - i3;
  const float u = fmaxf(uraw, floor_u);
  float value = i3 / u;
  const float go = a.grad_out ? a.grad_out[i] : 1.f;
  float ci, cs;
  if (uraw > floor_u) {
    const float u2 = u * u;
    ci = s / u2, cs = i3 / u2;
  } else {
    ci = 1.f / u, cs = 0.f;
  }
  const float ki = go * ci, ks = go * cs;
  float kin = ki, kaa = ks, kab = ks, kh = 0.f, kha = 0.f, khb = 0.f;
  if (SPACE) {
    kin = ki * h, kh = ki * inter;
    kaa = ks * ha, kab = ks * hb;
    kha = ks * aa, khb = ks * ab;
  }
  float gxa[4], gya[4], gxb[4], gyb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    gxa[k] = kin * gix_a[k] - kaa * gax_a[k], gya[k] = kin * giy_a[k] - kaa * gay_a[k];
    gxb[k] = kin * gix_b[k] - kab * gax_b[k], gyb[k] = kin * giy_b[k] - kab * gay_b[k];
  }
  float gza[2] = {0.f, 0.f}, gzb[2] = {0.f, 0.f};
  if (SPACE) {
    const float th = hraw > 0.f ? kh : 0.f;
    const bool top_a = A.zmax <= B.zmax, bot_a = A.zmin >= B.zmin;      // a tie goes to A
    gza[0] = kha - (bot_a ? th : 0.f), gza[1] = (top_a ? th : 0.f) - kha;
    gzb[0] = khb - (bot_a ? 0.f : th), gzb[1] = (top_a ? 0.f : th) - khb;
  }

  // ---- DIoU: minus the squared centre distance over the squared diagonal of the enclosing axis-aligned box
  if (DIOU) {
    const float dx = (A.x[0] + A.x[2]) * 0.5f - (B.x[0] + B.x[2]) * 0.5f;
    const float dy = (A.y[0] + A.y[2]) * 0.5f - (B.y[0] + B.y[2]) * 0.5f;
    float rho2 = dx * dx + dy * dy;
    const float x0 = fminf(A.minx, B.minx), x1 = fmaxf(A.maxx, B.maxx);
    const float y0 = fminf(A.miny, B.miny), y1 = fmaxf(A.maxy, B.maxy);
    const float w = x1 - x0, v = y1 - y0;
    float c2 = w * w + v * v;
    float dz = 0.f, d = 0.f;
    if (SPACE) {
      dz = (A.zmin + A.zmax) * 0.5f - (B.zmin + B.zmax) * 0.5f;
      rho2 = rho2 + dz * dz;
      d = fmaxf(A.zmax, B.zmax) - fminf(A.zmin, B.zmin);
      c2 = c2 + d * d;
    }
    const float c = fmaxf(c2, 1e-12f);
    value = value - rho2 / c;
    const float kr = go / c;
    const float kc = c2 > 1e-12f ? go * (rho2 / (c * c)) : 0.f;
    const float px = kr * dx, py = kr * dy;     // d rho2 / d centre = 2 * (the difference); a corner has half of it
    gxa[0] = gxa[0] - px, gya[0] = gya[0] - py, gxa[2] = gxa[2] - px, gya[2] = gya[2] - py;
    gxb[0] = gxb[0] + px, gyb[0] = gyb[0] + py, gxb[2] = gxb[2] + px, gyb[2] = gyb[2] + py;
    extreme_grad(A.x, B.x, x0, x1, kc * (w + w), gxa, gxb);
    extreme_grad(A.y, B.y, y0, y1, kc * (v + v), gya, gyb);
    if (SPACE) {
      const float pz = kr * dz;
      gza[0] = gza[0] - pz, gza[1] = gza[1] - pz;
      gzb[0] = gzb[0] + pz, gzb[1] = gzb[1] + pz;
      const float qz = kc * (d + d);
      if (A.zmax >= B.zmax) gza[1] = gza[1] + qz; else gzb[1] = gzb[1] + qz;
      if (A.zmin <= B.zmin) gza[0] = gza[0] - qz; else gzb[0] = gzb[0] - qz;
    }
  }

  if (a.value) a.value[i] = ok ? value : 0.f;
  if (a.gbev_a) store_corners(a.gbev_a, i, gxa, gya, reversed(a.bev_a, i, i < live_a), ok);
  if (a.gbev_b) store_corners(a.gbev_b, i, gxb, gyb, reversed(a.bev_b, i, i < live_b), ok);
  if (a.gz_a) *reinterpret_cast<float2 *>(a.gz_a + i * 2) = ok ? make_float2(gza[0], gza[1]) : make_float2(0.f, 0.f);
  if (a.gz_b) *reinterpret_cast<float2 *>(a.gz_b + i * 2) = ok ? make_float2(gzb[0], gzb[1]) : make_float2(0.f, 0.f);
}

// -------------------------------------------------------------------------------------------- corners, backward

__global__ void __launch_bounds__(256)
box_corners_bwd_kernel(const float *__restrict__ boxes, int nfeat, int n, const int32_t *__restrict__ n_boxes,
                       const float *__restrict__ gbev, const float *__restrict__ gzrange, float *__restrict__ gboxes) {
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
  const float c = cosf(b[6]), s = sinf(b[6]);
  const float hx = b[3] * 0.5f, hy = b[4] * 0.5f;
  const float4 u = *reinterpret_cast<const float4 *>(gbev + static_cast<size_t>(i) * 8);
  const float4 v = *reinterpret_cast<const float4 *>(gbev + static_cast<size_t>(i) * 8 + 4);
  const float gx[4] = {u.x, u.z, v.x, v.z}, gy[4] = {u.y, u.w, v.y, v.w};
  float2 gz = make_float2(0.f, 0.f);
  if (gzrange) gz = *reinterpret_cast<const float2 *>(gzrange + static_cast<size_t>(i) * 2);
  float o[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool px = k == 0 || k == 3, py = k < 2;                      // the corner's signs in x and y
    const float lx = px ? hx : -hx, ly = py ? hy : -hy;
    const float along = gx[k] * c + gy[k] * s, across = gy[k] * c - gx[k] * s;
    o[0] = o[0] + gx[k];
    o[1] = o[1] + gy[k];
    o[3] = px ? o[3] + along : o[3] - along;
    o[4] = py ? o[4] + across : o[4] - across;
    o[6] = o[6] + (gy[k] * (lx * c - ly * s) - gx[k] * (lx * s + ly * c));
  }
  o[2] = gz.x + gz.y;
  o[3] = o[3] * 0.5f;
  o[4] = o[4] * 0.5f;
  o[5] = (gz.y - gz.x) * 0.5f;
  float *out = gboxes + static_cast<size_t>(i) * nfeat;
#pragma unroll
  for (int j = 0; j < 7; ++j) out[j] = ok ? o[j] : 0.f;
  for (int j = 7; j < nfeat; ++j) out[j] = 0.f;
}

}  // namespace
}  // namespace spx

extern "C" {

int spx_boxes_iou_aligned_grad(const float *bev_a, const float *zrange_a, const int32_t *n_a_dev, const float *bev_b,
                               const float *zrange_b, const int32_t *n_b_dev, int n, int mode, int penalty,
                               const float *grad_out, float *value, float *gbev_a, float *gz_a, float *gbev_b,
                               float *gz_b, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(mode == SPX_BOX_IOU_BEV || mode == SPX_BOX_IOU_3D,
            "mode must be 1 (IoU in the plane) or 2 (IoU in space), got %d", mode);
  SPX_CHECK(penalty == SPX_BOX_PENALTY_NONE || penalty == SPX_BOX_PENALTY_DIOU,
            "penalty must be 0 (none) or 1 (DIoU), got %d", penalty);
  SPX_CHECK(n >= 0, "bad box counts %d", n);
  if (n == 0) return 0;
  const bool space = mode == SPX_BOX_IOU_3D;
  SPX_CHECK(bev_a && bev_b && (!space || (zrange_a && zrange_b)), "corners / zrange is NULL");
  SPX_CHECK(aligned_to(bev_a, 16) && aligned_to(bev_b, 16) && aligned_to(zrange_a, 8) && aligned_to(zrange_b, 8) &&
                aligned_to(gbev_a, 16) && aligned_to(gbev_b, 16) && aligned_to(gz_a, 8) && aligned_to(gz_b, 8) &&
                aligned_to(value, 4) && aligned_to(grad_out, 4) && aligned_to(n_a_dev, 4) && aligned_to(n_b_dev, 4),
            "pointer not aligned (corners and their gradients 16 bytes, zrange and its gradients 8)");
  const GradArgs a = {bev_a, zrange_a, n_a_dev, bev_b, zrange_b, n_b_dev, n, grad_out, value, gbev_a, gz_a, gbev_b, gz_b};
  const dim3 grid(div_up(n, kGradBlock)), block(kGradBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (space && penalty)
    hipLaunchKernelGGL((box_pair_grad_kernel<true, true>), grid, block, 0, s, a);
  else if (space)
    hipLaunchKernelGGL((box_pair_grad_kernel<true, false>), grid, block, 0, s, a);
  else if (penalty)
    hipLaunchKernelGGL((box_pair_grad_kernel<false, true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((box_pair_grad_kernel<false, false>), grid, block, 0, s, a);
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_boxes_to_corners_bwd(const float *boxes, int nfeat, int n, const int32_t *n_boxes_dev, const float *gbev,
                             const float *gzrange, float *gboxes, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(n >= 0, "bad box counts %d", n);
  SPX_CHECK(nfeat >= 7, "boxes need at least 7 columns (x, y, z, dx, dy, dz, heading), got %d", nfeat);
  if (n == 0) return 0;
  SPX_CHECK(boxes && gbev && gboxes, "boxes / gbev / gboxes is NULL");
  SPX_CHECK(aligned_to(boxes, 4) && aligned_to(gbev, 16) && aligned_to(gzrange, 8) && aligned_to(gboxes, 4) &&
                aligned_to(n_boxes_dev, 4),
            "pointer not aligned (corner gradients 16 bytes, zrange gradients 8)");
  hipLaunchKernelGGL(box_corners_bwd_kernel, dim3(div_up(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), boxes,
                     nfeat, n, n_boxes_dev, gbev, gzrange, gboxes);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
