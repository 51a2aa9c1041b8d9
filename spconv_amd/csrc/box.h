// What the rotated-box units share (box.hip, boxgrad.hip): the record a box is in a kernel, its load from a corner table,
// and the Sutherland-Hodgman clip behind the overlap.  See box.hip for the layout rules.
#pragma once
#include "common.h"

// no multiply-add pair may be contracted into an FMA: every float operation is rounded on its own
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kMaxPoly = 8;

__device__ __forceinline__ bool finite(float v) { return fabsf(v) < __builtin_huge_valf(); }      // (false for NaN)

struct BoxRec {
  float x[4], y[4];
  float minx, maxx, miny, maxy;
  float area, zmin, zmax;
  int cls;
};
static_assert(sizeof(BoxRec) == 64, "a staged box is 16 words");

// Box idx of a corner table (bev [*, 4, 2], zr [*, 2] or null), `exists`: the index lies below the device count.
__device__ __forceinline__ BoxRec load_box(const float *__restrict__ bev, const float *__restrict__ zr, long long idx,
                                           bool exists, int cls) {
  BoxRec r;
  float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
  float2 z = make_float2(0.f, 0.f);
  if (exists) {
    u = *reinterpret_cast<const float4 *>(bev + idx * 8);
    v = *reinterpret_cast<const float4 *>(bev + idx * 8 + 4);
    if (zr) z = *reinterpret_cast<const float2 *>(zr + idx * 2);
  }
  r.x[0] = u.x, r.y[0] = u.y, r.x[1] = u.z, r.y[1] = u.w;
  r.x[2] = v.x, r.y[2] = v.y, r.x[3] = v.z, r.y[3] = v.w;
  bool ok = exists && finite(z.x) && finite(z.y);
#pragma unroll
  for (int k = 0; k < 4; ++k) ok = ok && finite(r.x[k]) && finite(r.y[k]);
  float a = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) a = a + (r.x[k] * r.y[(k + 1) & 3] - r.x[(k + 1) & 3] * r.y[k]);
  if (a < 0.f) {                                // clockwise: walked in reverse, the area that of the reversed walk
    float t;
    t = r.x[0], r.x[0] = r.x[3], r.x[3] = t, t = r.x[1], r.x[1] = r.x[2], r.x[2] = t;
    t = r.y[0], r.y[0] = r.y[3], r.y[3] = t, t = r.y[1], r.y[1] = r.y[2], r.y[2] = t;
    a = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) a = a + (r.x[k] * r.y[(k + 1) & 3] - r.x[(k + 1) & 3] * r.y[k]);
  }
  r.minx = fminf(fminf(r.x[0], r.x[1]), fminf(r.x[2], r.x[3]));
  r.maxx = fmaxf(fmaxf(r.x[0], r.x[1]), fmaxf(r.x[2], r.x[3]));
  r.miny = fminf(fminf(r.y[0], r.y[1]), fminf(r.y[2], r.y[3]));
  r.maxy = fmaxf(fmaxf(r.y[0], r.y[1]), fmaxf(r.y[2], r.y[3]));
  r.area = ok ? fabsf(a) * 0.5f : __builtin_nanf("");
  r.zmin = z.x, r.zmax = z.y;
  r.cls = cls;
  return r;
}

__device__ __forceinline__ bool valid(const BoxRec &r) { return r.area == r.area; }

// Area of A clipped against the four edges of B, 0 when fewer than three vertices are left.  pa / pb: the lane's slots.
template <int LANES>
__device__ __forceinline__ float clip_area(const BoxRec &A, const BoxRec &B, float2 (&pa)[kMaxPoly][LANES],
                                           float2 (&pb)[kMaxPoly][LANES]) {
  const int l = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) pa[k][l] = make_float2(A.x[k], A.y[k]);
  int n = 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float2(&src)[kMaxPoly][LANES] = (e & 1) ? pb : pa;
    float2(&dst)[kMaxPoly][LANES] = (e & 1) ? pa : pb;
    const float ax = B.x[e], ay = B.y[e];
    const float ex = B.x[(e + 1) & 3] - ax, ey = B.y[(e + 1) & 3] - ay;
    float2 p = src[0][l];
    float dp = ex * (p.y - ay) - ey * (p.x - ax);
    const float2 p0 = p;
    const float d0 = dp;
    int m = 0;
    for (int i = 0; i < n; ++i) {
      float2 q = p0;
      float dq = d0;
      if (i + 1 < n) {
        q = src[i + 1][l];
        dq = ex * (q.y - ay) - ey * (q.x - ax);
      }
      const bool ip = dp >= 0.f, iq = dq >= 0.f;
      if (ip) {
        if (m < kMaxPoly) dst[m][l] = p;
        ++m;
      }
      if (ip != iq) {
        const float t = dp / (dp - dq);
        if (m < kMaxPoly) dst[m][l] = make_float2(p.x + t * (q.x - p.x), p.y + t * (q.y - p.y));
        ++m;
      }
      p = q, dp = dq;
    }
    n = min(m, kMaxPoly);
    if (n < 3) return 0.f;
  }
  // (four edges: the result lies in pa)
  float a = 0.f;
  float2 p = pa[0][l];
  const float2 p0 = p;
  for (int i = 0; i < n; ++i) {
    const float2 q = i + 1 < n ? pa[i + 1][l] : p0;
    a = a + (p.x * q.y - q.x * p.y);
    p = q;
  }
  return fabsf(a) * 0.5f;
}

// overlap of the bird's-eye quads of two VALID boxes (the subject first)
template <int LANES>
__device__ __forceinline__ float overlap_bev(const BoxRec &A, const BoxRec &B, float2 (&pa)[kMaxPoly][LANES],
                                             float2 (&pb)[kMaxPoly][LANES]) {
  if (A.maxx < B.minx || B.maxx < A.minx || A.maxy < B.miny || B.maxy < A.miny) return 0.f;
  return fminf(clip_area<LANES>(A, B, pa, pb), fminf(A.area, B.area));
}

}  // namespace
}  // namespace spx
