// Trilinear devoxelisation (spx_point_corners, spx_interp_fwd, spx_interp_bwd): voxel rows of a sparse level
// interpolated to points, the way the point-voxel networks (SPVCNN, PVCNN, the keypoint interpolation of the PV-RCNN
// family) read per-point features out of a sparse level.
//
//   corners   per point the K = 2^ndim voxels whose centres surround it: corner_rows [n_cap, K] (row of the level, -1:
//             outside the grid or no live row there) and corner_w [n_cap, K] (the multilinear weight, 0 where the row
//             is -1).  A coordinate lookup is lookup.h's: one load of the level's rank map for a key-ordered level, or
//             a probe of the builders' hash table, built from the level's rows, for rows in any order.
//   forward   out[i] = sum_c corner_w[i, c] * vfeat[corner_rows[i, c]]: one item per (point, piece), the K loads of a
//             piece in flight together, the sum in ascending c.
//   backward  dvfeat[v] = sum over the entries e = i * K + c of voxel v's group of corner_w[e] * dout[e / K]: a segment
//             sum over the TRANSPOSED corner list, which is spx_point_groups over the flattened corner table (a stable
//             sort: ascending e inside a group).  A voxel's row belongs to a group of G lanes as in collapse.hip, each
//             lane walks the whole list for its pieces (the segment walk of piece.h): no atomics, list order.
// All arithmetic is fp32 (fp64 accumulation for SPX_F64) with every operation rounded on its own, so a host loop
// reproduces every element bit for bit.
#include "common.h"
#include "lookup.h"
#include "piece.h"

// no multiply-add pair of this unit may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kBlock = 256;

// One thread per point.  RANKED: the lookup is rank_of over the level's rank map, else a probe of the table.
template <int NDIM, bool RANKED>
__global__ void __launch_bounds__(kBlock)
corner_kernel(const float *__restrict__ points, int nfeat, const int32_t *__restrict__ batch_ids, int n_cap,
              const int32_t *__restrict__ n_points, PointGeom g, LevelLookup look, int normalise,
              int32_t *__restrict__ corner_rows, float *__restrict__ corner_w) {
  constexpr int K = 1 << NDIM;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_cap) return;
  const RowFinder<RANKED> row_at(look);
  int rows[K];
  float w[K];
#pragma unroll
  for (int c = 0; c < K; ++c) {
    rows[c] = -1;
    w[c] = 0.f;
  }
  int b;
  bool valid = point_batch(g, batch_ids, n_cap, n_points, i, b);
  int base[NDIM] = {};
  float f[NDIM] = {};
  if (valid) {
    const float *pt = points + static_cast<size_t>(i) * nfeat;
#pragma unroll
    for (int j = 0; j < NDIM; ++j) {
      float cell;
      const float tj = point_cell<NDIM>(g, j, pt[j], cell, valid);
      const float gj = tj - 0.5f;
      const float bj = floorf(gj);
      f[j] = gj - bj;
      base[j] = valid ? static_cast<int>(bj) : 0;             // in [-1, extent - 1] for a valid point
    }
  }
  if (valid) {
#pragma unroll
    for (int c = 0; c < K; ++c) {
      long long key = b;
      bool in = true;
      float wc = 1.f;
#pragma unroll
      for (int d = 0; d < NDIM; ++d) {                        // grid axis d = point column j = NDIM - 1 - d
        const int j = NDIM - 1 - d;
        const int v = base[j] + ((c >> j) & 1);
        in = in && static_cast<unsigned>(v) < static_cast<unsigned>(g.level.dims[d]);
        key = key * g.level.dims[d] + v;
      }
#pragma unroll
      for (int j = 0; j < NDIM; ++j) {                        // ((wx * wy) * wz)
        const float wj = ((c >> j) & 1) ? f[j] : 1.0f - f[j];
        wc = j == 0 ? wj : wc * wj;
      }
      const int r = in ? row_at(key) : -1;
      if (r >= 0) {
        rows[c] = r;
        w[c] = wc;
      }
    }
    if (normalise) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < K; ++c)
        if (rows[c] >= 0) s = s + w[c];
#pragma unroll
      for (int c = 0; c < K; ++c) {
        if (s == 0.f) {
          rows[c] = -1;
          w[c] = 0.f;
        } else if (rows[c] >= 0) {
          w[c] = w[c] / s;
        }
      }
    }
  }
  int4 *ro = reinterpret_cast<int4 *>(corner_rows + static_cast<size_t>(i) * K);
  float4 *wo = reinterpret_cast<float4 *>(corner_w + static_cast<size_t>(i) * K);
#pragma unroll
  for (int q = 0; q < K / 4; ++q) {
    ro[q] = make_int4(rows[4 * q], rows[4 * q + 1], rows[4 * q + 2], rows[4 * q + 3]);
    wo[q] = make_float4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
}

// -------------------------------------------------------------------------------------------- forward

// One item per (point, piece): the K corner pieces are loaded together, then added in ascending corner index.
template <int DT, int V, int K>
__global__ void __launch_bounds__(kBlock)
interp_fwd_kernel(const void *__restrict__ vfeat_, int n, const int32_t *__restrict__ corner_rows,
                  const float *__restrict__ corner_w, long long total, int pieces, void *__restrict__ out_) {
  using E = Elem<DT>;
  using S = typename E::S;
  using A = typename E::A;
  using P = Piece<S, V>;
  const P *vfeat = static_cast<const P *>(vfeat_);
  P *out = static_cast<P *>(out_);
  for (long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * kBlock) {
    const long long i = row_of(item, total, pieces);
    const int p = static_cast<int>(item - i * pieces);
    int r[K];
    float w[K];
    P v[K];
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {           // (the point's corner row and weights: 16-byte loads, lanes of a point alike)
      const int4 rq = reinterpret_cast<const int4 *>(corner_rows)[i * (K / 4) + q];
      const float4 wq = reinterpret_cast<const float4 *>(corner_w)[i * (K / 4) + q];
      r[4 * q] = rq.x, r[4 * q + 1] = rq.y, r[4 * q + 2] = rq.z, r[4 * q + 3] = rq.w;
      w[4 * q] = wq.x, w[4 * q + 1] = wq.y, w[4 * q + 2] = wq.z, w[4 * q + 3] = wq.w;
    }
#pragma unroll
    for (int c = 0; c < K; ++c)
      if (static_cast<unsigned>(r[c]) >= static_cast<unsigned>(n)) r[c] = -1;      // (checked, not trusted)
#pragma unroll
    for (int c = 0; c < K; ++c)
      if (r[c] >= 0) v[c] = vfeat[static_cast<long long>(r[c]) * pieces + p];
    A acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = A(0);
#pragma unroll
    for (int c = 0; c < K; ++c) {
      if (r[c] < 0) continue;
      const A wc = static_cast<A>(w[c]);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = acc[j] + (wc * E::up(v[c].e[j]));
    }
    P o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.e[j] = E::down(acc[j]);
    out[item] = o;
  }
}

// -------------------------------------------------------------------------------------------- backward

// Items = (voxel row, lane of its group), the segment walk of piece.h over the transposed corner list: entry e brings
// its weight and the piece of dout row e >> kshift.
template <int DT, int V>
__global__ void __launch_bounds__(kBlock)
interp_bwd_kernel(const void *__restrict__ dout_, int n_cap, int kshift, const float *__restrict__ corner_w,
                  const int32_t *__restrict__ offsets, const int32_t *__restrict__ list, int n, int pieces, int gshift,
                  const int32_t *__restrict__ n_live, void *__restrict__ dvfeat_) {
  using E = Elem<DT>;
  using S = typename E::S;
  using A = typename E::A;
  using P = Piece<S, V>;
  const P *dout = static_cast<const P *>(dout_);
  P *dvfeat = static_cast<P *>(dvfeat_);
  const long long total = static_cast<long long>(n) << gshift;
  const int live = n_live ? min(*n_live, n) : n;
  const int G = 1 << gshift;
  const int entries = n_cap << kshift;
  for (long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * kBlock) {
    const Segment g = segment_of(item, gshift, live, offsets, entries);
    const int r = g.r, beg = g.beg, end = g.end;
    for (int p = g.sub; p < pieces; p += G) {
      A acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = A(0);
      for (int j0 = beg; j0 < end; j0 += kAhead) {
        int e[kAhead];
        float w[kAhead];
        P v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          e[u] = j0 + u < end ? list[j0 + u] : -1;
          if (static_cast<unsigned>(e[u]) >= static_cast<unsigned>(entries)) e[u] = -1;
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u)        // (the loads of four entries in flight together)
          if (e[u] >= 0) {
            w[u] = corner_w[e[u]];
            v[u] = dout[static_cast<long long>(e[u] >> kshift) * pieces + p];
          }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {      // (the additions in list order)
          if (e[u] < 0) continue;
          const A wu = static_cast<A>(w[u]);
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j] = acc[j] + (wu * E::up(v[u].e[j]));
        }
      }
      P o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.e[j] = E::down(acc[j]);
      dvfeat[static_cast<long long>(r) * pieces + p] = o;
    }
  }
}

// -------------------------------------------------------------------------------------------- host side

// 0 = ok: the counts of a corner table [n_cap, 2^ndim] over n rows (ndim checked before)
int check_table(int n_cap, int ndim, int n) {
  SPX_CHECK(n_cap >= 0 && n >= 0, "bad point / row counts %d / %d", n_cap, n);
  SPX_CHECK((static_cast<long long>(n_cap) << ndim) < 0x80000000LL, "n_cap * 2^ndim must stay below 2^31, got %d points", n_cap);
  return 0;
}

// the checks of the two interpolation calls that need no pointer: the bytes of an element, or -1 with the error set
int check_interp(int n_cap, int ndim, int n, int C, int dtype) {
  SPX_CHECK(ndim == 2 || ndim == 3, "ndim must be 2 or 3, got %d", ndim);
  const int eb = float_row_elem(dtype, C);
  if (eb < 0 || check_table(n_cap, ndim, n)) return -1;
  return eb;
}

}  // namespace
}  // namespace spx

extern "C" {

size_t spx_point_corners_ws_bytes(int n_cap, int ndim, int n) {
  if ((ndim != 2 && ndim != 3) || n_cap < 0 || n < 0) return 0;
  if ((static_cast<long long>(n_cap) << ndim) >= 0x80000000LL || n > spx::kMaxRows) return 0;
  return spx::LevelTableWs(nullptr, n).bytes;
}

int spx_point_corners(const float *points, int nfeat, const int32_t *batch_ids, int n_cap, const int32_t *n_points_dev,
                      int ndim, const float *vsize, const float *coors_range, const int32_t *indices, int n,
                      const int32_t *n_live, int batch, const int *spatial_h, const void *rankmap, size_t rankmap_bytes,
                      int flags, int32_t *corner_rows, float *corner_w, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  LevelLookup look;
  if (int rc = check_level("points", ndim, nfeat, n, n_live, batch, spatial_h, vsize, coors_range, rankmap, rankmap_bytes,
                           &look))
    return rc;
  if (int rc = check_table(n_cap, ndim, n)) return rc;
  SPX_CHECK(flags == 0 || flags == 1, "flags must be 0 or 1 (normalise), got %d", flags);
  if (n_cap == 0) return 0;
  SPX_CHECK(points && corner_rows && corner_w && (n == 0 || indices), "points / indices / corner_rows / corner_w is NULL");
  SPX_CHECK(aligned_to(corner_rows, 16) && aligned_to(corner_w, 16), "corner_rows / corner_w not aligned to 16 bytes");
  const PointGeom g(ndim, batch, spatial_h, vsize, coors_range);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool ranked = rankmap != nullptr;
  if (!ranked)
    if (int rc = build_level_table(ws, ws_bytes, indices, n, n_live, g.level, &look.table, s)) return rc;
  dispatch_value<2, 3>(ndim, [&](auto nd) {
    dispatch_value<0, 1>(ranked, [&](auto rk) {
      hipLaunchKernelGGL((corner_kernel<nd, rk != 0>), dim3(div_up(n_cap, kBlock)), dim3(kBlock), 0, s, points, nfeat,
                         batch_ids, n_cap, n_points_dev, g, look, flags & 1, corner_rows, corner_w);
    });
  });
  SPX_LAUNCH_CHECK();
  count(ranked ? kInterpCornersRanked : kInterpCornersHash);
  return 0;
}

int spx_interp_fwd(const void *vfeat, int n, const int32_t *corner_rows, const float *corner_w, int n_cap, int ndim, int C,
                   int dtype, void *out, spx_stream_t stream) {
  using namespace spx;
  const int eb = check_interp(n_cap, ndim, n, C, dtype);
  if (eb < 0) return eb;
  if (n_cap == 0) return 0;
  SPX_CHECK(corner_rows && corner_w && out && (n == 0 || vfeat), "vfeat / corner_rows / corner_w / out is NULL");
  SPX_CHECK(aligned_to(vfeat, eb) && aligned_to(out, eb), "pointer not aligned to its elements");
  SPX_CHECK(aligned_to(corner_rows, 16) && aligned_to(corner_w, 16), "corner_rows / corner_w not aligned to 16 bytes");
  const bool vec = (static_cast<long long>(C) * eb) % 16 == 0 && aligned_to(vfeat, 16) && aligned_to(out, 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_row(dtype, vec, [&](auto dt, auto v) {
    const int pieces = C / v;
    const long long total = static_cast<long long>(n_cap) * pieces;
    dispatch_value<2, 3>(ndim, [&](auto nd) {
      hipLaunchKernelGGL((interp_fwd_kernel<dt, v, (1 << nd)>), dim3(stream_blocks(total, kBlock)), dim3(kBlock), 0, s, vfeat,
                         n, corner_rows, corner_w, total, pieces, out);
    });
  });
  SPX_LAUNCH_CHECK();
  count(kInterpFwd);
  return 0;
}

int spx_interp_bwd(const void *dout, int n_cap, int ndim, const float *corner_w, const int32_t *offsets,
                   const int32_t *list, int n, const int32_t *n_live, int C, int dtype, void *dvfeat,
                   spx_stream_t stream) {
  using namespace spx;
  const int eb = check_interp(n_cap, ndim, n, C, dtype);
  if (eb < 0) return eb;
  if (n == 0) return 0;
  SPX_CHECK(offsets && dvfeat && (n_cap == 0 || (dout && corner_w && list)),
            "dout / corner_w / offsets / list / dvfeat is NULL");
  SPX_CHECK(aligned_to(dout, eb) && aligned_to(dvfeat, eb), "pointer not aligned to its elements");
  const bool vec = (static_cast<long long>(C) * eb) % 16 == 0 && aligned_to(dout, 16) && aligned_to(dvfeat, 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_row(dtype, vec, [&](auto dt, auto v) {
    const int pieces = C / v, gshift = group_shift(pieces);
    hipLaunchKernelGGL((interp_bwd_kernel<dt, v>), dim3(stream_blocks(static_cast<long long>(n) << gshift, kBlock)),
                       dim3(kBlock), 0, s, dout, n_cap, ndim, corner_w, offsets, list, n, pieces, gshift, n_live, dvfeat);
  });
  SPX_LAUNCH_CHECK();
  count(kInterpBwd);
  return 0;
}

}  // extern "C"
