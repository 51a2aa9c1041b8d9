// Point <-> voxel features (spx_point_groups, spx_voxel_to_point, spx_point_decorate): what a learned voxel feature
// encoder (DynamicVFE) needs between the voxeliser and the first sparse layer.
//
//   groups    the points of every voxel as {rows, offsets, list}, the group form spx_collapse_fwd / _bwd reduce:
//             key     rows[i] = the point's voxel, or -1; its SORT KEY = the voxel, or num_voxels for a point without
//                     one (behind *n_points, id outside [0, num_voxels)), so that those trail.
//             list    a STABLE argsort of the points by that key (the LSD radix of rowsort.hip on
//                     ceil(log2(num_voxels + 1)) bits) IS the list: ascending point index inside a group -- the order
//                     contract comes from the sort's stability, as in collapse.hip.
//             bounds  offsets[v] = first sorted position whose key is >= v, a bisection per voxel.  Voxel ids, unlike
//                     collapse.hip's ranks, have gaps (empty voxels, runs of them): a bisection costs the same for every
//                     v, where a walk from each boundary would hand a run of empty voxels to one thread.
//   gather    out[i] = vfeat[rows[i]] or the fill element: a byte-moving copy, one item per (point, piece).
//   decorate  the MLP's input row: the point, its offset from the voxel's cluster mean, its offset from the voxel
//             centre, zero padding; fp32 with every operation rounded on its own, one rounding into the output type.
// The reductions themselves (sum / mean / max over all points of a voxel, and the gather's gradient = a segment sum)
// are collapse.hip's kernels over these groups: no atomics, list order, one rounding.
#include <string.h>

#include "common.h"
#include "piece.h"

// The decoration promises float32 results a host reproduces bit for bit: no multiply-add pair of this unit may be
// contracted into an FMA.  (hipcc's __fmul_rn / __fadd_rn / __fsub_rn are the plain operators compiled under the
// contraction mode of where they are DEFINED, so two of them can still fuse; the operators below are written here.)
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ float f32_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float f32_add(float a, float b) { return a + b; }
__device__ __forceinline__ float f32_sub(float a, float b) { return a - b; }

// -------------------------------------------------------------------------------------------- groups

template <typename ID>
__global__ void __launch_bounds__(kBlock)
pv_key_kernel(const ID *__restrict__ ids, int n_cap, const int32_t *__restrict__ n_points, int num_voxels,
              int32_t *__restrict__ rows, uint32_t *__restrict__ sortkey) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_cap) return;
  const int n = n_points ? *n_points : n_cap;
  const long long v = i < n ? static_cast<long long>(ids[i]) : -1;
  const bool ok = v >= 0 && v < num_voxels;
  rows[i] = ok ? static_cast<int32_t>(v) : -1;
  sortkey[i] = ok ? static_cast<uint32_t>(v) : static_cast<uint32_t>(num_voxels);
}

// offsets[v] = the first position t of the sorted order with key >= v, v = 0 .. num_voxels (n = 0: all zero)
__global__ void __launch_bounds__(kBlock)
pv_offsets_kernel(const uint32_t *__restrict__ sortkey, const int32_t *__restrict__ list, int n, int num_voxels,
                  int32_t *__restrict__ offsets) {
  const long long v = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (v > num_voxels) return;
  unsigned lo = 0, hi = static_cast<unsigned>(n);
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    const unsigned src = static_cast<unsigned>(list[mid]);
    const uint32_t k = src < static_cast<unsigned>(n) ? sortkey[src] : 0xffffffffu;      // (checked, not trusted)
    if (k < static_cast<uint32_t>(v)) lo = mid + 1; else hi = mid;
  }
  offsets[v] = static_cast<int32_t>(lo);
}

// -------------------------------------------------------------------------------------------- gather

// One item per (point, piece), consecutive lanes on consecutive pieces of a row.  pshift >= 0: pieces = 1 << pshift.
template <typename P>
__global__ void __launch_bounds__(kBlock)
pv_gather_kernel(const P *__restrict__ vfeat, int num_voxels, const int32_t *__restrict__ rows, long long total,
                 int pieces, int pshift, P fill, P *__restrict__ out) {
  for (long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * kBlock) {
    const long long i = pshift >= 0 ? item >> pshift : row_of(item, total, pieces);
    const int p = static_cast<int>(item - i * pieces);
    const int r = rows[i];
    out[item] = static_cast<unsigned>(r) < static_cast<unsigned>(num_voxels)
                    ? vfeat[static_cast<long long>(r) * pieces + p] : fill;
  }
}

// -------------------------------------------------------------------------------------------- decorate

struct DecoGeom {
  int ndim;
  float vsize[kMaxNdim], lo[kMaxNdim];      // by POINT COLUMN (x, y, z): entry j belongs to index column ndim - j
};

__device__ __forceinline__ float pick(const float (&a)[kMaxNdim], int j) {
  float v = a[0];
#pragma unroll
  for (int d = 1; d < kMaxNdim; ++d) v = j == d ? a[d] : v;
  return v;
}

// column c of the decorated row of a point with voxel r >= 0
__device__ __forceinline__ float deco_value(const float *__restrict__ pt, int nfeat, int r,
                                            const int32_t *__restrict__ indices, const DecoGeom &g,
                                            const float *__restrict__ mean, int flags, int c) {
  if (c < nfeat) return pt[c];
  c -= nfeat;
  if (flags & 1) {
    if (c < g.ndim) return f32_sub(pt[c], mean[static_cast<long long>(r) * nfeat + c]);
    c -= g.ndim;
  }
  if ((flags & 2) && c < g.ndim) {
    const int cell = indices[static_cast<long long>(r) * (g.ndim + 1) + (g.ndim - c)];
    const float centre = f32_add(f32_mul(f32_add(static_cast<float>(cell), 0.5f), pick(g.vsize, c)), pick(g.lo, c));
    return f32_sub(pt[c], centre);
  }
  return 0.f;
}

// One item per (point, piece of its output row): V consecutive columns, one store.
template <int DT, int V>
__global__ void __launch_bounds__(kBlock)
pv_decorate_kernel(const float *__restrict__ points, int nfeat, long long total, int pieces,
                   const int32_t *__restrict__ rows, const int32_t *__restrict__ indices, DecoGeom g,
                   const float *__restrict__ mean, int flags, void *__restrict__ out_) {
  using E = Elem<DT>;
  using P = Piece<typename E::S, V>;
  P *out = static_cast<P *>(out_);
  for (long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * kBlock) {
    const long long i = row_of(item, total, pieces);
    const int p = static_cast<int>(item - i * pieces);
    const int r = rows[i];
    const float *pt = points + i * nfeat;
    P v;
#pragma unroll
    for (int j = 0; j < V; ++j)
      v.e[j] = E::down(r >= 0 ? deco_value(pt, nfeat, r, indices, g, mean, flags, p * V + j) : 0.f);
    out[item] = v;
  }
}

template <typename P>
void launch_gather(const void *vfeat, int num_voxels, const int32_t *rows, long long n_rows, int pieces, const void *fill16,
                   void *out, hipStream_t s) {
  P fill;
  memcpy(&fill, fill16, sizeof(P));
  int pshift = -1;
  for (int b = 0; b < 31; ++b)
    if (pieces == (1 << b)) pshift = b;
  const long long total = n_rows * pieces;
  hipLaunchKernelGGL(pv_gather_kernel<P>, dim3(stream_blocks(total, kBlock)), dim3(kBlock), 0, s,
                     static_cast<const P *>(vfeat), num_voxels, rows, total, pieces, pshift, fill, static_cast<P *>(out));
}

// scratch of a groups build: the points' sort keys, the radix sort's buffers
struct GroupsWs {
  uint32_t *sortkey;
  void *sort;
  size_t bytes;
  GroupsWs(void *ws, int n) {
    Carver c(ws);
    sortkey = c.take<uint32_t>(n > 0 ? n : 1);
    sort = c.take<char>(radix_argsort_ws_bytes(n));
    bytes = c.off;
  }
};

}  // namespace

// the gather declared in common.h (its callers: spx_voxel_to_point, spx_group_fwd of query.hip): 16-byte pieces where
// the row's byte count and both pointers allow them, else one element of 1, 2, 4 or 8 bytes
int gather_rows(const void *src, int n_src, const int32_t *rows, long long n_rows, int C, int elem_bytes,
                const void *fill16, void *out, hipStream_t s) {
  const long long row_bytes = static_cast<long long>(C) * elem_bytes;
  const bool vec = row_bytes % 16 == 0 && aligned_to(src, 16) && aligned_to(out, 16);
  if (vec) launch_gather<uint4>(src, n_src, rows, n_rows, static_cast<int>(row_bytes / 16), fill16, out, s);
  else if (elem_bytes == 8) launch_gather<unsigned long long>(src, n_src, rows, n_rows, C, fill16, out, s);
  else if (elem_bytes == 4) launch_gather<uint32_t>(src, n_src, rows, n_rows, C, fill16, out, s);
  else if (elem_bytes == 2) launch_gather<uint16_t>(src, n_src, rows, n_rows, C, fill16, out, s);
  else launch_gather<uint8_t>(src, n_src, rows, n_rows, C, fill16, out, s);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // namespace spx

extern "C" {

size_t spx_point_groups_ws_bytes(int n_cap, int num_voxels) {
  if (n_cap < 0 || num_voxels < 1) return 0;
  return spx::GroupsWs(nullptr, n_cap).bytes;
}

int spx_point_groups(const void *ids, int id_bytes, int n_cap, const int32_t *n_points_dev, int num_voxels,
                     int32_t *rows, int32_t *offsets, int32_t *list, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(id_bytes == 8 || id_bytes == 4, "id_bytes must be 8 (int64) or 4 (int32), got %d", id_bytes);
  SPX_CHECK(n_cap >= 0, "bad point count %d", n_cap);
  SPX_CHECK(num_voxels >= 1 && num_voxels < 0x7fffffff, "num_voxels must be in [1, 2^31 - 2], got %d", num_voxels);
  SPX_CHECK(offsets && (n_cap == 0 || (ids && rows && list)), "ids / rows / offsets / list is NULL");
  SPX_CHECK(aligned_to(ids, id_bytes), "ids not aligned to its elements");
  GroupsWs w(ws, n_cap);
  SPX_CHECK(n_cap == 0 || (ws && ws_bytes >= w.bytes), "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_cap > 0) {
    const dim3 gp(div_up(n_cap, kBlock));
    if (id_bytes == 8)
      hipLaunchKernelGGL(pv_key_kernel<long long>, gp, dim3(kBlock), 0, s, static_cast<const long long *>(ids), n_cap,
                         n_points_dev, num_voxels, rows, w.sortkey);
    else
      hipLaunchKernelGGL(pv_key_kernel<int32_t>, gp, dim3(kBlock), 0, s, static_cast<const int32_t *>(ids), n_cap,
                         n_points_dev, num_voxels, rows, w.sortkey);
    SPX_LAUNCH_CHECK();
    if (int rc = radix_argsort(w.sortkey, n_cap, key_bits(static_cast<uint32_t>(num_voxels)), list, w.sort, s)) return rc;
  }
  // (n_cap = 0: the bisection touches neither the keys nor the list)
  hipLaunchKernelGGL(pv_offsets_kernel, dim3(static_cast<unsigned>((static_cast<long long>(num_voxels) + kBlock) / kBlock)),
                     dim3(kBlock), 0, s, w.sortkey, list, n_cap, num_voxels, offsets);
  SPX_LAUNCH_CHECK();
  count(kPvGroups);
  return 0;
}

int spx_voxel_to_point(const void *vfeat, int num_voxels, const int32_t *rows, int n_cap, int C, int elem_bytes,
                       long long fill_bits, void *out, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8,
            "elem_bytes must be 1, 2, 4 or 8, got %d", elem_bytes);
  SPX_CHECK(C >= 1, "channel count must be >= 1, got %d", C);
  SPX_CHECK(n_cap >= 0 && num_voxels >= 0, "bad row counts %d / %d", n_cap, num_voxels);
  SPX_CHECK(static_cast<long long>(C) * elem_bytes <= 0x7fffffffLL, "row too long");
  if (n_cap == 0) return 0;
  SPX_CHECK(rows && out && (num_voxels == 0 || vfeat), "vfeat / rows / out is NULL");
  SPX_CHECK(aligned_to(vfeat, elem_bytes) && aligned_to(out, elem_bytes), "pointer not aligned to its elements");
  unsigned char fill16[16];
  for (int b = 0; b < 16; ++b) fill16[b] = static_cast<unsigned char>((static_cast<unsigned long long>(fill_bits) >> (8 * (b % elem_bytes))) & 0xffu);
  if (int rc = gather_rows(vfeat, num_voxels, rows, n_cap, C, elem_bytes, fill16, out, static_cast<hipStream_t>(stream))) return rc;
  count(kPvGather);
  return 0;
}

int spx_point_decorate(const float *points, int nfeat, int n_cap, const int32_t *rows, const int32_t *indices, int ndim,
                       const float *vsize, const float *coors_range, const float *cluster_mean, int flags, void *out,
                       int out_dtype, int C_out, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  SPX_CHECK(nfeat >= ndim, "points need at least %d columns, got %d", ndim, nfeat);
  SPX_CHECK(flags >= 0 && flags <= 3, "flags must be a combination of 1 (cluster offset) and 2 (centre offset), got %d", flags);
  SPX_CHECK(out_dtype == SPX_F32 || out_dtype == SPX_F16 || out_dtype == SPX_BF16,
            "out_dtype must be f32, f16 or bf16, got %d", out_dtype);
  const int need = nfeat + ndim * ((flags & 1) + ((flags >> 1) & 1));
  SPX_CHECK(C_out >= need, "C_out = %d is narrower than the decorated row (%d columns)", C_out, need);
  SPX_CHECK(n_cap >= 0, "bad point count %d", n_cap);
  SPX_CHECK(static_cast<long long>(C_out) * 4 <= 0x7fffffffLL, "row too long");
  if (n_cap == 0) return 0;
  SPX_CHECK(points && rows && out, "points / rows / out is NULL");
  SPX_CHECK(!(flags & 1) || cluster_mean, "the cluster offset needs cluster_mean");
  SPX_CHECK(!(flags & 2) || (indices && vsize && coors_range), "the centre offset needs indices, vsize and coors_range");
  const int eb = elem_bytes(out_dtype);
  SPX_CHECK(aligned_to(out, eb), "out not aligned to its elements");
  DecoGeom g;
  g.ndim = ndim;
  for (int j = 0; j < kMaxNdim; ++j) {              // the host arrays are zyx: point column j is axis ndim - 1 - j
    const bool in = j < ndim && (flags & 2);
    g.vsize[j] = in ? vsize[ndim - 1 - j] : 1.f;
    g.lo[j] = in ? coors_range[ndim - 1 - j] : 0.f;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = (static_cast<long long>(C_out) * eb) % 16 == 0 && aligned_to(out, 16);
  dispatch_row_of<SPX_F32, SPX_F16, SPX_BF16>(out_dtype, vec, [&](auto dt, auto v) {
    const int pieces = C_out / v;
    const long long total = static_cast<long long>(n_cap) * pieces;
    hipLaunchKernelGGL((pv_decorate_kernel<dt, v>), dim3(stream_blocks(total, kBlock)), dim3(kBlock), 0, s, points, nfeat,
                       total, pieces, rows, indices, g, cluster_mean, flags, out);
  });
  SPX_LAUNCH_CHECK();
  count(kPvDecorate);
  return 0;
}

}  // extern "C"
