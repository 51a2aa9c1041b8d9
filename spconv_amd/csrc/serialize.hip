// Voxel serialisation (spx_curve_keys, spx_serialize, spx_patch_plan, spx_patch_rows_bwd): the rows of a sparse level
// ordered along space-filling curves and cut into fixed-size patches, the step the serialised point / voxel
// transformers (Point Transformer V3, OctFormer, FlatFormer-style blocks) run between their SubM position encodings.
//
//   keys      per row and requested order the 64-bit key (batch << (ndim * depth)) | code: Z-order (bit interleave) or
//             Hilbert (Skilling's AxesToTranspose, then the interleave) over the row's spatial columns in the curve's
//             axis order; a dead row takes the key of all ones.  One launch, one thread per row, every order.
//   orders    per key row a stable LSD radix argsort over exactly the key bits in use (rowsort.hip: radix_argsort for
//             keys of at most 32 bits; radix_argsort64 beyond, every order in the same launches), the inverse
//             permutation, and the scenes' offsets by a bisection of the first order.
//   plan      scenes laid out on patch boundaries in P_cap = n / K + batch patches of K slots: a prefix over the
//             scenes by one workgroup, then one thread per slot.
//   rows_bwd  g_feat[r] = g[row_slot[r]] + g[row_slot2[r]]: one item per (row, piece), no atomics.
// Everything is an integer or a moved row, so a host loop reproduces every output bit for bit.
#include "common.h"
#include "piece.h"

namespace spx {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxOrders = 8;
constexpr int kMaxDepth = 16;

struct CurveSpec {
  int n_orders, depth, batch;
  unsigned char hilbert[kMaxOrders];            // 1: Hilbert, 0: Z-order
  unsigned char col[kMaxOrders][kMaxNdim];      // index column (1 + spatial axis) of X[j], the curve's axis order
};

// bit b of X[j] lands at bit b * ND + (ND - 1 - j): most significant bit first, X[0] ahead
template <int ND>
__device__ __forceinline__ unsigned long long interleave(const unsigned (&X)[ND], int depth) {
  unsigned long long code = 0;
  for (int b = 0; b < depth; ++b) {
#pragma unroll
    for (int j = 0; j < ND; ++j)
      code |= static_cast<unsigned long long>((X[j] >> b) & 1u) << (b * ND + (ND - 1 - j));
  }
  return code;
}

// Skilling, "Programming the Hilbert curve", AIP Conf. Proc. 707 (2004): AxesToTranspose, in place
template <int ND>
__device__ __forceinline__ void axes_to_transpose(unsigned (&X)[ND], int depth) {
  const unsigned M = 1u << (depth - 1);
  for (unsigned Q = M; Q > 1u; Q >>= 1) {       // inverse undo
    const unsigned P = Q - 1u;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      if (X[i] & Q) {
        X[0] ^= P;
      } else {
        const unsigned t = (X[0] ^ X[i]) & P;
        X[0] ^= t;
        X[i] ^= t;
      }
    }
  }
#pragma unroll
  for (int i = 1; i < ND; ++i) X[i] ^= X[i - 1];      // Gray encode
  unsigned t = 0;
  for (unsigned Q = M; Q > 1u; Q >>= 1)
    if (X[ND - 1] & Q) t ^= Q - 1u;
#pragma unroll
  for (int i = 0; i < ND; ++i) X[i] ^= t;
}

// One thread per row: its keys in every order.
template <int ND>
__global__ void __launch_bounds__(kBlock)
curve_keys_kernel(const int32_t *__restrict__ indices, int n, const int32_t *__restrict__ n_live, CurveSpec spec,
                  unsigned long long *__restrict__ keys /*[n_orders, n]*/) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int live = n_live ? min(*n_live, n) : n;
  int row[ND + 1];
  if constexpr (ND == 3) {
    const int4 v = reinterpret_cast<const int4 *>(indices)[i];
    row[0] = v.x, row[1] = v.y, row[2] = v.z, row[ND] = v.w;
  } else {
#pragma unroll
    for (int c = 0; c <= ND; ++c) row[c] = indices[static_cast<size_t>(i) * (ND + 1) + c];
  }
  bool ok = i < live && row[0] >= 0 && row[0] < spec.batch;
#pragma unroll
  for (int c = 1; c <= ND; ++c) ok = ok && static_cast<unsigned>(row[c]) < (1u << spec.depth);
  const unsigned long long head = static_cast<unsigned long long>(ok ? row[0] : 0) << (ND * spec.depth);
  for (int k = 0; k < spec.n_orders; ++k) {
    unsigned long long key = ~0ull;
    if (ok) {
      unsigned X[ND];
#pragma unroll
      for (int j = 0; j < ND; ++j) {            // (a select chain: the row stays in registers)
        const int col = spec.col[k][j];
        int v = row[1];
#pragma unroll
        for (int c = 2; c <= ND; ++c) v = col == c ? row[c] : v;
        X[j] = static_cast<unsigned>(v);
      }
      if (spec.hilbert[k]) axes_to_transpose<ND>(X, spec.depth);
      key = head | interleave<ND>(X, spec.depth);
    }
    keys[static_cast<size_t>(k) * n + i] = key;
  }
}

// keys of at most 32 bits in use: their low words, every order (the existing 32-bit sort reads them)
__global__ void __launch_bounds__(kBlock)
narrow_keys_kernel(const unsigned long long *__restrict__ keys, long long total, uint32_t mask,
                   uint32_t *__restrict__ keys32) {
  for (long long e = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; e < total;
       e += static_cast<long long>(gridDim.x) * kBlock)
    keys32[e] = static_cast<uint32_t>(keys[e]) & mask;
}

// inverse[k, order[k, t]] = t for every order (behind the 32-bit sort, whose last pass does not write it)
__global__ void __launch_bounds__(kBlock)
inverse_kernel(const int32_t *__restrict__ order, int n, long long total, int32_t *__restrict__ inverse) {
  for (long long e = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; e < total;
       e += static_cast<long long>(gridDim.x) * kBlock) {
    const long long k = e / n;
    const int t = static_cast<int>(e - k * n);
    const int r = order[e];
    if (static_cast<unsigned>(r) < static_cast<unsigned>(n)) inverse[k * n + r] = t;      // (checked, not trusted)
  }
}

// offsets[b] = the first position of the first order whose key is >= b << shift: live rows of a smaller batch index
__global__ void __launch_bounds__(kBlock)
scene_offsets_kernel(const unsigned long long *__restrict__ keys, const int32_t *__restrict__ order, int n, int batch,
                     int shift, int32_t *__restrict__ offsets) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b > batch) return;
  const unsigned long long bound = static_cast<unsigned long long>(b) << shift;
  unsigned lo = 0, hi = static_cast<unsigned>(n);
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    const unsigned r = static_cast<unsigned>(order[mid]);
    const unsigned long long key = r < static_cast<unsigned>(n) ? keys[r] : ~0ull;      // (checked, not trusted)
    if (key < bound) lo = mid + 1; else hi = mid;
  }
  offsets[b] = static_cast<int32_t>(lo);
}

// -------------------------------------------------------------------------------------------- patches

// rows [beg, beg + c) of scene b, read defensively: inside [0, n], never negative
__device__ __forceinline__ void scene_range(const int32_t *__restrict__ offsets, int b, int n, int &beg, int &c) {
  const int lo = min(max(offsets[b], 0), n), hi = min(max(offsets[b + 1], lo), n);
  beg = lo;
  c = hi - lo;
}

// pstart[b] = patches of the scenes before b (b = 0 .. batch), by ONE workgroup; n_patches = pstart[batch]
__global__ void __launch_bounds__(kBlock)
patch_prefix_kernel(const int32_t *__restrict__ offsets, int n, int batch, int K, int32_t *__restrict__ pstart,
                    int32_t *__restrict__ n_patches) {
  __shared__ int lds_wave[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < batch; base += kBlock) {
    const int b = base + threadIdx.x;
    int v = 0;
    if (b < batch) {
      int beg, c;
      scene_range(offsets, b, n, beg, c);
      v = c / K + (c % K != 0);
    }
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    __syncthreads();                            // (lds_wave of the previous round has been read)
    if (lane == 63) lds_wave[wave] = incl;
    __syncthreads();
    int prefix = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      const int s = lds_wave[w];
      if (w < wave) prefix += s;
      total += s;
    }
    if (b < batch) pstart[b] = carry + prefix + incl - v;
    carry += total;
  }
  if (threadIdx.x == 0) {
    pstart[batch] = carry;
    *n_patches = carry;
  }
}

// the scene whose interval [start[b], start[b + 1]) holds x (start ascending, empty intervals skipped); x < start[batch]
__device__ __forceinline__ int scene_of(const int32_t *__restrict__ start, int batch, int x) {
  int lo = 0, hi = batch - 1;                   // the first b with start[b + 1] > x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (start[mid + 1] > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// One thread per slot s = patch * K + j: the slot's row (patch_rows, patch_rows_canon, patch_scene); the thread also
// takes the SORTED POSITION t = s while s < n: the canonical and the borrowed slot of row order[t] (row_slot,
// row_slot2).  Every output element is written exactly once.
__global__ void __launch_bounds__(kBlock)
patch_slots_kernel(const int32_t *__restrict__ order, const int32_t *__restrict__ offsets,
                   const int32_t *__restrict__ pstart, int n, int batch, int K, int borrow, long long slots,
                   int32_t *__restrict__ patch_rows, int32_t *__restrict__ patch_rows_canon,
                   int32_t *__restrict__ row_slot, int32_t *__restrict__ row_slot2, int32_t *__restrict__ patch_scene) {
  const int used = min(max(pstart[batch], 0), static_cast<int>(slots / K));
  for (long long s = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; s < slots;
       s += static_cast<long long>(gridDim.x) * kBlock) {
    const int p = static_cast<int>(s / K), j = static_cast<int>(s - static_cast<long long>(p) * K);
    int row = -1, canon = -1, scene = -1;
    if (p < used) {
      scene = scene_of(pstart, batch, p);
      int beg, c;
      scene_range(offsets, scene, n, beg, c);
      const long long q = static_cast<long long>(p - pstart[scene]) * K + j;
      if (q >= 0 && q < c) {
        row = canon = order[beg + q];
      } else if (borrow && c >= K && q >= K && q - K < c) {
        row = order[beg + q - K];
      }
      if (static_cast<unsigned>(row) >= static_cast<unsigned>(n)) row = canon = -1;      // (checked, not trusted)
    }
    patch_rows[s] = row;
    patch_rows_canon[s] = canon;
    if (j == 0) patch_scene[p] = scene;
    if (s < n) {
      const int t = static_cast<int>(s);
      const int r = order[t];
      if (static_cast<unsigned>(r) >= static_cast<unsigned>(n)) continue;
      const int live = min(max(offsets[batch], 0), n);
      long long s1 = -1, s2 = -1;
      if (t < live) {
        const int b = scene_of(offsets, batch, t);
        int beg, c;
        scene_range(offsets, b, n, beg, c);
        const int q = t - beg;
        if (q >= 0 && q < c) {
          s1 = static_cast<long long>(pstart[b]) * K + q;
          const long long room = static_cast<long long>(c / K + (c % K != 0)) * K;
          if (borrow && c >= K && q + K >= c && q + K < room) s2 = s1 + K;
          if (s1 >= slots) s1 = -1;
          if (s2 >= slots) s2 = -1;
        }
      }
      row_slot[r] = static_cast<int32_t>(s1);
      row_slot2[r] = static_cast<int32_t>(s2);
    }
  }
}

// -------------------------------------------------------------------------------------------- rows_bwd

// One item per (row, piece): the canonical slot's piece, plus the borrowed slot's when the row has one.
template <int DT, int V>
__global__ void __launch_bounds__(kBlock)
patch_rows_bwd_kernel(const void *__restrict__ g_, int slots, const int32_t *__restrict__ row_slot,
                      const int32_t *__restrict__ row_slot2, long long total, int pieces, void *__restrict__ out_) {
  using E = Elem<DT>;
  using S = typename E::S;
  using A = typename E::A;
  using P = Piece<S, V>;
  const P *g = static_cast<const P *>(g_);
  P *out = static_cast<P *>(out_);
  for (long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * kBlock) {
    const long long r = total <= 0x7fffffffLL
                            ? static_cast<long long>(static_cast<unsigned>(item) / static_cast<unsigned>(pieces))
                            : item / pieces;
    const int p = static_cast<int>(item - r * pieces);
    int s1 = row_slot[r], s2 = row_slot2[r];
    if (static_cast<unsigned>(s1) >= static_cast<unsigned>(slots)) s1 = -1;      // (checked, not trusted)
    if (static_cast<unsigned>(s2) >= static_cast<unsigned>(slots)) s2 = -1;
    P a, b, o;
    if (s1 >= 0) a = g[static_cast<long long>(s1) * pieces + p];
    if (s2 >= 0) b = g[static_cast<long long>(s2) * pieces + p];
    if (s1 >= 0 && s2 >= 0) {
#pragma unroll
      for (int j = 0; j < V; ++j) o.e[j] = E::down(E::up(a.e[j]) + E::up(b.e[j]));
    } else if (s1 >= 0) {
      o = a;                                    // (one term: the row keeps its bits)
    } else if (s2 >= 0) {
      o = b;
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) o.e[j] = E::down(A(0));
    }
    out[item] = o;
  }
}

int bit_length(unsigned v) {
  int b = 0;
  while (v) {
    ++b;
    v >>= 1;
  }
  return b;
}

// 0 = ok: the checks of a key geometry that need no pointer
int check_curve(int n, int ndim, int batch, int depth, int n_orders) {
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  SPX_CHECK(depth >= 1 && depth <= kMaxDepth, "depth must be in [1,16], got %d", depth);
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  SPX_CHECK(n_orders >= 1 && n_orders <= kMaxOrders, "1 to 8 orders per call, got %d", n_orders);
  SPX_CHECK(n >= 0, "bad row count %d", n);
  SPX_CHECK(ndim * depth + bit_length(static_cast<unsigned>(batch)) <= 63,
            "key of %d x %d curve bits and %d batch bits exceeds 63 bits", ndim, depth,
            bit_length(static_cast<unsigned>(batch)));
  return 0;
}

// whether (key_bits, batch_shift, batch) describe keys whose dead value sorts behind every live one
bool sort_geometry_ok(int n, int n_orders, int key_bits, int batch_shift, int batch) {
  return n >= 0 && n_orders >= 1 && n_orders <= kMaxOrders && key_bits >= 1 && key_bits <= 63 && batch >= 1 &&
         batch_shift >= 0 && batch_shift < key_bits && bit_length(static_cast<unsigned>(batch)) <= key_bits - batch_shift;
}

// scratch of an orders call: the narrowed keys of every order (keys of at most 32 bits), the sort's buffers
struct SerializeWs {
  uint32_t *keys32;
  void *sort;
  size_t bytes;
  SerializeWs(void *ws, int n, int n_orders, int key_bits) {
    Carver c(ws);
    const size_t nn = n > 0 ? n : 1;
    keys32 = nullptr;
    if (key_bits <= 32) {
      keys32 = c.take<uint32_t>(nn * n_orders);
      sort = c.take<char>(radix_argsort_ws_bytes(n));
    } else {
      sort = c.take<char>(radix_argsort64_ws_bytes(n, n_orders));
    }
    bytes = c.off;
  }
};

bool plan_geometry_ok(int n, int batch, int patch_size) {
  if (n < 0 || batch < 1 || patch_size < 1) return false;
  return (static_cast<long long>(n / patch_size) + batch) * patch_size < 0x80000000LL;
}

}  // namespace
}  // namespace spx

extern "C" {

int spx_curve_keys(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, int depth, int n_orders,
                   const int *orders_h, const int *axes_h, uint64_t *keys, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_curve(n, ndim, batch, depth, n_orders)) return rc;
  SPX_CHECK(orders_h && axes_h, "orders / axes is NULL");
  CurveSpec spec = {};
  spec.n_orders = n_orders;
  spec.depth = depth;
  spec.batch = batch;
  unsigned seen = 0;
  for (int j = 0; j < ndim; ++j) {
    SPX_CHECK(axes_h[j] >= 0 && axes_h[j] < ndim && !(seen & (1u << axes_h[j])),
              "axes must be a permutation of 0 .. %d", ndim - 1);
    seen |= 1u << axes_h[j];
  }
  for (int k = 0; k < n_orders; ++k) {
    const int o = orders_h[k];
    SPX_CHECK(o == SPX_ORDER_Z || o == SPX_ORDER_Z_TRANS || o == SPX_ORDER_HILBERT || o == SPX_ORDER_HILBERT_TRANS,
              "unknown order code %d", o);
    spec.hilbert[k] = (o == SPX_ORDER_HILBERT || o == SPX_ORDER_HILBERT_TRANS) ? 1 : 0;
    const bool trans = (o == SPX_ORDER_Z_TRANS || o == SPX_ORDER_HILBERT_TRANS) && ndim >= 2;
    for (int j = 0; j < ndim; ++j) {
      const int src = trans && j < 2 ? 1 - j : j;
      spec.col[k][j] = static_cast<unsigned char>(1 + axes_h[src]);
    }
  }
  if (n == 0) return 0;
  SPX_CHECK(indices && keys, "indices / keys is NULL");
  SPX_CHECK(aligned_to(indices, ndim == 3 ? 16 : 4) && aligned_to(keys, 8), "indices / keys not aligned");
  dispatch_value<1, 2, 3, 4>(ndim, [&](auto nd) {
    hipLaunchKernelGGL(curve_keys_kernel<nd>, dim3(div_up(n, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       indices, n, n_live, spec, reinterpret_cast<unsigned long long *>(keys));
  });
  SPX_LAUNCH_CHECK();
  count(kSerKeys);
  return 0;
}

size_t spx_serialize_ws_bytes(int n, int n_orders, int key_bits) {
  if (!spx::sort_geometry_ok(n, n_orders, key_bits, 0, 1)) return 0;
  return spx::SerializeWs(nullptr, n, n_orders, key_bits).bytes;
}

int spx_serialize(const uint64_t *keys, int n, int n_orders, int key_bits, int batch, int batch_shift, int32_t *order,
                  int32_t *inverse, int32_t *offsets, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(sort_geometry_ok(n, n_orders, key_bits, batch_shift, batch),
            "bad sort geometry: n %d, orders %d, key bits %d, batch %d at bit %d", n, n_orders, key_bits, batch,
            batch_shift);
  SPX_CHECK(offsets && (n == 0 || (keys && order && inverse)), "keys / order / inverse / offsets is NULL");
  SerializeWs w(ws, n, n_orders, key_bits);
  SPX_CHECK(n == 0 || (ws && ws_bytes >= w.bytes), "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned long long *k64 = reinterpret_cast<const unsigned long long *>(keys);
  if (n > 0 && key_bits <= 32) {                // the 32-bit sort, order by order, between a narrowing and an inverse launch
    const long long total = static_cast<long long>(n) * n_orders;
    const dim3 grid(stream_blocks(total, kBlock));
    const uint32_t mask = key_bits == 32 ? 0xffffffffu : (1u << key_bits) - 1u;
    hipLaunchKernelGGL(narrow_keys_kernel, grid, dim3(kBlock), 0, s, k64, total, mask, w.keys32);
    SPX_LAUNCH_CHECK();
    for (int k = 0; k < n_orders; ++k) {
      const size_t at = static_cast<size_t>(k) * n;
      if (int rc = radix_argsort(w.keys32 + at, n, key_bits, order + at, w.sort, s)) return rc;
    }
    hipLaunchKernelGGL(inverse_kernel, grid, dim3(kBlock), 0, s, order, n, total, inverse);
    SPX_LAUNCH_CHECK();
  } else if (n > 0) {                           // every order pass by pass together: three launches per digit
    if (int rc = radix_argsort64(keys, n, n_orders, key_bits, order, inverse, w.sort, s)) return rc;
  }
  if (n > 0)
    for (int k = 0; k < n_orders; ++k) count(kSerSort);
  // (n = 0: the bisection touches neither the keys nor the order)
  hipLaunchKernelGGL(scene_offsets_kernel, dim3(div_up(batch + 1, kBlock)), dim3(kBlock), 0, s, k64, order, n, batch,
                     batch_shift, offsets);
  SPX_LAUNCH_CHECK();
  count(kSerOffsets);
  return 0;
}

size_t spx_patch_plan_ws_bytes(int n, int batch, int patch_size) {
  if (!spx::plan_geometry_ok(n, batch, patch_size)) return 0;
  return spx::align_up((static_cast<size_t>(batch) + 1) * sizeof(int32_t), 256);
}

int spx_patch_plan(const int32_t *order, const int32_t *offsets, int n, int batch, int patch_size, int pad,
                   int32_t *patch_rows, int32_t *patch_rows_canon, int32_t *row_slot, int32_t *row_slot2,
                   int32_t *patch_scene, int32_t *n_patches_dev, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(patch_size >= 1, "patch_size must be >= 1, got %d", patch_size);
  SPX_CHECK(n >= 0 && batch >= 1, "bad row count / batch %d / %d", n, batch);
  SPX_CHECK(plan_geometry_ok(n, batch, patch_size), "(n / patch_size + batch) * patch_size must stay below 2^31");
  SPX_CHECK(pad == SPX_PAD_MASK || pad == SPX_PAD_BORROW, "pad must be 0 (mask) or 1 (borrow), got %d", pad);
  SPX_CHECK(offsets && patch_rows && patch_rows_canon && patch_scene && n_patches_dev &&
                (n == 0 || (order && row_slot && row_slot2)), "null pointer");
  SPX_CHECK(ws && ws_bytes >= spx_patch_plan_ws_bytes(n, batch, patch_size), "workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t *pstart = static_cast<int32_t *>(ws);
  const long long slots = (static_cast<long long>(n / patch_size) + batch) * patch_size;
  hipLaunchKernelGGL(patch_prefix_kernel, dim3(1), dim3(kBlock), 0, s, offsets, n, batch, patch_size, pstart,
                     n_patches_dev);
  hipLaunchKernelGGL(patch_slots_kernel, dim3(stream_blocks(slots, kBlock)), dim3(kBlock), 0, s, order, offsets, pstart, n,
                     batch, patch_size, pad == SPX_PAD_BORROW ? 1 : 0, slots, patch_rows, patch_rows_canon, row_slot,
                     row_slot2, patch_scene);
  SPX_LAUNCH_CHECK();
  count(kSerPlan);
  return 0;
}

int spx_patch_rows_bwd(const void *g, int slots, const int32_t *row_slot, const int32_t *row_slot2, int n, int C,
                       int dtype, void *g_feat, spx_stream_t stream) {
  using namespace spx;
  const int eb = float_row_elem(dtype, C);
  if (eb < 0) return eb;
  SPX_CHECK(n >= 0 && slots >= 0, "bad row / slot counts %d / %d", n, slots);
  if (n == 0) return 0;
  SPX_CHECK(row_slot && row_slot2 && g_feat && (slots == 0 || g), "g / row_slot / row_slot2 / g_feat is NULL");
  SPX_CHECK(aligned_to(g, eb) && aligned_to(g_feat, eb), "pointer not aligned to its elements");
  const bool vec = (static_cast<long long>(C) * eb) % 16 == 0 && aligned_to(g, 16) && aligned_to(g_feat, 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_row(dtype, vec, [&](auto dt, auto v) {
    const int pieces = C / v;
    const long long total = static_cast<long long>(n) * pieces;
    hipLaunchKernelGGL((patch_rows_bwd_kernel<dt, v>), dim3(stream_blocks(total, kBlock)), dim3(kBlock), 0, s, g, slots,
                       row_slot, row_slot2, total, pieces, g_feat);
  });
  SPX_LAUNCH_CHECK();
  count(kSerBwd);
  return 0;
}

}  // extern "C"
