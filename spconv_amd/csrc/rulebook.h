// What the rulebook ("indice pair") builders share: rulebook_subm.hip (SubM over the hash table and over a rank map),
// rulebook_conv.hip (first-seen convolution), rulebook_sorted.hip (convolution numbered by key rank) and
// rulebook_lists.hip (conversions between the table and the Native-list form).  Here: the problem and output
// descriptors the convolution entry points fill once, the geometry checks, the candidate iterator of the compact passes,
// and the kernels more than one unit launches (Native-list compaction, masks from a finished table).  Every definition
// has internal linkage -- each including unit gets its own copy of a kernel, as with scan.h, fill.h and rankmap.h.
//
// Design (MI355X-first, not a translation of the reference kernels):
//  * one open-addressing hash table in global memory (table.h);
//  * NO order-dependent atomics anywhere: duplicate keys are resolved with atomicMin (smallest index wins == the CPU
//    path's unordered_map::insert), the dense tables are written by the thread that owns the row (coalesced along the
//    voxel axis), and every compaction / numbering step is a count -> scan -> scatter pipeline built on wave64 ballot +
//    mbcnt prefix sums.  The result is therefore bit-identical to the reference CPU loops
//    (csrc/sparse/indices.py:1639-1778), including list order and the first-seen numbering of regular-conv outputs;
//  * kernel boundaries are the only inter-workgroup synchronisation (XCD L2s are not coherent inside a launch).
#pragma once
#include "common.h"
#include "fill.h"
#include "scan.h"
#include "table.h"

namespace spx {
namespace {

constexpr int kBlock = 256;
constexpr int kItems = 2048;  // entries per block in count/scatter passes (8 x 256)
static_assert(kBlock == kScanThreads, "scan.h's primitives are written for the builders' workgroup size");

// A convolution problem as the C entry points receive it (the int arrays have ndim entries; dilation may be null).
struct ConvProblem {
  const int32_t *indices;
  int n_in, ndim, batch_size;
  const int *in_shape, *out_shape, *ksize, *stride, *padding, *dilation;
  int transposed;
};

// The tables a build writes.  n_out: output rows (the count of the two-call form, the bound of the static-shape form).
struct ConvOutputs {
  int n_out;
  int32_t *out_indices, *pair_fwd, *pair_bwd;
  uint32_t *mask_fwd, *mask_bwd;
  int32_t *pair_native, *num_per_loc;
};

int check_geom(int ndim, int n, int kv) {
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  SPX_CHECK(n >= 0, "negative voxel count %d", n);
  SPX_CHECK(kv >= 1 && static_cast<long long>(kv) * n < 2147483647LL,
            "kernel volume %d x %d voxels overflows int32 positions", kv, n);
  return 0;
}

// The checks every pass of a convolution build starts with; g: the problem in canonical 4-d form.
int conv_geom(const ConvProblem &p, Geom &g) {
  SPX_CHECK(p.ndim >= 1 && p.ndim <= kMaxNdim, "ndim must be in [1,4], got %d", p.ndim);
  g = make_geom(p.ndim, p.batch_size, p.in_shape, p.out_shape, p.ksize, p.stride, p.padding, p.dilation);
  if (check_geom(p.ndim, p.n_in, g.kv)) return -1;
  for (int i = 0; i < p.ndim; ++i)
    SPX_CHECK(p.out_shape[i] > 0 && p.stride[i] > 0, "bad output shape / stride at dim %d", i);
  return 0;
}

// Two-call forms: {outputs found, overflow flag} of a count pass, read back (synchronises the stream).
int read_count(const int32_t *d_nout, hipStream_t s, int *n_out_h, int *overflow_h = nullptr) {
  int32_t host_n[2] = {0, 0};
  SPX_HIP(hipMemcpyAsync(host_n, d_nout, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  SPX_HIP(hipStreamSynchronize(s));
  *n_out_h = host_n[0];
  if (overflow_h) *overflow_h = host_n[1];
  return 0;
}

// Static-shape entry points (first-seen and sorted): their argument checks, and the -1 fills of the outputs -- both
// sizes are known up front, so the fills ride in the first pass's fill launch (`pre`).
int static_prologue(const ConvProblem &p, const ConvOutputs &o, const int32_t *n_out_dev, FillList &pre) {
  SPX_CHECK(o.n_out > 0 && n_out_dev && o.out_indices, "n_out_cap > 0, n_out_dev and out_indices are required");
  SPX_CHECK(p.n_in > 0, "static-shape rulebook needs n_in > 0 (pad the input with batch = -1 rows)");
  SPX_CHECK(o.pair_fwd && o.pair_bwd, "pair_fwd and pair_bwd are required");
  int kv = 1;
  for (int i = 0; i < p.ndim; ++i) kv *= p.ksize[i];
  pre.add(o.out_indices, sizeof(int32_t) * static_cast<size_t>(o.n_out) * (p.ndim + 1), 0xFFFFFFFFu);
  pre.add(o.pair_fwd, sizeof(int32_t) * static_cast<size_t>(kv) * o.n_out, 0xFFFFFFFFu);
  return 0;
}

// ------------------------------------------- Native-list compaction (a4/a5)

// mode 0 (SubM): list k in [0, kv/2) is the set {(in=e, out=row[e])} with
//   row = pair_fwd[kv-1-k] (== pair_bwd[k]); the mirror list kv-1-k gets the
//   roles swapped (indices.py:1692-1696).
// mode 1 (conv): list k in [0, kv) from row = pair_bwd[k] (indices.py:1767-1768).
__device__ __forceinline__ const int32_t *list_row(const int32_t *table, int mode, int list,
                                                    int kv, int n) {
  const int row = mode == 0 ? kv - 1 - list : list;
  return table + static_cast<size_t>(row) * n;
}

__global__ void __launch_bounds__(kBlock)
compact_count_kernel(const int32_t *__restrict__ table, int mode, int kv, int n, int nblk,
                     int32_t *__restrict__ blockcount) {
  __shared__ int lds_wave[kBlock / 64];
  const int list = blockIdx.y, blk = blockIdx.x;
  const int32_t *row = list_row(table, mode, list, kv, n);
  const int begin = blk * kItems;
  int cnt = 0;
#pragma unroll
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    const bool pred = e < n && row[e] >= 0;
    cnt += __popcll(__ballot(pred));
  }
  if ((threadIdx.x & 63) == 0) lds_wave[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kBlock / 64; ++w) s += lds_wave[w];
    blockcount[static_cast<size_t>(list) * nblk + blk] = s;
  }
}

__global__ void __launch_bounds__(kBlock)
compact_scatter_kernel(const int32_t *__restrict__ table, int mode, int kv, int n, int nblk,
                       const int32_t *__restrict__ blockoff, int32_t *__restrict__ native) {
  __shared__ int lds_wave[kBlock / 64];
  const int list = blockIdx.y, blk = blockIdx.x;
  const int32_t *row = list_row(table, mode, list, kv, n);
  const int begin = blk * kItems;
  int running = blockoff[static_cast<size_t>(list) * nblk + blk];
  const size_t plane = static_cast<size_t>(kv) * n;  // native[1] offset
  int32_t *in_k = native + static_cast<size_t>(list) * n;
  int32_t *out_k = native + plane + static_cast<size_t>(list) * n;
  int32_t *in_m = native + static_cast<size_t>(kv - 1 - list) * n;
  int32_t *out_m = native + plane + static_cast<size_t>(kv - 1 - list) * n;
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    const int v = e < n ? row[e] : -1;
    int total;
    const int rank = block_rank(v >= 0, total, lds_wave);
    if (v >= 0) {
      const int j = running + rank;
      in_k[j] = e;
      out_k[j] = v;
      if (mode == 0) {
        in_m[j] = v;
        out_m[j] = e;
      }
    }
    running += total;
  }
}

// ConvAlgo.Native lists of a SubM rulebook from the finished table, in the CPU loop's order
// (ascending input row inside a list, indices.py:1685-1696): blockIdx.y = list L < kv/2 (and its
// mirror kv-1-L with the roles swapped), or kv/2 = the identity list.  The block's output offset
// is the sum of the 256-voxel hit counts the probe kernel left (no separate scan launch); block 0
// of a list also writes num_per_loc[L].  Positions past a list's length are set to -1 here
// (ops.py:191-193 starts from a -1 filled tensor), so the caller's buffer needs no pre-fill.
__global__ void __launch_bounds__(kBlock)
subm_lists_kernel(const int32_t *__restrict__ pair_fwd, int kv, int n, int nblk256,
                  const int32_t *__restrict__ blockcount, int32_t *__restrict__ native,
                  int32_t *__restrict__ num_per_loc, int num_len, int conv = 0) {
  // conv != 0: regular / transposed convolution -- `pair_fwd` is then pair_bwd [kv, n_in], list k is
  // read off its row k (indices.py:1767-1768), there is no mirror list and no identity list
  __shared__ int lds_wave[kBlock / 64];
  __shared__ int lds_red[2][kBlock / 64];
  const int list = blockIdx.y, blk = blockIdx.x;
  const int begin = blk * kItems;
  const size_t plane = static_cast<size_t>(kv) * n;
  if (!conv && list == kv / 2) {               // identity lists (indices.py:1678-1682)
    // counts exist for k < kv/2 only (indices.py:1685,1692); the rest of num_per_loc reads 0
    if (blk == 0)
      for (int i = kv / 2 + threadIdx.x; i < num_len; i += kBlock) num_per_loc[i] = 0;
    if (!native) return;
    for (int it = 0; it < kItems / kBlock; ++it) {
      const int e = begin + it * kBlock + threadIdx.x;
      if (e < n) {
        native[static_cast<size_t>(list) * n + e] = e;
        native[plane + static_cast<size_t>(list) * n + e] = e;
      }
    }
    return;
  }
  // the block's table entries are requested first, ahead of the count prefix (two independent latencies)
  const int32_t *row = pair_fwd + static_cast<size_t>(conv ? list : kv - 1 - list) * n;
  int vals[kItems / kBlock];
#pragma unroll
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    vals[it] = (native && e < n) ? row[e] : -1;
  }
  // prefix of the hit counts before this block's first 256-voxel group, and the list total
  const int32_t *cnt = blockcount + static_cast<size_t>(list) * nblk256;
  const int first_group = blk * (kItems / kBlock);
  int before = 0, all = 0;
  for (int i = threadIdx.x; i < nblk256; i += kBlock) {
    const int v = cnt[i];
    all += v;
    if (i < first_group) before += v;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    before += __shfl_xor(before, d, 64);
    all += __shfl_xor(all, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    lds_red[0][threadIdx.x >> 6] = before;
    lds_red[1][threadIdx.x >> 6] = all;
  }
  __syncthreads();
  before = all = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) {
    before += lds_red[0][w];
    all += lds_red[1][w];
  }
  if (blk == 0 && threadIdx.x == 0 && num_per_loc) num_per_loc[list] = all;
  if (!native) return;
  int32_t *in_k = native + static_cast<size_t>(list) * n;
  int32_t *out_k = native + plane + static_cast<size_t>(list) * n;
  int32_t *in_m = native + static_cast<size_t>(kv - 1 - list) * n;
  int32_t *out_m = native + plane + static_cast<size_t>(kv - 1 - list) * n;
  int running = before;
#pragma unroll
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    const int v = vals[it];
    int total;
    const int rank = block_rank(v >= 0, total, lds_wave);
    if (v >= 0) {
      const int j = running + rank;
      in_k[j] = e;
      out_k[j] = v;
      if (!conv) {
        in_m[j] = v;
        out_m[j] = e;
      }
    }
    running += total;
    if (e < n && e >= all) {                   // tail of the list: this block's own position range
      in_k[e] = -1;
      out_k[e] = -1;
      if (!conv) {
        in_m[e] = -1;
        out_m[e] = -1;
      }
    }
  }
}

// mask[row][w] bit k = (table[k][row] >= 0)  (indices.py:652-676)
__global__ void __launch_bounds__(kBlock)
mask_from_table_kernel(const int32_t *__restrict__ table, int kv, int n, int words,
                       uint32_t *__restrict__ mask) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t mcur = 0;
  for (int k = 0; k < kv; ++k) {
    if (table[static_cast<size_t>(k) * n + i] >= 0) mcur |= 1u << (k & 31);
    if ((k & 31) == 31 || k == kv - 1) {
      mask[static_cast<size_t>(i) * words + (k >> 5)] = mcur;
      mcur = 0;
    }
  }
}

// Both masks of a regular-conv rulebook in one launch: rows [0, n_a) of table a, then rows of b.
__global__ void __launch_bounds__(kBlock)
mask_from_tables_kernel(const int32_t *__restrict__ ta, int n_a, uint32_t *__restrict__ ma,
                        const int32_t *__restrict__ tb, int n_b, uint32_t *__restrict__ mb,
                        int kv, int words) {
  int i = blockIdx.x * kBlock + threadIdx.x;
  const int32_t *table = ta;
  uint32_t *mask = ma;
  int n = n_a;
  if (i >= n_a) {
    i -= n_a;
    table = tb;
    mask = mb;
    n = n_b;
  }
  if (i >= n) return;
  uint32_t mcur = 0;
  for (int k = 0; k < kv; ++k) {
    if (table[static_cast<size_t>(k) * n + i] >= 0) mcur |= 1u << (k & 31);
    if ((k & 31) == 31 || k == kv - 1) {
      mask[static_cast<size_t>(i) * words + (k >> 5)] = mcur;
      mcur = 0;
    }
  }
}

// ------------------------------------------ compact candidates of a strided convolution (rulebook_conv.hip)
constexpr int kMaxCand = 8;       // candidates per input the compact passes are instantiated for
constexpr int kMaxKv3 = 64;       // offsets (bit-map rows held in LDS)

struct CandIter {
  uint32_t vm[4], v[4];
  bool live;
  // valid offsets per axis of input coordinate c (regular conv): bit r of vm[d]
  __device__ __forceinline__ void init(const Geom &g, const int (&c)[4], bool row_ok) {
    live = row_ok;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const float inv = 1.0f / static_cast<float>(g.stride[d]);
      uint32_t m = 0;
      for (int r = 0; r < g.ksize[d]; ++r) {
        const int h = c[d] + g.padding[d] - r * g.dilation[d];
        const int q = __float2int_rn(static_cast<float>(h) * inv);
        if (q * g.stride[d] == h && q >= 0 && q < g.out_dims[d]) m |= 1u << r;
      }
      vm[d] = v[d] = m;
      live = live && m != 0;
    }
  }
  // current candidate: offset index k and output coordinate q
  __device__ __forceinline__ int offset(const Geom &g, const int (&c)[4], int (&q)[4]) const {
    int k = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int r = __builtin_ctz(v[d]);
      k = k * g.ksize[d] + r;
      const int h = c[d] + g.padding[d] - r * g.dilation[d];
      q[d] = __float2int_rn(static_cast<float>(h) * (1.0f / static_cast<float>(g.stride[d])));
    }
    return k;
  }
  __device__ __forceinline__ int offset(const Geom &g) const {
    int k = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) k = k * g.ksize[d] + __builtin_ctz(v[d]);
    return k;
  }
  __device__ __forceinline__ void next() {     // odometer over the bit sets, last axis fastest
#pragma unroll
    for (int d = 3; d >= 0; --d) {
      v[d] &= v[d] - 1;
      if (v[d]) return;
      v[d] = vm[d];
    }
    live = false;
  }
};

int gcd_int(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a < 0 ? -a : a;
}

size_t conv_max_out(int n_in, int ndim, const int *ksize, const int *stride, const int *dilation,
                    int transposed) {
  // Upper bound of distinct outputs.  The reference's SpconvOps.get_handcrafted_max_act_out
  // (all.py:1557-1578) uses N * prod(ceil(k/s)), which ignores dilation: along one axis an input
  // reaches the outputs o with o*s = c + p - r*d, and r*d mod s repeats with period s / gcd(d, s),
  // so up to ceil(k * gcd(d, s) / s) offsets r hit a multiple of s (k = 3, s = 2, d = 2: all 3,
  // not 2).  Transposed: kv * N (ops.py:569-570).
  size_t kv = 1, m = 1;
  for (int i = 0; i < ndim; ++i) {
    kv *= ksize[i];
    const int g = gcd_int(dilation ? dilation[i] : 1, stride[i]);
    size_t per = (static_cast<size_t>(ksize[i]) * g + stride[i] - 1) / stride[i];
    if (per > static_cast<size_t>(ksize[i])) per = ksize[i];
    m *= per;
  }
  if (transposed || m > kv) m = kv;
  return m * static_cast<size_t>(n_in);
}

// Candidates per input the compact passes (conv3_*, conv4_*) run with -- 1, 2, 4 or 8 -- or 0 when the
// problem takes the thread-per-(offset, input) passes: transposed convolution, stride 1 (every offset
// is a candidate), more than 8 candidates, kv > 64, coordinates beyond the float-exact range.
int conv3_cands(const ConvProblem &p) {
  if (option_int("SPX_CONV_V", 3) < 3 || p.transposed) return 0;     // (2: the generic passes, for A/B runs)
  int kv = 1;
  for (int i = 0; i < p.ndim; ++i) {
    kv *= p.ksize[i];
    const long long reach = static_cast<long long>(p.ksize[i]) * (p.dilation ? p.dilation[i] : 1);
    if (p.ksize[i] > 32 || p.in_shape[i] + static_cast<long long>(p.padding[i]) >= (1 << 21) || reach >= (1 << 21))
      return 0;
  }
  const size_t m = conv_max_out(1, p.ndim, p.ksize, p.stride, p.dilation, 0);
  if (kv > kMaxKv3 || m > kMaxCand || 2 * m > static_cast<size_t>(kv)) return 0;
  return m <= 1 ? 1 : (m <= 2 ? 2 : (m <= 4 ? 4 : 8));
}

// Shares per input row of the compact passes that are bound by dependent memory round trips (grid.y): a
// power of two <= the candidate count, enough for ~1.5 M threads.
int conv3_shares(int n_in, int mj) {
  // tests only (spx_set_option): 1, 2 or 4 shares whatever the size, at most mj (0 = by size) -- a share count below
  // mj otherwise takes 187 500 inputs and more
  const int forced = option_int("SPX_TEST_CONV3_SHARES", 0);
  if (forced == 1 || forced == 2 || forced == 4) return forced < mj ? forced : mj;
  int s = 1;
  while (s < mj && static_cast<long long>(n_in) * s < 1500000) s <<= 1;
  return s;
}

#define SPX_CONV3_LAUNCH(kernel, mj, ...)                                     \
  do {                                                                        \
    if ((mj) == 1) hipLaunchKernelGGL(kernel<1>, __VA_ARGS__);                \
    else if ((mj) == 2) hipLaunchKernelGGL(kernel<2>, __VA_ARGS__);           \
    else if ((mj) == 4) hipLaunchKernelGGL(kernel<4>, __VA_ARGS__);           \
    else hipLaunchKernelGGL(kernel<8>, __VA_ARGS__);                          \
  } while (0)

// Launches the count -> scan -> scatter compaction that builds the Native lists (native null: their lengths only).
int launch_native_lists(const int32_t *table, int mode, int kv, int n, int nlists, int nblk, int32_t *blockcount,
                        int32_t *blockoff, int32_t *native, int32_t *num_per_loc, hipStream_t s) {
  if (n == 0 || nlists == 0) return 0;
  dim3 grid(nblk, nlists);
  hipLaunchKernelGGL(compact_count_kernel, grid, dim3(kBlock), 0, s, table, mode, kv, n, nblk, blockcount);
  hipLaunchKernelGGL(scan_kernel, dim3(nlists), dim3(kBlock), 0, s, blockcount, blockoff, nblk, num_per_loc);
  if (native)
    hipLaunchKernelGGL(compact_scatter_kernel, grid, dim3(kBlock), 0, s, table, mode, kv, n, nblk, blockoff, native);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace spx
