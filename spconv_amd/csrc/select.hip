// Voxel pruning: row scores, top-k flags and the stable compaction of the selected rows (spx_row_score,
// spx_topk_flags, spx_select_count / _fill / _static).  The pruned down-sampling blocks of SPS-Conv and VoxelNeXt and
// every sparse head that keeps its top-scoring voxels; include/spconv_amd.h (voxel pruning) holds the contract.
//
//   score   a row belongs to a group of G lanes (G = a power of two covering the row's pieces, at most a wave); lane s
//           adds |x| over the pieces s, s + G, ... in order, the lanes' sums meet in a butterfly whose lane 0 adds
//           acc[s] + acc[s + d] for d = G / 2 .. 1: an order that depends on C and the dtype only.  One launch.
//           absmax takes the larger of the two at every step, and a NaN from either side: a row with a NaN element
//           scores a positive NaN under both ops.
//   top-k   radix select on the order-preserving key of the fp32 score, 8 bits per digit from the top: a histogram
//           pass over the live rows whose decided digits equal the prefix (per-wave LDS copies, merged with integer
//           atomics), a pick by one workgroup (suffix sums of the 256 counts: the digit of the k-th largest key, the
//           rows still to take inside it).  After four digits the threshold key T and the number of ties to take are
//           known: the tie rows are counted per workgroup, the counts scanned, and the flag pass keeps key > T and the
//           first `ties` rows with key == T in row order (block_rank inside a workgroup).
//   select  count (selected rows per workgroup, live rows) -> scan -> scatter: out row = the workgroup's offset + the
//           row's rank inside it, so the compaction is stable; rows beyond the cap are cut in row order; the scatter
//           also writes the -1 tail of out_indices and src.  The rank map of the result, when asked for, is
//           spx_rankmap_from_sorted over out_indices: a subset of key-ordered rows is key-ordered.
#include "common.h"
#include "fill.h"
#include "piece.h"
#include "rankmap.h"
#include "scan.h"

namespace spx {
namespace {

constexpr int kBlock = 256;
static_assert(kBlock == kScanThreads, "scan.h's primitives are written for this unit's workgroup size");
constexpr int kDigits = 4, kBins = 256;               // 8-bit digits of the 32-bit key, most significant first
constexpr int kState = 8;                             // {prefix, rows still to take, live, k, -, -, -, -}
constexpr int kCounters = 4;                          // {selected rows, live rows, -, -}

enum { kOpMean = SPX_SCORE_ABSMEAN, kOpMax = SPX_SCORE_ABSMAX };

__device__ __forceinline__ float absval(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double absval(double v) { return __builtin_fabs(v); }
// IEEE 754-2019 maximum: a NaN on either side gives NaN (one v_maximum3_f32 on gfx950; fp64: a max and a select)
__device__ __forceinline__ float nan_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ double nan_max(double a, double b) { return __builtin_elementwise_maximum(a, b); }

// -------------------------------------------------------------------------------------------- row score

// Items = (row, lane of its group).  `aligned`: the row's 16-byte pieces can be loaded as such; otherwise the same
// elements arrive one by one, in the same order.
template <int DT, int V, int OP>
__global__ void __launch_bounds__(kBlock)
score_kernel(const void *__restrict__ feat_, int n, int C, int pieces, int gshift, int aligned,
             const int32_t *__restrict__ n_live, float *__restrict__ score) {
  using E = Elem<DT>;
  using S = typename E::S;
  using A = typename E::A;
  using P = Piece<S, V>;
  const S *feat = static_cast<const S *>(feat_);
  int nl = n;
  if (n_live) {
    nl = *n_live;
    nl = nl < 0 ? 0 : (nl > n ? n : nl);
  }
  const long long total = static_cast<long long>(n) << gshift;
  const int G = 1 << gshift;
  for (long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * kBlock) {
    const int i = static_cast<int>(item >> gshift);
    const int sub = static_cast<int>(item) & (G - 1);
    A acc = A(0);
    if (i < nl) {
      const S *row = feat + static_cast<size_t>(i) * C;
      for (int p = sub; p < pieces; p += G) {
        P v;
        if (V > 1 && aligned) {
          v = *reinterpret_cast<const P *>(row + static_cast<size_t>(p) * V);
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) v.e[j] = row[static_cast<size_t>(p) * V + j];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const A x = absval(E::up(v.e[j]));
          if (OP == kOpMean) acc += x;
          else acc = nan_max(acc, x);
        }
      }
    }
    // (groups are lane-aligned and whole: every partner below is an active lane of the same row)
    for (int d = G >> 1; d >= 1; d >>= 1) {
      const A o = __shfl_xor(acc, d, 64);
      if (OP == kOpMean) acc += o;
      else acc = nan_max(acc, o);
    }
    if (sub == 0) {
      float r = -__builtin_inff();
      if (i < nl) r = static_cast<float>(OP == kOpMean ? acc / static_cast<A>(C) : acc);
      score[i] = r;
    }
  }
}

// -------------------------------------------------------------------------------------------- top-k flags

__device__ __forceinline__ uint32_t score_key(float s) {
  const uint32_t b = __builtin_bit_cast(uint32_t, s);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

struct TopkRows {
  const float *score;
  const int32_t *indices;             // NULL, or [n, ndim + 1]
  const int32_t *n_live;
  int n, ndim, batch;
};

__device__ __forceinline__ int live_bound(const int32_t *__restrict__ n_live, int n) {
  if (!n_live) return n;
  const int v = *n_live;
  return v < 0 ? 0 : (v > n ? n : v);
}

__device__ __forceinline__ bool topk_live(const TopkRows &r, int nl, long long i) {
  if (i >= nl) return false;
  if (!r.indices) return true;
  const int b = r.indices[static_cast<size_t>(i) * (r.ndim + 1)];
  return static_cast<unsigned>(b) < static_cast<unsigned>(r.batch);
}

// Digit d (0 = the top byte) of the live rows whose d decided digits equal the prefix.
__global__ void __launch_bounds__(kBlock)
topk_hist_kernel(TopkRows r, int d, const uint32_t *__restrict__ state, int32_t *__restrict__ hist) {
  __shared__ int lds_hist[kBlock / 64][kBins];
  static_assert(kBins == kBlock, "a thread per bin");
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) lds_hist[w][threadIdx.x] = 0;
  __syncthreads();
  const int nl = live_bound(r.n_live, r.n);
  const uint32_t prefix = d ? state[0] : 0u;
  const int decided = 32 - 8 * d;                     // keys agree with the prefix above this bit (d > 0)
  const int shift = 24 - 8 * d;
  const int wave = threadIdx.x >> 6;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < r.n;
       i += static_cast<long long>(gridDim.x) * kBlock) {
    if (!topk_live(r, nl, i)) continue;
    const uint32_t key = score_key(r.score[i]);
    if (d == 0 || (key >> decided) == (prefix >> decided)) atomicAdd(&lds_hist[wave][(key >> shift) & 255u], 1);
  }
  __syncthreads();
  int c = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) c += lds_hist[w][threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], c);            // (an integer count: order-free)
}

// One workgroup: the digit of the k-th largest key among the rows that agree with the prefix, and how many rows are
// still to be taken inside that digit.  d == 0 also fixes live and k; d == 3 leaves sel_dev.
__global__ void __launch_bounds__(kBlock)
topk_pick_kernel(const int32_t *__restrict__ hist, int d, int k_abs, double ratio, uint32_t *__restrict__ state,
                 int32_t *__restrict__ sel_dev) {
  __shared__ int suffix[kBins];
  const int t = threadIdx.x;
  suffix[t] = hist[t];
  __syncthreads();
  for (int off = 1; off < kBins; off <<= 1) {         // suffix[t] = rows whose digit is >= t
    const int v = t + off < kBins ? suffix[t + off] : 0;
    __syncthreads();
    suffix[t] += v;
    __syncthreads();
  }
  int live, k, rem;
  uint32_t prefix = 0u;
  if (d == 0) {
    live = suffix[0];
    if (k_abs >= 0) {
      k = k_abs < live ? k_abs : live;
    } else {
      k = static_cast<int>(ratio * static_cast<double>(live));
      k = k < 0 ? 0 : (k > live ? live : k);          // (ratio is in [0, 1]: a no-op that keeps every index in range)
    }
    rem = k;
  } else {
    prefix = state[0];
    rem = static_cast<int>(state[1]);
    live = static_cast<int>(state[2]);
    k = static_cast<int>(state[3]);
  }
  __syncthreads();                                    // (every thread has read the state before one rewrites it)
  const int above = t + 1 < kBins ? suffix[t + 1] : 0;
  const int shift = 24 - 8 * d;
  if (rem > 0 && suffix[t] >= rem && above < rem) {   // exactly one thread: rem <= the rows that agree with the prefix
    const uint32_t p = prefix | (static_cast<uint32_t>(t) << shift);
    state[0] = p;
    state[1] = static_cast<uint32_t>(rem - above);
    if (d == kDigits - 1) {
      sel_dev[2] = static_cast<int32_t>(p);
      sel_dev[3] = rem - above;
    }
  }
  if (t == 0) {
    if (d == 0) {
      state[2] = static_cast<uint32_t>(live);
      state[3] = static_cast<uint32_t>(k);
      if (k == 0) {
        state[0] = 0u;
        state[1] = 0u;
      }
    }
    if (d == kDigits - 1) {
      sel_dev[0] = live;
      sel_dev[1] = k;
      if (rem == 0) {                                 // (k = 0: nothing is kept, no threshold)
        sel_dev[2] = -1;
        sel_dev[3] = 0;
      }
    }
  }
}

// state: {T, ties to take, live, k}
template <bool FLAGS>
__global__ void __launch_bounds__(kBlock)
topk_flags_kernel(TopkRows r, const uint32_t *__restrict__ state, int32_t *__restrict__ blockties,
                  const int32_t *__restrict__ blockoff, uint8_t *__restrict__ keep) {
  __shared__ int lds_wave[kBlock / 64];
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const int nl = live_bound(r.n_live, r.n);
  const uint32_t T = state[0];
  const int ties = static_cast<int>(state[1]), k = static_cast<int>(state[3]);
  const bool live = i < r.n && k > 0 && topk_live(r, nl, i);
  const uint32_t key = live ? score_key(r.score[i]) : 0u;
  const bool tie = live && key == T;
  int total;
  const int rank = block_rank(tie, total, lds_wave);
  if (!FLAGS) {
    if (threadIdx.x == 0) blockties[blockIdx.x] = total;
  } else if (i < r.n) {
    keep[i] = live && (key > T || (tie && blockoff[blockIdx.x] + rank < ties)) ? 1 : 0;
  }
}

// -------------------------------------------------------------------------------------------- row selection

struct SelRows {
  const int32_t *indices;
  const int32_t *n_live;
  const uint8_t *keep;
  int n, invert;
  LevelGeom g;
};

// a live row inside the level (level_holds of rankmap.h: the grid of a selection need not fit a key)
__device__ __forceinline__ bool sel_live(const SelRows &r, int nl, long long i) {
  return i < nl && level_holds(r.indices + static_cast<size_t>(i) * (r.g.ndim + 1), r.g);
}

__global__ void __launch_bounds__(kBlock)
select_count_kernel(SelRows r, int32_t *__restrict__ blockcount, int32_t *__restrict__ live_rows) {
  __shared__ int lds_wave[kBlock / 64];
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const int nl = live_bound(r.n_live, r.n);
  const bool live = i < r.n && sel_live(r, nl, i);
  const bool sel = live && ((r.keep[i] != 0) != (r.invert != 0));
  int total;
  block_rank(sel, total, lds_wave);
  if (threadIdx.x == 0) blockcount[blockIdx.x] = total;
  const unsigned long long bal = __ballot(live);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(live_rows, __popcll(bal));        // (an integer count: order-free)
}

// Exclusive scan of the blocks' counts by one workgroup; counters[0] = the selected rows, n_out_dev (static form) =
// {found, 0, live = min(found, cap)}.
__global__ void __launch_bounds__(kBlock)
select_scan_kernel(const int32_t *__restrict__ cnt, int32_t *__restrict__ off, int len, int cap,
                   int32_t *__restrict__ counters, int32_t *__restrict__ n_out_dev) {
  __shared__ int lds_wave[kBlock / 64];
  const int carry = block_scan_loop(cnt, off, len, lds_wave);
  if (threadIdx.x == 0) {
    counters[0] = carry;
    if (n_out_dev) {
      n_out_dev[0] = carry;
      n_out_dev[1] = 0;
      n_out_dev[2] = carry > cap ? cap : carry;
    }
  }
}

// Thread i serves input row i (its rows entry, and the output row it lands on) and output row i of the -1 tail.
__global__ void __launch_bounds__(kBlock)
select_scatter_kernel(SelRows r, const int32_t *__restrict__ blockoff, int nblk, const int32_t *__restrict__ found,
                      int cap, int32_t *__restrict__ rows, int32_t *__restrict__ src,
                      int32_t *__restrict__ out_indices) {
  __shared__ int lds_wave[kBlock / 64];
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const int nl = live_bound(r.n_live, r.n);
  const bool sel = i < r.n && sel_live(r, nl, i) && ((r.keep[i] != 0) != (r.invert != 0));
  int total;
  const int rank = block_rank(sel, total, lds_wave);
  const int width = r.g.ndim + 1;
  int o = -1;
  if (sel) {
    o = (static_cast<int>(blockIdx.x) < nblk ? blockoff[blockIdx.x] : 0) + rank;
    if (o >= cap) o = -1;                             // cut in row order
  }
  if (i < r.n) rows[i] = o;
  if (o >= 0) {
    src[o] = static_cast<int32_t>(i);
    const int32_t *from = r.indices + static_cast<size_t>(i) * width;
    int32_t *to = out_indices + static_cast<size_t>(o) * width;
    for (int c = 0; c < width; ++c) to[c] = from[c];
  }
  const int f = *found;
  if (i >= (f < cap ? f : cap) && i < cap) {
    src[i] = -1;
    int32_t *to = out_indices + static_cast<size_t>(i) * width;
    for (int c = 0; c < width; ++c) to[c] = -1;
  }
}

// -------------------------------------------------------------------------------------------- host side

// scratch of a top-k call: the four digits' histograms, the select's state, the blocks' tie counts and their scan
struct TopkWs {
  int32_t *hist;
  uint32_t *state;
  int32_t *blockties, *blockoff;
  int nblk;
  size_t bytes;
  TopkWs(void *ws, long long n) {
    Carver c(ws);
    nblk = static_cast<int>((n + kBlock - 1) / kBlock);
    hist = c.take<int32_t>(kDigits * kBins);
    state = c.take<uint32_t>(kState);
    blockties = c.take<int32_t>(nblk > 0 ? nblk : 1);
    blockoff = c.take<int32_t>(nblk > 0 ? nblk : 1);
    bytes = c.off;
  }
};

// scratch of a selection build: the blocks' counts, their scan, the counters
struct SelectWs {
  int32_t *blockcount, *blockoff, *counters;
  int nblk;
  size_t bytes;
  SelectWs(void *ws, long long n) {
    Carver c(ws);
    nblk = static_cast<int>((n + kBlock - 1) / kBlock);
    blockcount = c.take<int32_t>(nblk > 0 ? nblk : 1);
    blockoff = c.take<int32_t>(nblk > 0 ? nblk : 1);
    counters = c.take<int32_t>(kCounters);
    bytes = c.off;
  }
};

// 0 = ok: the checks every selection call shares, none of which looks at a pointer's target
int make_select(int n, int ndim, int batch, const int *spatial_h, int invert, const void *rankmap, size_t rankmap_bytes,
                LevelGeom &g) {
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  SPX_CHECK(invert == 0 || invert == 1, "invert must be 0 or 1, got %d", invert);
  SPX_CHECK(n >= 0, "bad row count %d", n);
  SPX_CHECK(batch >= 1, "batch must be >= 1, got %d", batch);
  SPX_CHECK(spatial_h, "spatial shape is NULL");
  g = LevelGeom(ndim, batch, spatial_h);
  if (rankmap) {
    const size_t W = rank_words(ndim, batch, spatial_h);
    SPX_CHECK(W > 0 && rankmap_bytes >= rank_bytes(W), "rank map too small, or the key space does not fit one (%zu words)", W);
  }
  return 0;
}

int count_rows(const SelRows &r, const SelectWs &w, int cap, int32_t *n_out_dev, hipStream_t s) {
  {
    FillList fills;                   // (the live rows' count starts at zero on every call)
    fills.add(w.counters, kCounters * sizeof(int32_t), 0u);
    SPX_HIP(fills.launch(s));
  }
  if (r.n > 0) {
    hipLaunchKernelGGL(select_count_kernel, dim3(w.nblk), dim3(kBlock), 0, s, r, w.blockcount, w.counters + 1);
    SPX_LAUNCH_CHECK();
    count(kSelCount);
  }
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(kBlock), 0, s, w.blockcount, w.blockoff, w.nblk, cap, w.counters,
                     n_out_dev);
  SPX_LAUNCH_CHECK();
  count(kSelScan);
  return 0;
}

int scatter_rows(const SelRows &r, const SelectWs &w, int cap, int32_t *out_indices, int32_t *rows, int32_t *src,
                 const int *spatial_h, void *rankmap, size_t rankmap_bytes, int32_t *violation, hipStream_t s) {
  const long long items = r.n > cap ? r.n : cap;
  if (items > 0) {
    hipLaunchKernelGGL(select_scatter_kernel, dim3(static_cast<unsigned>((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       r, w.blockoff, w.nblk, w.counters, cap, rows, src, out_indices);
    SPX_LAUNCH_CHECK();
    count(kSelScatter);
  }
  if (rankmap) {
    if (int rc = spx_rankmap_from_sorted(out_indices, cap, r.g.ndim, r.g.batch, spatial_h, rankmap, rankmap_bytes,
                                         violation, s))
      return rc;
    count(kSelMap);
  }
  return 0;
}

}  // namespace
}  // namespace spx

extern "C" {

int spx_row_score(const void *feat, int n, int C, int dtype, int op, const int32_t *n_live, float *score,
                  spx_stream_t stream) {
  using namespace spx;
  const int eb = float_row_elem(dtype, C);
  if (eb < 0) return eb;
  SPX_CHECK(op == kOpMean || op == kOpMax, "op must be absmean (0) or absmax (1), got %d", op);
  SPX_CHECK(n >= 0, "bad row count %d", n);
  if (n == 0) return 0;
  SPX_CHECK(feat && score, "feat / score is NULL");
  SPX_CHECK(aligned_to(feat, eb) && aligned_to(score, 4), "pointer not aligned to its elements");
  const bool vec = (static_cast<long long>(C) * eb) % 16 == 0, aligned = aligned_to(feat, 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_row(dtype, vec, [&](auto dt, auto v) {
    const int pieces = C / v, gshift = group_shift(pieces);
    dispatch_value<kOpMean, kOpMax>(op, [&](auto o) {
      hipLaunchKernelGGL((score_kernel<dt, v, o>), dim3(stream_blocks(static_cast<long long>(n) << gshift, kBlock)),
                         dim3(kBlock), 0, s, feat, n, C, pieces, gshift, vec && aligned ? 1 : 0, n_live, score);
    });
  });
  SPX_LAUNCH_CHECK();
  count(kSelScore);
  return 0;
}

size_t spx_topk_ws_bytes(long long n) {
  if (n < 0 || n > 0x7fffffffLL) return 0;
  return spx::TopkWs(nullptr, n).bytes;
}

int spx_topk_flags(const float *score, const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch,
                   int k_abs, double ratio, uint8_t *keep, int32_t *sel_dev, void *ws, size_t ws_bytes,
                   spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(n >= 0, "bad row count %d", n);
  SPX_CHECK(k_abs >= 0 || (ratio >= 0.0 && ratio <= 1.0), "ratio must be in [0, 1], got %g", ratio);
  SPX_CHECK(!indices || (ndim >= 1 && ndim <= kMaxNdim && batch >= 1), "with indices: ndim in [1,4] and batch >= 1, got %d / %d",
            ndim, batch);
  SPX_CHECK(sel_dev && (n == 0 || (score && keep)), "score / keep / sel_dev is NULL");
  TopkWs w(ws, n);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  {
    FillList fills;
    fills.add(w.hist, kDigits * kBins * sizeof(int32_t), 0u);
    fills.add(w.state, kState * sizeof(uint32_t), 0u);
    SPX_HIP(fills.launch(s));
  }
  const TopkRows r{score, indices, n_live, n, ndim, batch};
  for (int d = 0; d < kDigits; ++d) {
    if (n > 0) {
      hipLaunchKernelGGL(topk_hist_kernel, dim3(stream_blocks(n, kBlock)), dim3(kBlock), 0, s, r, d, w.state,
                         w.hist + d * kBins);
      SPX_LAUNCH_CHECK();
      count(kSelHist);
    }
    hipLaunchKernelGGL(topk_pick_kernel, dim3(1), dim3(kBlock), 0, s, w.hist + d * kBins, d, k_abs, ratio, w.state,
                       sel_dev);
    SPX_LAUNCH_CHECK();
    count(kSelPick);
  }
  if (n == 0) return 0;
  hipLaunchKernelGGL(topk_flags_kernel<false>, dim3(w.nblk), dim3(kBlock), 0, s, r, w.state, w.blockties, w.blockoff,
                     keep);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScanThreads), 0, s, w.blockties, w.blockoff, w.nblk,
                     static_cast<int32_t *>(nullptr));
  SPX_LAUNCH_CHECK();
  count(kSelTies);
  hipLaunchKernelGGL(topk_flags_kernel<true>, dim3(w.nblk), dim3(kBlock), 0, s, r, w.state, w.blockties, w.blockoff,
                     keep);
  SPX_LAUNCH_CHECK();
  count(kSelFlags);
  return 0;
}

size_t spx_select_ws_bytes(int ndim, long long n) {
  if (ndim < 1 || ndim > spx::kMaxNdim || n < 0 || n > 0x7fffffffLL) return 0;
  return spx::SelectWs(nullptr, n).bytes;
}

int spx_select_count(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, const int *spatial_h,
                     const uint8_t *keep, int invert, void *ws, size_t ws_bytes, int *result_h, spx_stream_t stream) {
  using namespace spx;
  LevelGeom g;
  if (int rc = make_select(n, ndim, batch, spatial_h, invert, nullptr, 0, g)) return rc;
  SPX_CHECK(result_h && (n == 0 || (indices && keep)), "result_h / indices / keep is NULL");
  SelectWs w(ws, n);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const SelRows r{indices, n_live, keep, n, invert, g};
  if (int rc = count_rows(r, w, 0x7fffffff, nullptr, s)) return rc;
  int32_t host[kCounters];
  SPX_HIP(hipMemcpyAsync(host, w.counters, sizeof(host), hipMemcpyDeviceToHost, s));
  SPX_HIP(hipStreamSynchronize(s));
  result_h[0] = host[0];
  result_h[1] = host[1];
  return 0;
}

int spx_select_fill(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, const int *spatial_h,
                    const uint8_t *keep, int invert, int n_out, int32_t *out_indices, int32_t *rows, int32_t *src,
                    void *rankmap, size_t rankmap_bytes, int32_t *violation, const void *ws, size_t ws_bytes,
                    spx_stream_t stream) {
  using namespace spx;
  LevelGeom g;
  if (int rc = make_select(n, ndim, batch, spatial_h, invert, rankmap, rankmap_bytes, g)) return rc;
  SPX_CHECK(n_out >= 0 && n_out <= n, "n_out = %d outside [0, rows = %d]", n_out, n);
  SPX_CHECK((n == 0 || (indices && keep && rows)) && (n_out == 0 || (out_indices && src)),
            "indices / keep / out_indices / rows / src is NULL");
  SelectWs w(const_cast<void *>(ws), n);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  const SelRows r{indices, n_live, keep, n, invert, g};
  return scatter_rows(r, w, n_out, out_indices, rows, src, spatial_h, rankmap, rankmap_bytes, violation,
                      static_cast<hipStream_t>(stream));
}

int spx_select_static(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, const int *spatial_h,
                      const uint8_t *keep, int invert, int n_out_cap, int32_t *out_indices, int32_t *rows,
                      int32_t *src, int32_t *n_out_dev, void *rankmap, size_t rankmap_bytes, int32_t *violation,
                      void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  LevelGeom g;
  if (int rc = make_select(n, ndim, batch, spatial_h, invert, rankmap, rankmap_bytes, g)) return rc;
  SPX_CHECK(n_out_cap > 0 && n_out_dev && out_indices && src, "n_out_cap must be > 0, and n_out_dev / out_indices / src not NULL");
  SPX_CHECK(n == 0 || (indices && keep && rows), "indices / keep / rows is NULL");
  SelectWs w(ws, n);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // every launch is stream-ordered and nothing is read back: the call can sit in a hipGraph
  const SelRows r{indices, n_live, keep, n, invert, g};
  if (int rc = count_rows(r, w, n_out_cap, n_out_dev, s)) return rc;
  return scatter_rows(r, w, n_out_cap, out_indices, rows, src, spatial_h, rankmap, rankmap_bytes, violation, s);
}

}  // extern "C"
