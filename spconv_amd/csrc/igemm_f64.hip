// Float64 gather-GEMM, input gradient, weight gradient and bias / activation epilogue for gfx950 (MI355X).
//
// Every product and every sum is float64: the matrix work runs on v_mfma_f64_16x16x4_f64, the partial weight-gradient
// tiles are float64, the second stage sums them in float64.  The layers accept any channel count (tails are predicated
// loads and stores), any kernel volume in one launch and every table form of the 16-bit / fp32 kernels, so that a model
// converted with .double() runs the same code path and `torch.autograd.gradcheck` can be pointed at it.
//
//  * gemm_f64_kernel: output-stationary implicit GEMM for the forward (out[o] = sum_k feat[pair[k][o]] W_k^T) and the
//    input gradient (din[i] = sum_k dout[pair[k][i]] W_k).  One 256-thread workgroup owns 64 destination rows x 64
//    output channels; wave w computes rows 16w .. 16w + 15 of the tile as four 16 x 16 accumulators.  For every offset
//    some row of the tile has, the 64 source rows are gathered in 16-element pieces into LDS next to the matching
//    [64 x 16] weight piece, and each wave issues 4 x 4 MFMAs per piece.  Every destination row is written once, no
//    atomics.
//  * wgrad_f64_kernel + wgrad_f64_reduce_kernel: dW[:, k, :] = sum_j dout[out_j]^T (x) feat[in_j] over the Native pair
//    lists.  Each offset's list is cut into fixed chunks; a workgroup contracts one chunk into a 64 x 64 float64 partial
//    tile, and a second launch sums the partial tiles of every offset in chunk order.  No floating-point atomics: two
//    backward passes give bit-identical results.
//
// MFMA fragment layout of v_mfma_f64_16x16x4_f64 (D = A[16x4] B[4x16] + C): lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15]; the four accumulator values of lane l are D[(l >> 4) + 4 r][l & 15], r = 0 .. 3.  (The f32 16x16
// forms put row 4 (l >> 4) + r there instead.)
//
// All addressing is 64-bit (flat global loads, size_t offsets): no tensor size wraps a 32-bit buffer offset.  Nothing is
// read back to the host; the launches are shaped by the call's sizes only, so the path can be captured in a graph.
#include "igemm_defs.h"

namespace spx {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kF64Threads = 256;
constexpr int kF64TM = 64;            // destination rows per workgroup
constexpr int kF64TN = 64;            // output channels per workgroup
constexpr int kF64KC = 16;            // reduction elements staged per step
constexpr int kF64Ld = kF64KC + 1;    // LDS row stride (doubles): conflict-free fragment reads
constexpr int kF64MaxWords = 16;      // mask words the tile OR keeps (kernel volumes up to 512; beyond: pair table)

constexpr int kWF64T = 64;            // weight-gradient tile edge
constexpr int kWF64J = 16;            // pairs staged per step
constexpr int kWF64Ld = kWF64T + 16;  // LDS row stride (doubles): the two half-wave rows land on disjoint banks

__device__ __forceinline__ f64x4 mfma_f64(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ double act_f64(double v, int act, float alpha) {
  if (act == SPX_ACT_RELU) return !(v <= 0.0) ? v : 0.0;      // (NaN stays NaN, as torch.relu has it)
  if (act == SPX_ACT_LEAKY_RELU) return v > 0.0 ? v : v * static_cast<double>(alpha);
  if (act == SPX_ACT_SIGMOID) return 1.0 / (1.0 + exp(-v));
  return v;
}

// GemmParams as for the other gather-GEMMs (igemm_defs.h), tables by row or in tile order (no rows layout: the caller
// drops it).  B element (k, n, c) at k * strideK + n * strideN + c * strideD.
__global__ void __launch_bounds__(kF64Threads)
gemm_f64_kernel(GemmParams p) {
  __shared__ double As[kF64TM * kF64Ld];
  __shared__ double Bs[kF64TN * kF64Ld];
  __shared__ int dst_row[kF64TM];
  __shared__ int src_row[kF64TM];
  __shared__ uint32_t tile_mask[kF64MaxWords];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long t0 = static_cast<long long>(blockIdx.x) * kF64TM;
  const int n0 = blockIdx.y * kF64TN;
  const int words = (p.kv + 31) >> 5;
  const bool tile_skip = p.mask && words <= kF64MaxWords;
  const double *A = static_cast<const double *>(p.A);
  const double *B = static_cast<const double *>(p.B);
  if (tid < kF64TM) {
    const long long t = t0 + tid;
    dst_row[tid] = t < p.n_dst ? (p.argsort ? p.argsort[t] : static_cast<int>(t)) : -1;
  }
  if (tid < kF64MaxWords) tile_mask[tid] = 0u;
  __syncthreads();
  if (tile_skip && tid < kF64TM && dst_row[tid] >= 0) {
    const long long tr = p.tile_order ? t0 + tid : dst_row[tid];
    for (int w = 0; w < words; ++w) atomicOr(&tile_mask[w], p.mask[static_cast<size_t>(tr) * words + w]);
  }
  __syncthreads();

  f64x4 acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) acc[nb] = f64x4{0.0, 0.0, 0.0, 0.0};
  // fragment reads, reduction index lane >> 4: A row 16 wave + (lane & 15), B column 16 nb + (lane & 15)
  const int arow = (wave * 16 + (lane & 15)) * kF64Ld + (lane >> 4);
  const int bcol = (lane & 15) * kF64Ld + (lane >> 4);

  for (int k = 0; k < p.kv; ++k) {
    if (tile_skip && !((tile_mask[k >> 5] >> (k & 31)) & 1u)) continue;      // no row of the tile has this offset
    int have = 0;
    if (tid < kF64TM) {
      const int r = dst_row[tid];
      int s = -1;
      if (r >= 0) {
        const long long tr = p.tile_order ? t0 + tid : r;
        const bool on = !p.mask || ((p.mask[static_cast<size_t>(tr) * words + (k >> 5)] >> (k & 31)) & 1u);
        if (on) s = k == p.identity_k ? r : p.pair[static_cast<size_t>(k) * p.n_dst + tr];
      }
      src_row[tid] = s;
      have = s >= 0;
    }
    if (!__syncthreads_or(have)) continue;
    const long long kb = p.b_reverse ? p.kv - 1 - k : k;
    for (int c0 = 0; c0 < p.CIN; c0 += kF64KC) {
      // Every load of the step is issued before the first LDS store: out-of-range elements read element 0 (some source
      // row exists, or the offset was skipped) and are replaced by zeros afterwards.  Gathered rows: 16 consecutive
      // threads read one row's 128-byte piece; the weight piece [n][c] is walked along the layout's contiguous index
      // (c forward, n dgrad).
      constexpr int kPer = kF64TM * kF64KC / kF64Threads;
      double av[kPer], bv[kPer];
      bool aok[kPer], bok[kPer];
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int e = tid + i * kF64Threads, row = e / kF64KC, c = e % kF64KC;
        const int s = src_row[row];
        aok[i] = s >= 0 && c0 + c < p.CIN;
        av[i] = A[aok[i] ? static_cast<size_t>(s) * p.CIN + c0 + c : 0];
        const int n = p.strideD == 1 ? e / kF64KC : e % kF64TN, cb = p.strideD == 1 ? e % kF64KC : e / kF64TN;
        bok[i] = n0 + n < p.COUT && c0 + cb < p.CIN;
        bv[i] = B[bok[i] ? kb * p.strideK + static_cast<long long>(n0 + n) * p.strideN +
                               static_cast<long long>(c0 + cb) * p.strideD
                         : 0];
      }
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int e = tid + i * kF64Threads;
        As[(e / kF64KC) * kF64Ld + e % kF64KC] = aok[i] ? av[i] : 0.0;
        const int n = p.strideD == 1 ? e / kF64KC : e % kF64TN, cb = p.strideD == 1 ? e % kF64KC : e / kF64TN;
        Bs[n * kF64Ld + cb] = bok[i] ? bv[i] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < kF64KC / 4; ++s) {
        const double a = As[arow + 4 * s];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)    // (columns past COUT were staged as zeros)
          acc[nb] = mfma_f64(a, Bs[nb * 16 * kF64Ld + bcol + 4 * s], acc[nb]);
      }
      __syncthreads();
    }
  }

  const double *bias = static_cast<const double *>(p.bias);
  double *out = static_cast<double *>(p.out);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    const int col = n0 + nb * 16 + (lane & 15);
    if (col >= p.COUT) continue;
    const double b = bias ? bias[col] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int d = dst_row[wave * 16 + (lane >> 4) + 4 * r];
      if (d >= 0) out[static_cast<size_t>(d) * p.COUT + col] = act_f64(acc[nb][r] + b, p.act, p.act_alpha);
    }
  }
}

struct WgradF64Params {
  const double *feat;      // [n_in, C]
  const double *dout;      // [n_out, K]
  double *partial;         // [kv][nchunks][tiles][64 * 64]
  const int32_t *native;   // [2, kv, n_in]
  const int32_t *num;      // [kv] device counts
  int n_in, C, K, kv, subm, chunk, nchunks, tiles_c, tiles_k;
};

__device__ __forceinline__ int f64_list_count(const WgradF64Params &q, int k) {
  int c;
  if (!q.subm) c = q.num[k];
  else if (k == q.kv / 2) c = q.n_in;
  else c = k < q.kv / 2 ? q.num[k] : q.num[q.kv - 1 - k];   // mirror rule, ops.py:962-968
  return c < q.n_in ? c : q.n_in;
}

// grid (nchunks, kv, tiles): chunk blockIdx.x of offset blockIdx.y's list into the float64 partial tile blockIdx.z.
// Chunks past the list's end leave at once (the grid is sized without reading the counts back).
__global__ void __launch_bounds__(kF64Threads)
wgrad_f64_kernel(WgradF64Params q) {
  __shared__ double Ds[kWF64J * kWF64Ld];    // [pair][dout channel]
  __shared__ double Fs[kWF64J * kWF64Ld];    // [pair][feature channel]
  const int k = blockIdx.y, ch = blockIdx.x, tile = blockIdx.z;
  const int cnt = f64_list_count(q, k);
  const int begin = ch * q.chunk;
  if (begin >= cnt) return;
  const int end = cnt - begin < q.chunk ? cnt : begin + q.chunk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = (tile / q.tiles_c) * kWF64T, c0 = (tile % q.tiles_c) * kWF64T;
  const bool identity = q.subm && k == q.kv / 2;
  const int32_t *in_list = q.native + static_cast<size_t>(k) * q.n_in;
  const int32_t *out_list = q.native + static_cast<size_t>(q.kv + k) * q.n_in;
  f64x4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc[cb] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int frag = (lane >> 4) * kWF64Ld + (lane & 15);
  constexpr int kPer = kWF64J * kWF64T / kF64Threads;
  for (int j0 = begin; j0 < end; j0 += kWF64J) {
    // all list words first, then all rows (out-of-range elements read the first pair's and become zeros)
    int oi[kPer], ii[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int jj = j0 + (tid + i * kF64Threads) / kWF64T;
      const int jc = jj < end ? jj : begin;
      oi[i] = identity ? jc : out_list[jc];
      ii[i] = identity ? jc : in_list[jc];
    }
    double dv[kPer], fv[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int col = (tid + i * kF64Threads) % kWF64T;
      dv[i] = q.dout[static_cast<size_t>(oi[i]) * q.K + (n0 + col < q.K ? n0 + col : 0)];
      fv[i] = q.feat[static_cast<size_t>(ii[i]) * q.C + (c0 + col < q.C ? c0 + col : 0)];
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int e = tid + i * kF64Threads, j = e / kWF64T, col = e % kWF64T;
      const bool in = j0 + j < end;
      Ds[j * kWF64Ld + col] = in && n0 + col < q.K ? dv[i] : 0.0;
      Fs[j * kWF64Ld + col] = in && c0 + col < q.C ? fv[i] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kWF64J / 4; ++s) {     // (channels past K / C were staged as zeros)
      const double a = Ds[4 * s * kWF64Ld + frag + wave * 16];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[cb] = mfma_f64(a, Fs[4 * s * kWF64Ld + frag + cb * 16], acc[cb]);
    }
    __syncthreads();
  }
  const int ntile = q.tiles_c * q.tiles_k;
  double *dst = q.partial + ((static_cast<size_t>(k) * q.nchunks + ch) * ntile + tile) * (kWF64T * kWF64T);
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dst[(wave * 16 + (lane >> 4) + 4 * r) * kWF64T + cb * 16 + (lane & 15)] = acc[cb][r];
}

// dw[n][k][c] = sum over the chunks of offset k's list, in chunk order (deterministic); 0 for an empty list
__global__ void __launch_bounds__(kF64Threads)
wgrad_f64_reduce_kernel(WgradF64Params q, double *__restrict__ dw) {
  const long long gid = static_cast<long long>(blockIdx.x) * kF64Threads + threadIdx.x;
  const long long per_k = static_cast<long long>(q.K) * q.C;
  if (gid >= per_k * q.kv) return;
  const int k = static_cast<int>(gid / per_k);
  const long long rem = gid - k * per_k;
  const int n = static_cast<int>(rem / q.C), c = static_cast<int>(rem % q.C);
  const int cnt = f64_list_count(q, k);
  const int nch = (cnt + q.chunk - 1) / q.chunk;
  const int ntile = q.tiles_c * q.tiles_k;
  const int tile = (n / kWF64T) * q.tiles_c + c / kWF64T;
  const size_t stride = static_cast<size_t>(ntile) * (kWF64T * kWF64T);
  const double *src = q.partial + (static_cast<size_t>(k) * q.nchunks * ntile + tile) * (kWF64T * kWF64T) +
                      (n % kWF64T) * kWF64T + c % kWF64T;
  double s = 0.0;
  for (int ch = 0; ch < nch; ++ch) s += src[static_cast<size_t>(ch) * stride];
  dw[(static_cast<size_t>(n) * q.kv + k) * q.C + c] = s;
}

__global__ void __launch_bounds__(kF64Threads)
bias_act_f64_kernel(double *__restrict__ out, const double *__restrict__ bias, long long total, int K, int act,
                    float alpha) {
  const long long gid = static_cast<long long>(blockIdx.x) * kF64Threads + threadIdx.x;
  if (gid >= total) return;
  double v = out[gid];
  if (bias) v += bias[gid % K];
  out[gid] = act_f64(v, act, alpha);
}

// pairs per weight-gradient chunk: ~128 chunks for the identity list, whole 256-pair multiples
int wgrad_f64_chunk(int n_in) {
  int c = ((n_in / 128 + 255) / 256) * 256;
  if (c < 256) c = 256;
  if (c > 4096) c = 4096;
  return c;
}

}  // namespace

int run_gather_gemm_f64(const GemmParams &p0, bool dgrad, hipStream_t s) {
  if (p0.n_dst == 0) return 0;
  GemmParams p = p0;
  drop_rows_layout(p);          // the rows layout's appendix tables are walked by row, as by the generic kernel
  SPX_CHECK(p.CIN > 0 && p.COUT > 0 && p.kv > 0, "bad sizes");
  const dim3 grid(static_cast<unsigned>(div_up(p.n_dst, kF64TM)), static_cast<unsigned>(div_up(p.COUT, kF64TN)));
  count(kFamF64);
  count(dgrad ? kF64Dgrad : kF64Fwd);
  hipLaunchKernelGGL(gemm_f64_kernel, grid, dim3(kF64Threads), 0, s, p);
  SPX_LAUNCH_CHECK();
  return 0;
}

size_t wgrad_f64_ws_bytes(int n_in, int C, int K, int kv) {
  const size_t nchunks = div_up(n_in > 0 ? n_in : 1, wgrad_f64_chunk(n_in));
  const size_t tiles = static_cast<size_t>(div_up(C, kWF64T)) * div_up(K, kWF64T);
  return align_up(static_cast<size_t>(kv) * nchunks * tiles * kWF64T * kWF64T * sizeof(double), 256);
}

int wgrad_f64(const void *feat, const void *dout, void *dw, const int32_t *pair_native, const int32_t *num_per_loc,
              int n_in, int C, int K, int kv, int subm, void *ws, size_t ws_bytes, hipStream_t s) {
  SPX_CHECK(feat && dout && dw && ws, "null tensor pointer");
  SPX_CHECK(pair_native && num_per_loc, "Native pair lists and counts are required");
  SPX_CHECK(ws_bytes >= wgrad_f64_ws_bytes(n_in, C, K, kv),
            "workspace too small for the float64 weight gradient (spx_igemm_wgrad_ws_bytes_dtype)");
  WgradF64Params q{};
  q.feat = static_cast<const double *>(feat);
  q.dout = static_cast<const double *>(dout);
  q.partial = static_cast<double *>(ws);
  q.native = pair_native;
  q.num = num_per_loc;
  q.n_in = n_in;
  q.C = C;
  q.K = K;
  q.kv = kv;
  q.subm = subm;
  q.chunk = wgrad_f64_chunk(n_in);
  q.nchunks = div_up(n_in > 0 ? n_in : 1, q.chunk);
  q.tiles_c = div_up(C, kWF64T);
  q.tiles_k = div_up(K, kWF64T);
  SPX_CHECK(kv <= 65535 && q.tiles_c * q.tiles_k <= 65535, "kernel volume / channel counts beyond the launch grid");
  const dim3 grid(static_cast<unsigned>(q.nchunks), static_cast<unsigned>(kv),
                  static_cast<unsigned>(q.tiles_c * q.tiles_k));
  count(kF64Wgrad);
  hipLaunchKernelGGL(wgrad_f64_kernel, grid, dim3(kF64Threads), 0, s, q);
  SPX_LAUNCH_CHECK();
  const long long total = static_cast<long long>(K) * C * kv;
  hipLaunchKernelGGL(wgrad_f64_reduce_kernel, dim3(static_cast<unsigned>((total + kF64Threads - 1) / kF64Threads)),
                     dim3(kF64Threads), 0, s, q, static_cast<double *>(dw));
  SPX_LAUNCH_CHECK();
  return 0;
}

int bias_act_f64(void *out, const void *bias, int n, int K, int act, float act_alpha, hipStream_t s) {
  const long long total = static_cast<long long>(n) * K;
  if (total == 0) return 0;
  hipLaunchKernelGGL(bias_act_f64_kernel, dim3(static_cast<unsigned>((total + kF64Threads - 1) / kF64Threads)),
                     dim3(kF64Threads), 0, s, static_cast<double *>(out), static_cast<const double *>(bias), total, K,
                     act, act_alpha);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // namespace spx
