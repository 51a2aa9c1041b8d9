// Sparse convolution gather-GEMM for gfx950 (MI355X): dispatch and the C ABI of forward, int8 forward, dgrad and
// the fused backward.
//
//  * run_gather_gemm / run_gather_gemm_single: which kernel a layer takes (mfma_ok) -- the output-stationary MFMA
//    kernels of igemm_v4.h (f16 instantiated here, the other operand types in their own units), their column-blocked,
//    weight-stationary and first-generation relatives, or the generic kernel below -- and the group loop of kernel
//    volumes 33 .. 128.
//  * gather_gemm_generic_kernel: one thread per output element, fp32 accumulate, any dtype / channel count.
//  * the fused backward driver: dgrad tiles and wgrad ranges in one launch (igemm_bwd.h, f16 instantiated here); the
//    weight gradient itself -- kernels, plan, work split, second stage -- lives in igemm_wgrad.hip.
//  * bias_act, pad_rows, and the timeline dump of the debug build.
//
// Roofline note: at C=K=64 these kernels are HBM/L2-bandwidth bound (SURVEY.md
// section 8d): ~110 MB of compulsory traffic per fwd+bwd at 100k voxels versus
// 2.5 GFLOP, so the design spends its effort on coalesced 128-byte row
// gathers, mask-predicated rulebook reads and single-pass outputs, not on MFMA
// utilisation.
#include <cstring>
#include "igemm_bwd.h"

namespace spx {
namespace {

// --------------------------------------------------------------------------
// generic gather-GEMM: any dtype / channel count, fp32 accumulate.
// one thread per (dst row, out channel).
// --------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kThreads)
gather_gemm_generic_kernel(GemmParams p) {
  const long long gid = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  const long long total = static_cast<long long>(p.n_dst) * p.COUT;
  if (gid >= total) return;
  const int d = static_cast<int>(gid / p.COUT), n = static_cast<int>(gid % p.COUT);
  const T *A = static_cast<const T *>(p.A);
  const T *B = static_cast<const T *>(p.B);
  const int words = (p.kv + 31) / 32;
  float acc = 0.f;
  for (int k = 0; k < p.kv; ++k) {
    if (p.mask && !((p.mask[static_cast<size_t>(d) * words + (k >> 5)] >> (k & 31)) & 1u)) continue;
    const int idx = (k == p.identity_k) ? d : p.pair[static_cast<size_t>(k) * p.n_dst + d];
    if (idx < 0) continue;
    const int kb = p.b_reverse ? p.kv - 1 - k : k;
    const T *a = A + static_cast<size_t>(idx) * p.CIN;
    const T *b = B + static_cast<size_t>(kb) * p.strideK + static_cast<size_t>(n) * p.strideN;
    for (int c = 0; c < p.CIN; ++c) acc = fmaf(load_f(a + c), load_f(b + c * p.strideD), acc);
  }
  if (p.bias) acc += load_f(static_cast<const T *>(p.bias) + n);
  acc = apply_act(acc, p.act, p.act_alpha);
  store_f(static_cast<T *>(p.out) + static_cast<size_t>(d) * p.COUT + n, acc);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
bias_act_kernel(T *__restrict__ out, const T *__restrict__ bias, long long total, int K, int act,
                float alpha) {
  const long long gid = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (gid >= total) return;
  float v = load_f(out + gid);
  if (bias) v += load_f(bias + gid % K);
  store_f(out + gid, apply_act(v, act, alpha));
}

bool mfma_ok(int dtype, int cin, int cout, int kv) {
  if (dtype != SPX_F16 && dtype != SPX_BF16 && dtype != SPX_F32) return false;
  if (cin % (dtype == SPX_F32 ? 4 : 8) != 0) return false;     // 16-byte lane pieces
  if (kv > 128) return false;                                  // 33 .. 128: groups of 32 offsets
  if (cout == 16 || cout == 32 || cout == 64 || cout == 128 || cout == 256) return true;
  // beyond 256: the column-blocked launch (igemm_wide.hip); SPX_WIDE = 0 keeps the generic kernel (A/B runs:
  // tools/bench_wide.py -- the tables must then be the row-order ones: tables in tile order are an error on that kernel)
  return wide_cout(cout) && option_int("SPX_WIDE", 1) != 0;
}

int run_gather_gemm_single(const GemmParams &p, int dtype, hipStream_t s);

// Kernel volumes 33 .. 128 (5x5x5, 4-d 3^4, ...): the reference covers them with multi-word masks
// (indices.py:1601-1618, ops.py:448,494-503); here the layer runs as ceil(kv / 32) launches of the same
// kernel, one mask word each, whose partial sums travel through an fp32 [n_dst, COUT] scratch -- the
// result is rounded once, like a single launch.
int run_gather_gemm(const GemmParams &p, int dtype, hipStream_t s) {
  if (p.n_dst == 0) return 0;
  if (p.kv <= 32 || !mfma_ok(dtype, p.CIN, p.COUT, p.kv) || !p.pair) return run_gather_gemm_single(p, dtype, s);
  const int words = div_up(p.kv, 32);
  const bool fits = fits32(p.n_dst, words, 4) &&          // the group's mask words, row stride `words`
                    fits32(p.n_dst, p.COUT, 4) &&         // the fp32 scratch
                    v4_ok(p, dtype == SPX_F32 ? 4 : 2, dtype == SPX_F32 ? 4 : 2) && !p.argsort;
  if (!fits || !p.acc) {
    GemmParams q = p;                 // no scratch / beyond 32-bit offsets: the generic kernel
    q.acc = nullptr;
    return run_gather_gemm_single(q, dtype, s);
  }
  for (int g = 0; g < words; ++g) {
    GemmParams q = p;
    q.kbase = 32 * g;
    q.pair = p.pair + static_cast<size_t>(32 * g) * p.n_dst;
    q.mask = p.mask ? p.mask + g : nullptr;
    q.mask_words = p.mask ? words : 1;
    q.identity_k = (p.identity_k >= 32 * g && p.identity_k < 32 * g + 32) ? p.identity_k - 32 * g : -1;
    q.acc_mode = (g > 0 ? 1 : 0) | (g < words - 1 ? 2 : 0);
    if (int rc = run_gather_gemm_single(q, dtype, s)) return rc;
  }
  return 0;
}

int run_gather_gemm_single(const GemmParams &p, int dtype, hipStream_t s) {
  if (p.n_dst == 0) return 0;
  const bool grouped = p.acc_mode != 0;
  if (dtype == SPX_F32 && mfma_ok(dtype, p.CIN, p.COUT, p.kv) && v4_ok(p, 4, 4) &&
      (p.kv <= 32 || grouped))
    return dispatch_gather_gemm_f32(p, s);
  // (widths beyond 256 have no first-generation instance: past the 32-bit buffer offsets they keep the generic kernel)
  if (dtype != SPX_F32 && mfma_ok(dtype, p.CIN, p.COUT, p.kv) && (p.kv <= 32 || grouped) &&
      (!wide_cout(p.COUT) || v4_ok(p)))
    return dtype == SPX_BF16 ? dispatch_gather_gemm_bf16(p, s) : dispatch_gather_gemm<false>(p, s);
  if (p.cls) {                     // (as above: the generic kernel reads the tables by row)
    GemmParams q = p;
    drop_rows_layout(q);
    return run_gather_gemm_single(q, dtype, s);
  }
  if (p.tile_order) {
    set_error("tables in tile order are supported by the MFMA kernels only (channel counts / kernel volume)");
    return -1;
  }
  const long long total = static_cast<long long>(p.n_dst) * p.COUT;
  const dim3 grid(static_cast<unsigned>((total + kThreads - 1) / kThreads));
  count(kFamGeneric);
  if (int rc = with_elem_type(dtype, [&](auto t, auto slot) {
        count_inst<inst::generic(decltype(slot)::value)>();
        hipLaunchKernelGGL(gather_gemm_generic_kernel<decltype(t)>, grid, dim3(kThreads), 0, s, p);
      }))
    return rc;
  SPX_LAUNCH_CHECK();
  return 0;
}

GemmParams dgrad_params(const void *dout, const void *weight, void *din, const int32_t *pair,
                        const uint32_t *mask, const int32_t *argsort, int n_out, int n_in, int C,
                        int K, int kv, int subm) {
  GemmParams p{};
  p.A = dout;
  p.B = weight;                                   // KRSC read in place: (k, n=c, d=kk)
  p.out = din;
  p.pair = pair;
  p.mask = mask;
  p.argsort = argsort;
  p.bias = nullptr;
  p.strideK = C;
  p.strideN = 1;
  p.strideD = static_cast<long long>(kv) * C;
  p.n_src = n_out;
  p.n_dst = n_in;
  p.CIN = K;
  p.COUT = C;
  p.kv = kv;
  p.identity_k = subm ? kv / 2 : -1;
  p.b_reverse = subm ? 1 : 0;
  p.act = SPX_ACT_NONE;
  p.act_alpha = 0.f;
  return p;
}

// what the forward and the int8 forward share; act, layout and epilogue are the caller's
GemmParams fwd_params(const void *feat, const void *weight, void *out, const int32_t *pair, const uint32_t *mask,
                      const int32_t *argsort, const void *bias, int n_in, int n_out, int C, int K, int kv,
                      int identity_k) {
  GemmParams p{};
  p.A = feat;
  p.B = weight;
  p.out = out;
  p.pair = pair;
  p.mask = mask;
  p.argsort = argsort;
  p.bias = bias;
  p.strideK = C;                                  // KRSC: W[n][k][c]
  p.strideN = static_cast<long long>(kv) * C;
  p.strideD = 1;
  p.n_src = n_in;
  p.n_dst = n_out;
  p.CIN = C;
  p.COUT = K;
  p.kv = kv;
  p.identity_k = identity_k;
  p.b_reverse = 0;
  return p;
}

// rows of `sw` 16-bit words copied into rows of `dw` >= sw words, the tail zero-filled: the channel padding of a layer
// whose width the MFMA kernels are not instantiated for (a backbone's 3-5 channel first layer) in ONE launch -- torch's
// pad is a fill and a copy
__global__ void __launch_bounds__(kThreads)
pad_rows_kernel(const uint16_t *__restrict__ src, uint16_t *__restrict__ dst, long long total, int sw, int dw) {
  const long long i = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= total) return;
  const long long r = i / dw;
  const int c = static_cast<int>(i - r * dw);
  dst[i] = c < sw ? src[r * sw + c] : static_cast<uint16_t>(0);
}
}  // namespace
}  // namespace spx

using namespace spx;

extern "C" {

size_t spx_igemm_acc_bytes(int n_dst, int cout, int kv) {
  return kv > 32 ? align_up(static_cast<size_t>(n_dst > 0 ? n_dst : 1) * cout * sizeof(float), 256) : 0;
}

static int igemm_fwd_impl(const void *feat, const void *weight, void *out, const int32_t *pair,
                          const uint32_t *mask, const int32_t *argsort, int tile_order, int n_in, int n_out, int C,
                          int K, int kv, int dtype, int identity_k, const void *bias, int act,
                          float act_alpha, void *ws, size_t ws_bytes, spx_stream_t stream, float *stats,
                          const int32_t *n_live, int *slots_used_h) {
  if (slots_used_h) *slots_used_h = 0;
  SPX_CHECK(C > 0 && K > 0 && kv > 0 && n_in >= 0 && n_out >= 0, "bad sizes");
  if (n_out == 0) return 0;                                   // empty scene: nothing to write
  SPX_CHECK((feat || n_in == 0) && weight && out, "null tensor pointer");
  SPX_CHECK(pair || kv == 1, "pair table required");
  GemmParams p = fwd_params(feat, weight, out, pair, mask, argsort, bias, n_in, n_out, C, K, kv, identity_k);
  int dense_hint = 0, app_m = -1;
  apply_rows_layout(p, split_tile_order(tile_order, &dense_hint, &app_m));
  p.dense_hint = dense_hint;
  if (p.cls) p.app_m = app_m;
  p.act = act & 0xff;
  if (act & SPX_OUT_CACHED) p.dbg = 0x400;       // plain result stores: the next launch reads the rows
  p.act_alpha = act_alpha;
  // float64: its own kernel for every width, kernel volume and table form; no scratch, no statistics (*slots_used_h = 0)
  if (dtype == SPX_F64) return run_gather_gemm_f64(p, false, static_cast<hipStream_t>(stream));
  if (ws && ws_bytes >= spx_igemm_acc_bytes(n_out, K, kv) && kv > 32) p.acc = static_cast<float *>(ws);
  if (stats && kv <= 32 && !bias && p.act == SPX_ACT_NONE) {   // (the training-mode call: plain rows)
    p.stats = stats;
    p.n_live = n_live;
    p.grid_out = slots_used_h;
  }
  return run_gather_gemm(p, dtype, static_cast<hipStream_t>(stream));
}

int spx_igemm_fwd(const void *feat, const void *weight, void *out, const int32_t *pair,
                  const uint32_t *mask, const int32_t *argsort, int tile_order, int n_in, int n_out, int C,
                  int K, int kv, int dtype, int identity_k, const void *bias, int act,
                  float act_alpha, void *ws, size_t ws_bytes, spx_stream_t stream) {
  return igemm_fwd_impl(feat, weight, out, pair, mask, argsort, tile_order, n_in, n_out, C, K, kv, dtype, identity_k,
                        bias, act, act_alpha, ws, ws_bytes, stream, nullptr, nullptr, nullptr);
}

int spx_igemm_fwd_stats_slots(int n_out) {
  // upper bound of the workgroups of a forward launch over n_out rows: 64-row tiles + the appendix workgroups the
  // class rule allows (n / 4 rows) + slack
  return n_out <= 0 ? 0 : div_up(n_out, 64) + div_up(n_out, 256) + 8;
}

int spx_igemm_fwd_stats(const void *feat, const void *weight, void *out, const int32_t *pair,
                        const uint32_t *mask, const int32_t *argsort, int tile_order, int n_in, int n_out, int C,
                        int K, int kv, int dtype, int identity_k, const void *bias, int act,
                        float act_alpha, void *ws, size_t ws_bytes, float *stats, int stats_slots,
                        const int32_t *n_live, int *slots_used_h, spx_stream_t stream) {
  SPX_CHECK(slots_used_h, "slots_used_h is required");
  SPX_CHECK(!stats || stats_slots >= spx_igemm_fwd_stats_slots(n_out), "statistics buffer too small: %d slots < %d",
            stats_slots, spx_igemm_fwd_stats_slots(n_out));
  return igemm_fwd_impl(feat, weight, out, pair, mask, argsort, tile_order, n_in, n_out, C, K, kv, dtype, identity_k,
                        bias, act, act_alpha, ws, ws_bytes, stream, stats, n_live, slots_used_h);
}

int spx_igemm_fwd_int8(const void *feat, const void *weight, void *out, const int32_t *pair,
                       const uint32_t *mask, const int32_t *argsort, int n_in, int n_out, int C,
                       int K, int kv, int identity_k, const float *scale, const float *bias,
                       const void *add, float add_scale, int out_dtype, int act, float act_alpha,
                       spx_stream_t stream) {
  SPX_CHECK(C > 0 && K > 0 && kv > 0 && n_in >= 0 && n_out >= 0, "bad sizes");
  if (n_out == 0) return 0;                                   // empty scene: nothing to write
  SPX_CHECK((feat || n_in == 0) && weight && out, "null tensor pointer");
  SPX_CHECK(pair || kv == 1, "pair table required");
  // the reference has the same restriction (test/test_all_algo.py:376-377)
  SPX_CHECK(C % 16 == 0, "int8 needs in_channels %% 16 == 0, got %d", C);
  SPX_CHECK(K == 16 || K == 32 || K == 64 || K == 128 || K == 256 || wide_cout(K),
            "int8 supports out_channels 16/32/64/128/256 or a multiple of 128 beyond, got %d", K);
  SPX_CHECK(kv <= 32, "int8 supports kernel volumes up to 32, got %d", kv);
  SPX_CHECK(out_dtype == SPX_I8 || out_dtype == SPX_F16 || out_dtype == SPX_BF16 || out_dtype == SPX_F32,
            "bad output dtype %d", out_dtype);
  GemmParams p = fwd_params(feat, weight, out, pair, mask, argsort, bias, n_in, n_out, C, K, kv, identity_k);
  apply_rows_layout(p, (act & SPX_ROWS_LAYOUT_ACT) ? SPX_ROWS_LAYOUT : ((act & SPX_TILE_ORDER) ? 1 : 0));
  const bool hinted = p.cls && (act & SPX_SPARSE_HINT);   // the host has seen class word 1: a launch-shape hint
  if (hinted) p.app_rows = ((act >> 16) & 0xffff) * 64;   // ... and M (in units of 64 rows, 0 = not told)
  p.act = act & 0xff;
  p.act_alpha = act_alpha;
  p.scale = scale;
  p.add = add;
  p.add_scale = add_scale;
  p.out_dtype = out_dtype;
  const int oes = out_dtype == SPX_I8 ? 1 : (out_dtype == SPX_F32 ? 4 : 2);
  SPX_CHECK(v4_ok(p, 1, oes), "tensor too large for 32-bit buffer offsets");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // tile height by density class (igemm_i8.hip): tables in tile order or the host's sparse hint -> 64-row tiles
  return launch_gather_gemm_int8(p, p.tile_order || hinted, s);
}

size_t spx_igemm_dgrad_ws_bytes(int C, int K, int kv, int dtype) {
  (void)C; (void)K; (void)kv; (void)dtype;
  return 0;  // the weight transpose happens inside the kernel (LDS staging); kv > 32: spx_igemm_acc_bytes
}

int spx_igemm_dgrad(const void *dout, const void *weight, void *din, const int32_t *pair,
                    const uint32_t *mask, const int32_t *argsort, int tile_order, int n_out, int n_in, int C,
                    int K, int kv, int dtype, int subm, void *ws, size_t ws_bytes,
                    spx_stream_t stream) {
  if (n_in == 0) return 0;                                    // empty input: no gradient rows
  SPX_CHECK((dout || n_out == 0) && weight && din, "null tensor pointer");
  SPX_CHECK(pair || kv == 1, "pair table required");
  GemmParams p = dgrad_params(dout, weight, din, pair, mask, argsort, n_out, n_in, C, K, kv, subm);
  int dense_hint = 0, app_m = -1;
  apply_rows_layout(p, split_tile_order(tile_order, &dense_hint, &app_m));
  p.dense_hint = dense_hint;
  if (p.cls) p.app_m = app_m;
  if (dtype == SPX_F64) return run_gather_gemm_f64(p, true, static_cast<hipStream_t>(stream));
  if (ws && ws_bytes >= spx_igemm_acc_bytes(n_in, C, kv) && kv > 32) p.acc = static_cast<float *>(ws);
  return run_gather_gemm(p, dtype, static_cast<hipStream_t>(stream));
}

static int igemm_bwd_impl(const void *feat, const void *dout, const void *weight, void *din, void *dw,
                          const int32_t *pair, const uint32_t *mask, const int32_t *argsort, int tile_order,
                          const int32_t *pair_native, const int32_t *num_per_loc, const int32_t *plan,
                          int n_in, int n_out, int C, int K, int kv, int dtype, int subm, void *ws,
                          size_t ws_bytes, spx_stream_t stream, void *stage2_job) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_in == 0 || n_out == 0) {                              // empty scene: din empty / zero, dW zero
    SPX_CHECK(dw && C > 0 && K > 0 && kv > 0, "null tensor pointer");
    SPX_HIP(hipMemsetAsync(dw, 0, static_cast<size_t>(K) * kv * C * elem_bytes(dtype), s));
    if (n_in > 0) {
      SPX_CHECK(din, "null tensor pointer");
      SPX_HIP(hipMemsetAsync(din, 0, static_cast<size_t>(n_in) * C * elem_bytes(dtype), s));
    }
    return 0;
  }
  SPX_CHECK(feat && dout && weight && din && dw && ws, "null tensor pointer");
  SPX_CHECK(pair_native && num_per_loc, "Native pair lists and counts are required");
  SPX_CHECK(pair || kv == 1, "pair table required");
  if (dtype == SPX_F64) {                  // float64: the input gradient, then the weight gradient (no fused launch)
    SPX_CHECK(!stage2_job, "float64 backward has no deferred second stage (use spx_igemm_bwd)");
    SPX_CHECK(ws_bytes >= wgrad_f64_ws_bytes(n_in, C, K, kv),
              "workspace too small for the float64 weight gradient (spx_igemm_wgrad_ws_bytes_dtype)");
    if (spx_igemm_dgrad(dout, weight, din, pair, mask, argsort, tile_order, n_out, n_in, C, K, kv, dtype, subm,
                        nullptr, 0, stream))
      return -2;
    return wgrad_f64(feat, dout, dw, pair_native, num_per_loc, n_in, C, K, kv, subm, ws, ws_bytes, s);
  }
  SPX_CHECK(ws_bytes >= spx_igemm_wgrad_ws_bytes(n_in, C, K, kv), "workspace too small");
  GemmParams p = dgrad_params(dout, weight, din, pair, mask, argsort, n_out, n_in, C, K, kv, subm);
  int dense_hint = 0, app_m = -1;
  apply_rows_layout(p, split_tile_order(tile_order, &dense_hint, &app_m));
  p.dense_hint = dense_hint;
  if (p.cls) p.app_m = app_m;
  // dgrad + wgrad in one launch (settled A/B) where both halves have an MFMA kernel
  const int es = dtype == SPX_F32 ? 4 : 2, lanes = 16 / es;
  const bool fusable = (dtype == SPX_F16 || dtype == SPX_BF16 || dtype == SPX_F32) && C % lanes == 0 &&
                       K % lanes == 0 && mfma_ok(dtype, p.CIN, p.COUT, kv) && kv <= 32 && p.COUT <= 128 &&
                       v4_ok(p, es, es) && wgrad_rows_fit(n_in, n_out, C, K, es) && wgrad_lists_fit(n_in, kv) &&
                       n_in > 0 && n_out > 0;
  if (!fusable) {
    if (spx_igemm_dgrad(dout, weight, din, pair, mask, argsort, tile_order, n_out, n_in, C, K, kv, dtype, subm,
                        nullptr, 0, stream))
      return -2;
    return igemm_wgrad_impl(feat, dout, dw, pair_native, num_per_loc, plan, n_in, n_out, C, K, kv, dtype,
                            subm, ws, ws_bytes, stream, stage2_job);
  }
  plan = wgrad_plan_or_build(plan, num_per_loc, n_in, kv, subm, ws, ws_bytes, stream);
  if (!plan) return -2;
  const Wgrad2Params q = wgrad2_params(feat, dout, ws, pair_native, num_per_loc, plan, n_in, n_out, C, K, kv, subm);
  const int ntile = q.tiles_c * q.tiles_k;
  const int rc = dtype == SPX_F32 ? dispatch_bwd_f32(p, q, q.G * ntile, s)
                                  : (dtype == SPX_BF16 ? dispatch_bwd_bf16(p, q, q.G * ntile, s)
                                                       : dispatch_bwd<0>(p, q, q.G * ntile, s));
  if (rc) return rc;
  return launch_reduce2(q, dw, dtype, ntile, s, stage2_job);
}

int spx_igemm_bwd(const void *feat, const void *dout, const void *weight, void *din, void *dw,
                  const int32_t *pair, const uint32_t *mask, const int32_t *argsort, int tile_order,
                  const int32_t *pair_native, const int32_t *num_per_loc, const int32_t *plan,
                  int n_in, int n_out, int C, int K, int kv, int dtype, int subm, void *ws,
                  size_t ws_bytes, spx_stream_t stream) {
  return igemm_bwd_impl(feat, dout, weight, din, dw, pair, mask, argsort, tile_order, pair_native, num_per_loc, plan, n_in,
                        n_out, C, K, kv, dtype, subm, ws, ws_bytes, stream, nullptr);
}

int spx_igemm_bwd_deferred(const void *feat, const void *dout, const void *weight, void *din, void *dw,
                           const int32_t *pair, const uint32_t *mask, const int32_t *argsort, int tile_order,
                           const int32_t *pair_native, const int32_t *num_per_loc, const int32_t *plan,
                           int n_in, int n_out, int C, int K, int kv, int dtype, int subm, void *ws,
                           size_t ws_bytes, spx_stream_t stream, void *stage2_job) {
  SPX_CHECK(stage2_job, "stage2_job is required");
  SPX_CHECK(dtype != SPX_F64, "float64 backward has no deferred second stage (use spx_igemm_bwd)");
  memset(stage2_job, 0, SPX_STAGE2_JOB_BYTES);
  return igemm_bwd_impl(feat, dout, weight, din, dw, pair, mask, argsort, tile_order, pair_native, num_per_loc, plan, n_in,
                        n_out, C, K, kv, dtype, subm, ws, ws_bytes, stream, stage2_job);
}

int spx_bias_act_inplace(void *out, const void *bias, int n, int K, int dtype, int act,
                         float act_alpha, spx_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long total = static_cast<long long>(n) * K;
  if (total == 0) return 0;
  if (dtype == SPX_F64) return bias_act_f64(out, bias, n, K, act, act_alpha, s);
  const dim3 grid(static_cast<unsigned>((total + kThreads - 1) / kThreads));
  if (int rc = with_elem_type(dtype, [&](auto t, auto) {
        using T = decltype(t);
        hipLaunchKernelGGL(bias_act_kernel<T>, grid, dim3(kThreads), 0, s, static_cast<T *>(out),
                           static_cast<const T *>(bias), total, K, act, act_alpha);
      }))
    return rc;
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_pad_rows(const void *src, void *dst, long long rows, int src_row_bytes, int dst_row_bytes,
                 spx_stream_t stream) {
  SPX_CHECK(src_row_bytes > 0 && dst_row_bytes >= src_row_bytes && src_row_bytes % 2 == 0 && dst_row_bytes % 2 == 0,
            "row sizes must be even, destination rows at least as long as source rows");
  if (rows <= 0) return 0;
  SPX_CHECK(src && dst, "null tensor pointer");
  const long long total = rows * (dst_row_bytes / 2);
  hipLaunchKernelGGL(pad_rows_kernel, dim3(static_cast<unsigned>((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(src), static_cast<uint16_t *>(dst),
                     total, src_row_bytes / 2, dst_row_bytes / 2);
  SPX_LAUNCH_CHECK();
  return 0;
}

#ifdef SPX_TIMELINE
// debug builds only: copies the timeline table (8192 workgroups x 8 stamps, uint64) to host memory
int spx_debug_timeline(unsigned long long *dst_h) {
  SPX_HIP(hipDeviceSynchronize());
  SPX_HIP(hipMemcpyFromSymbol(dst_h, HIP_SYMBOL(g_timeline), sizeof(unsigned long long) * kTlMaxWg * kTlSlots));
  return 0;
}
#endif

}  // extern "C"
