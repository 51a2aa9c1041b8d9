// Kernel point convolution over a VoxelNeighbors table (spx_kpconv_fwd / _bwd): rigid KPConv with the linear influence
// and sum aggregation -- KPFCNN's convolution, the encoder of Predator, D3Feat and GeoTransformer.
//
//   h(m, s, k)  = valid(m, s) ? max(0, 1 - ||offsets[m, s] - kernel_points[k]|| / sigma) : 0             fp32
//   WF[m, k, :] = sum_s h(m, s, k) feats[rows[m, s], :]                                                  fp32 sum
//   out[m, :]   = (sum_k WF[m, k, :] @ weight[k]) * (normalize ? 1 / max(1, valid slots of m) : 1)
//
// Two small matrix products per query, both on v_mfma_f32_16x16x32: the 16 rows of a tile are the kernel points (K <=
// 16, padded with zero rows), the neighbour slots are the reduction axis of the first product, K * Cin that of the
// second.  No [M, S, Cin] and no [M, S, K] tensor exists in memory.
//
//   FORWARD     a workgroup of four waves owns TQ queries (32 while a channel block is <= 64 wide, 16 at 128: the WF
//               tile, TQ * 16 * block * 2 bytes, stays at 64 KB).  Cin above 128 walks in blocks of 128 that accumulate
//               into the same registers.
//     phase A   a wave takes the queries of the tile in turn.  A operand: h^T [16 kernel points x 32 slots], lane (k =
//               lane & 15, g = lane >> 4) computes the 8 slots 8 g .. 8 g + 7 of a step in fp32 and rounds them.  B
//               operand: lane (p = lane & 15, g) reads the 16-byte piece p (8 channels) of the rows of the same 8 slots
//               straight from feats -- 8 pieces in flight -- and turns the 8 x 8 block in its registers: column t of
//               the block is the B fragment of MFMA t, whose column p stands for channel 8 p + t.  Eight MFMAs cover 32
//               slots of 128 channels; their results, rounded once, leave as four 16-byte pieces per lane into the LDS
//               tile WF[query][k][piece ^ (query & mask)] (and into the [M, K, Cin] copy a backward reads).
//     phase B   out^T [Cout x TQ] = weight^T [Cout x (K * block)] @ WF^T: the A operand is the weight, pre-packed in
//               fragment order by a small launch (one coalesced 16-byte load per lane and MFMA, from L2), the B operand
//               a 16-byte LDS read; the waves split the 16-column blocks of Cout.  A lane ends up with 4 consecutive
//               output channels of one query: normalised, rounded once, one 8-byte store.
//   BACKWARD Q  the same tiles.  (d_out * norm), rounded, goes to LDS (and to the workspace for the weight side).  Per
//               channel c: dWF^T [16 kernel points x TQ] = weight[:, c, :] @ (d_out * norm)^T, the weight read in place
//               (its Cout axis is contiguous), into LDS as dWF[query][c][k].  Then per query and 16 slots dG^T [channels
//               x slots] = dWF^T @ h^T on v_mfma_f32_16x16x16 (the reduction axis is the 16 kernel points), h recomputed
//               from the offsets, two MFMAs whose rows are interleaved so that a lane holds 8 consecutive channels of a
//               slot: one 16-byte store into dG [M, S, Cin].  spx_group_bwd turns dG into dfeats.
//   BACKWARD W  dweight[(k, c), co] = sum_m WF[m, (k, c)] (d_out * norm)[m, co]: both operands are read as 16-byte pieces
//               of 8 queries per lane and turned in registers as in phase A; a workgroup owns 128 rows of K * Cin, 128
//               columns and a contiguous chunk of queries (its waves split the columns 8 p + t by t) and writes one
//               fp32 partial; a second launch adds the partials in chunk order and rounds once.
//
// Every table entry is range-checked before it addresses anything; loops are bounded by S, Cin, Cout or the chunk; no
// spin, grid barrier, cooperative launch, memset or atomic: identical run to run.
#include "igemm_defs.h"
#include "piece.h"

namespace spx {
namespace {

constexpr int kBlock = 256, kWaves = 4;
constexpr int kMaxSample = 128, kMaxPoints = 16, kMaxChannels = 256;
constexpr int kBlockC = 128;                      // channels of Cin a tile holds in LDS at a time
constexpr int kWgChunks = 32, kWgMinChunk = 256;  // weight side: at most that many query chunks of at least that size

struct KpArgs {
  const void *feats;                              // forward: the rows; backward: unused
  const int32_t *rows;
  const float *offsets, *kp;
  const void *weight;                             // forward: packed (pack_kernel); backward: [K, Cin, Cout]
  const void *dout;
  int M, S, n;
  const int32_t *n_queries, *n_live;
  int K, Cin, Cout;
  float sigma;
  int normalize;
  void *out;                                      // forward: out; backward: dG or NULL
  void *wf;                                       // forward: the [M, K, Cin] copy or NULL
  void *dy;                                       // backward: (d_out * norm) [M, Cout] for the weight side, or NULL
};

struct WgArgs {
  const void *wf, *dy;
  float *partial;                                 // [chunks][K * Cin][Cout]
  int M, KC, Cout, chunk;
  const int32_t *n_queries;
};

__device__ __forceinline__ int live_count(const int32_t *dev, int n) {
  const int live = dev ? min(*dev, n) : n;
  return live < 0 ? 0 : live;
}

__device__ __forceinline__ float influence(const float *__restrict__ o, float kx, float ky, float kz, float sigma) {
  const float dx = o[0] - kx, dy = o[1] - ky, dz = o[2] - kz;
  return fmaxf(0.f, 1.f - sqrtf(dx * dx + dy * dy + dz * dz) / sigma);
}

// column t of the 8 x 8 block of 16-bit elements a lane holds as 8 pieces: element j of the result is element t of x[j]
__device__ __forceinline__ uint4 column_of(const uint4 (&x)[8], int t) {
  const int d = t >> 1, sh = (t & 1) << 4;
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (dword_of4(x[j], d) >> sh) & 0xffffu;
  return make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

// v_mfma_f32_16x16x16: 4 reduction elements per lane and operand (4 g .. 4 g + 3)
template <bool BF16> __device__ __forceinline__ f32x4 mfma16k16(const uint2 &a, const uint2 &b, f32x4 c) {
  if constexpr (BF16) {
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
  } else {
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), c, 0, 0, 0);
  }
}

template <bool BF16> __device__ __forceinline__ uint32_t scale2(uint32_t v, float f) {
  return pack2<BF16>(to_float<BF16>(static_cast<uint16_t>(v)) * f, to_float<BF16>(static_cast<uint16_t>(v >> 16)) * f);
}

// 1 / max(1, valid slots) of the tile's queries (1 without normalize, and for a query that does not exist)
template <int TQ> __device__ __forceinline__ void tile_norms(float *snorm, const KpArgs &a, int m0, int nq, int live) {
  constexpr int LQ = kBlock / TQ;
  const int q = threadIdx.x / LQ, sub = threadIdx.x % LQ, m = m0 + q;
  int cnt = 0;
  if (a.normalize && m < nq)
    for (int s = sub; s < a.S; s += LQ)
      cnt += static_cast<unsigned>(a.rows[static_cast<long long>(m) * a.S + s]) < static_cast<unsigned>(live) ? 1 : 0;
#pragma unroll
  for (int o = LQ >> 1; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (sub == 0) snorm[q] = 1.f / static_cast<float>(max(cnt, 1));
}

// chunks of 32 reduction elements of a channel block of width cw
__host__ __device__ inline int block_chunks(int K, int cw) { return (K * cw + 31) >> 5; }

// The weight in the fragment order of phase B: piece ((chunk * NB + nb) * 64 + lane) of a channel block holds, for
// lane (r, g), weight[k][c0 + c .. c + 7][nb * 16 + r] with k * cw + c = chunk * 32 + 8 g; zeros beyond K.
__global__ void __launch_bounds__(kBlock)
kpconv_pack_kernel(const uint16_t *__restrict__ w, uint4 *__restrict__ wp, int K, int Cin, int Cout, int total) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int NB = Cout >> 4, lane = idx & 63, r = lane & 15, g = lane >> 4;
  int rest = idx >> 6, cb0 = 0, cw = min(kBlockC, Cin);
  for (; rest >= block_chunks(K, cw) * NB; cb0 += kBlockC, cw = min(kBlockC, Cin - cb0)) rest -= block_chunks(K, cw) * NB;
  const int ch = rest / NB, nb = rest - ch * NB;
  const int e = ch * 32 + 8 * g, k = e / cw, c = e - k * cw;
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    h[j] = k < K ? w[(static_cast<long long>(k) * Cin + cb0 + c + j) * Cout + nb * 16 + r] : 0u;
  wp[idx] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

template <bool BF16, int CBT>
__global__ void __launch_bounds__(kBlock)
kpconv_fwd_kernel(KpArgs a) {
  constexpr int TQ = CBT <= 64 ? 32 : 16, MB = TQ / 16, P = CBT / 8;
  __shared__ uint4 swf[TQ * 16 * P];              // WF[q][k][piece ^ (q & (P - 1))]
  __shared__ float snorm[TQ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * TQ;
  const int live = live_count(a.n_live, a.n), nq = live_count(a.n_queries, a.M);
  tile_norms<TQ>(snorm, a, m0, nq, live);
  const bool kok = ln < a.K;                      // this lane's row of the A operand: kernel point ln
  const float kx = kok ? a.kp[3 * ln] : 0.f, ky = kok ? a.kp[3 * ln + 1] : 0.f, kz = kok ? a.kp[3 * ln + 2] : 0.f;
  const uint16_t *feats = static_cast<const uint16_t *>(a.feats);
  const uint4 *wp = static_cast<const uint4 *>(a.weight);
  const int NB = a.Cout >> 4;
  f32x4 acc[4][MB];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[u][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int cb0 = 0; cb0 < a.Cin; cb0 += kBlockC) {
    const int cw = min(kBlockC, a.Cin - cb0);
    const bool pok = 8 * ln < cw;                 // this lane's piece of the block exists
    if (cb0) __syncthreads();
    // ---- phase A: WF of the tile's queries into LDS
    for (int q = wave; q < TQ; q += kWaves) {
      const int m = m0 + q;
      const long long e0 = static_cast<long long>(m) * a.S;
      f32x4 wf[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) wf[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (m < nq) {
        for (int s0 = 0; s0 < a.S; s0 += 32) {
          uint4 x[8];
          float hv[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {           // (the pieces of 8 slots in flight together)
            const int s = s0 + 8 * g + j;
            const int r = s < a.S ? a.rows[e0 + s] : -1;
            const bool ok = static_cast<unsigned>(r) < static_cast<unsigned>(live);
            x[j] = make_uint4(0u, 0u, 0u, 0u);
            hv[j] = 0.f;
            if (ok && pok) x[j] = *reinterpret_cast<const uint4 *>(feats + static_cast<long long>(r) * a.Cin + cb0 + 8 * ln);
            if (ok && kok) hv[j] = influence(a.offsets + (e0 + s) * 3, kx, ky, kz, a.sigma);
          }
          const uint4 hf = make_uint4(pack2<BF16>(hv[0], hv[1]), pack2<BF16>(hv[2], hv[3]), pack2<BF16>(hv[4], hv[5]),
                                      pack2<BF16>(hv[6], hv[7]));
#pragma unroll
          for (int t = 0; t < 8; ++t) wf[t] = mfma16<BF16>(hf, column_of(x, t), wf[t]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {               // (kernel point 4 g + i, channels 8 ln .. 8 ln + 7: rounded once)
        const int k = 4 * g + i;
        const uint4 piece = make_uint4(pack2<BF16>(wf[0][i], wf[1][i]), pack2<BF16>(wf[2][i], wf[3][i]),
                                       pack2<BF16>(wf[4][i], wf[5][i]), pack2<BF16>(wf[6][i], wf[7][i]));
        if (ln < P) swf[(q * 16 + k) * P + (ln ^ (q & (P - 1)))] = piece;
        if (a.wf && m < a.M && k < a.K && pok)
          *reinterpret_cast<uint4 *>(static_cast<uint16_t *>(a.wf) + (static_cast<long long>(m) * a.K + k) * a.Cin + cb0 +
                                     8 * ln) = piece;
      }
    }
    __syncthreads();
    // ---- phase B: out^T += weight^T @ WF^T over the block's K * cw reduction elements
    const int nch = block_chunks(a.K, cw);
    int kk = 0, cc = 8 * g;                       // this lane's 8 elements of a chunk: kernel point kk, channels cc ..
    while (cc >= cw) cc -= cw, ++kk;
#pragma unroll 2
    for (int ch = 0; ch < nch; ++ch) {
      uint4 bq[MB];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const int q = mb * 16 + ln;
        bq[mb] = swf[(q * 16 + kk) * P + ((cc >> 3) ^ (q & (P - 1)))];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int nb = wave + kWaves * u;
        if (nb < NB) {
          const uint4 wa = wp[((ch * NB + nb) << 6) + lane];
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) acc[u][mb] = mfma16<BF16>(wa, bq[mb], acc[u][mb]);
        }
      }
      cc += 32;
      while (cc >= cw) cc -= cw, ++kk;
    }
    wp += (nch * NB) << 6;
  }
  // ---- epilogue: query mb * 16 + ln, channels nb * 16 + 4 g .. + 3
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int nb = wave + kWaves * u;
    if (nb >= NB) continue;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int q = mb * 16 + ln, m = m0 + q;
      if (m >= a.M) continue;
      const float f = snorm[q];
      const uint2 o = make_uint2(pack2<BF16>(acc[u][mb][0] * f, acc[u][mb][1] * f),
                                 pack2<BF16>(acc[u][mb][2] * f, acc[u][mb][3] * f));
      *reinterpret_cast<uint2 *>(static_cast<uint16_t *>(a.out) + static_cast<long long>(m) * a.Cout + nb * 16 + 4 * g) = o;
    }
  }
}

template <bool BF16, int CBT>
__global__ void __launch_bounds__(kBlock)
kpconv_bwd_query_kernel(KpArgs a) {
  constexpr int TQ = CBT <= 64 ? 32 : 16, MB = TQ / 16;
  __shared__ uint2 sdwf[TQ * CBT * 4];            // dWF[q][c][k]: 16 kernel points = 4 pieces of 8 bytes
  __shared__ uint4 sdy[TQ * (kMaxChannels / 8)];  // (d_out * norm)[q][piece ^ (q & 3)], Cout padded to 32 with zeros
  float *snorm = reinterpret_cast<float *>(sdwf);  // (read before the first dWF is written: two tiles of 80 KB fit a CU)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * TQ;
  const int live = live_count(a.n_live, a.n), nq = live_count(a.n_queries, a.M);
  const int PC = ((a.Cout + 31) >> 5) << 2;       // pieces of a padded d_out row
  tile_norms<TQ>(snorm, a, m0, nq, live);
  __syncthreads();
  for (int i = threadIdx.x; i < TQ * PC; i += kBlock) {
    const int q = i / PC, p = i - q * PC, m = m0 + q;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    const bool col = 8 * p < a.Cout;
    if (m < nq && col) {
      v = *reinterpret_cast<const uint4 *>(static_cast<const uint16_t *>(a.dout) + static_cast<long long>(m) * a.Cout + 8 * p);
      if (a.normalize) {
        const float f = snorm[q];
        v = make_uint4(scale2<BF16>(v.x, f), scale2<BF16>(v.y, f), scale2<BF16>(v.z, f), scale2<BF16>(v.w, f));
      }
    }
    sdy[q * PC + (p ^ (q & 3))] = v;
    if (a.dy && m < a.M && col)
      *reinterpret_cast<uint4 *>(static_cast<uint16_t *>(a.dy) + static_cast<long long>(m) * a.Cout + 8 * p) = v;
  }
  if (!a.out) return;                             // (the weight side alone: only d_out * norm was wanted)
  float kp[4][3];                                 // the kernel points 4 g .. 4 g + 3: this lane's elements of h^T
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int d = 0; d < 3; ++d) kp[j][d] = 4 * g + j < a.K ? a.kp[3 * (4 * g + j) + d] : 0.f;
  const uint16_t *w = static_cast<const uint16_t *>(a.weight);
  uint16_t *dg = static_cast<uint16_t *>(a.out);
  for (int cb0 = 0; cb0 < a.Cin; cb0 += kBlockC) {
    const int cw = min(kBlockC, a.Cin - cb0);
    __syncthreads();
    // ---- dWF^T [16 x TQ] of channel c = weight[:, c, :] @ (d_out * norm)^T, four channels at a time
    for (int c0 = wave * 4; c0 < cw; c0 += 4 * kWaves) {
      f32x4 acc[4][MB];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[u][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int co = 0; co < a.Cout; co += 32) {
        uint4 bq[MB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          const int q = mb * 16 + ln;
          bq[mb] = sdy[q * PC + (((co >> 3) + g) ^ (q & 3))];
        }
        const bool wok = ln < a.K && co + 8 * g < a.Cout;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          uint4 wa = make_uint4(0u, 0u, 0u, 0u);
          if (wok) wa = *reinterpret_cast<const uint4 *>(w + (static_cast<long long>(ln) * a.Cin + cb0 + c0 + u) * a.Cout + co + 8 * g);
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) acc[u][mb] = mfma16<BF16>(wa, bq[mb], acc[u][mb]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)           // (query mb * 16 + ln, kernel points 4 g .. 4 g + 3: rounded once)
          sdwf[((mb * 16 + ln) * CBT + c0 + u) * 4 + g] = make_uint2(pack2<BF16>(acc[u][mb][0], acc[u][mb][1]),
                                                                     pack2<BF16>(acc[u][mb][2], acc[u][mb][3]));
    }
    __syncthreads();
    // ---- dG^T [channels x 16 slots] = dWF^T @ h^T per query
    for (int q = wave; q < TQ; q += kWaves) {
      const int m = m0 + q;
      if (m >= a.M) break;
      const long long e0 = static_cast<long long>(m) * a.S;
      for (int s0 = 0; s0 < a.S; s0 += 16) {
        const int s = s0 + ln;
        const int r = (s < a.S && m < nq) ? a.rows[e0 + s] : -1;
        float h[4] = {0.f, 0.f, 0.f, 0.f};
        if (static_cast<unsigned>(r) < static_cast<unsigned>(live)) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * g + j < a.K) h[j] = influence(a.offsets + (e0 + s) * 3, kp[j][0], kp[j][1], kp[j][2], a.sigma);
        }
        const uint2 hf = make_uint2(pack2<BF16>(h[0], h[1]), pack2<BF16>(h[2], h[3]));
        for (int cp = 0; cp < cw; cp += 32) {
          f32x4 d[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {           // (row r of MFMA u is channel cp + 8 (r / 4) + 4 u + r % 4)
            const int c = cp + 8 * (ln >> 2) + 4 * u + (ln & 3);
            const uint2 av = c < cw ? sdwf[(q * CBT + c) * 4 + g] : make_uint2(0u, 0u);
            d[u] = mfma16k16<BF16>(av, hf, f32x4{0.f, 0.f, 0.f, 0.f});
          }
          if (s < a.S && cp + 8 * g < cw)
            *reinterpret_cast<uint4 *>(dg + (e0 + s) * a.Cin + cb0 + cp + 8 * g) =
                make_uint4(pack2<BF16>(d[0][0], d[0][1]), pack2<BF16>(d[0][2], d[0][3]), pack2<BF16>(d[1][0], d[1][1]),
                           pack2<BF16>(d[1][2], d[1][3]));
        }
      }
    }
  }
}

template <bool BF16>
__global__ void __launch_bounds__(kBlock)
kpconv_wgrad_kernel(WgArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 15, g = lane >> 4;
  const int nq = live_count(a.n_queries, a.M);
  const int pa = blockIdx.x * 16 + ln, pb = blockIdx.y * 16 + ln;       // this lane's piece of a WF row / a d_out row
  const bool aok = 8 * pa < a.KC, bok = 8 * pb < a.Cout;
  const int mbeg = min(static_cast<int>(blockIdx.z) * a.chunk, nq), mend = min(mbeg + a.chunk, nq);
  const uint16_t *wf = static_cast<const uint16_t *>(a.wf), *dy = static_cast<const uint16_t *>(a.dy);
  f32x4 acc[8][2];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int m1 = mbeg; m1 < mend; m1 += 32) {
    uint4 xa[8], xb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int m = m1 + 8 * g + j;
      xa[j] = xb[j] = make_uint4(0u, 0u, 0u, 0u);
      if (m < mend && aok) xa[j] = *reinterpret_cast<const uint4 *>(wf + static_cast<long long>(m) * a.KC + 8 * pa);
      if (m < mend && bok) xb[j] = *reinterpret_cast<const uint4 *>(dy + static_cast<long long>(m) * a.Cout + 8 * pb);
    }
    const uint4 yb0 = column_of(xb, 2 * wave), yb1 = column_of(xb, 2 * wave + 1);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const uint4 ya = column_of(xa, t);
      acc[t][0] = mfma16<BF16>(ya, yb0, acc[t][0]);
      acc[t][1] = mfma16<BF16>(ya, yb1, acc[t][1]);
    }
  }
  if (!bok) return;
  float *part = a.partial + static_cast<size_t>(blockIdx.z) * a.KC * a.Cout;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {                 // (row 8 (piece 4 g + i of the block) + t, columns 8 pb + 2 wave, + 1)
      const int row = 8 * (blockIdx.x * 16 + 4 * g + i) + t;
      if (row < a.KC)
        *reinterpret_cast<float2 *>(part + static_cast<size_t>(row) * a.Cout + 8 * pb + 2 * wave) =
            make_float2(acc[t][0][i], acc[t][1][i]);
    }
}

template <bool BF16>
__global__ void __launch_bounds__(kBlock)
kpconv_wgrad_sum_kernel(const float *__restrict__ partial, int chunks, int total, uint16_t *__restrict__ dw) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += partial[static_cast<size_t>(c) * total + i];      // (chunk order: fixed)
  dw[i] = from_float<BF16>(s);
}

// ------------------------------------------------------------------------------------------------ host side

int check_shape(int M, int S, int n, int K, int Cin, int Cout, int dtype) {
  SPX_CHECK(dtype == SPX_F16 || dtype == SPX_BF16, "dtype must be f16 or bf16, got %d", dtype);
  SPX_CHECK(K >= 1 && K <= kMaxPoints, "K must be in 1 .. %d, got %d", kMaxPoints, K);
  SPX_CHECK(Cin >= 16 && Cin <= kMaxChannels && Cin % 16 == 0, "Cin must be a multiple of 16 in 16 .. %d, got %d",
            kMaxChannels, Cin);
  SPX_CHECK(Cout >= 16 && Cout <= kMaxChannels && Cout % 16 == 0, "Cout must be a multiple of 16 in 16 .. %d, got %d",
            kMaxChannels, Cout);
  SPX_CHECK(M >= 0 && n >= 0, "bad query / row counts %d / %d", M, n);
  SPX_CHECK(S >= 1 && S <= kMaxSample, "nsample must be in 1 .. %d, got %d", kMaxSample, S);
  SPX_CHECK(static_cast<long long>(M) * S * 3 < 0x80000000LL, "M * nsample * 3 must stay below 2^31, got %d x %d", M, S);
  return 0;
}

size_t packed_pieces(int K, int Cin, int Cout) {
  size_t chunks = 0;
  for (int cb0 = 0; cb0 < Cin; cb0 += kBlockC) chunks += block_chunks(K, Cin - cb0 < kBlockC ? Cin - cb0 : kBlockC);
  return chunks * (Cout >> 4) * 64;
}

// the weight side's split of the queries: host-known sizes only
void wgrad_split(int M, int *chunks, int *chunk) {
  int c = (M + kWgMinChunk - 1) / kWgMinChunk;
  c = c < 1 ? 1 : (c > kWgChunks ? kWgChunks : c);
  *chunk = (((M + c - 1) / c + 31) & ~31);
  if (*chunk < 32) *chunk = 32;
  *chunks = c;
}

size_t dy_bytes(int M, int Cout) { return align_up(static_cast<size_t>(M) * Cout * 2, 256); }

// f(cbt): the instance of the channel block's LDS width, the power of two that holds min(Cin, 128)
template <typename F> void dispatch_block(int Cin, F &&f) {
  const int cw = Cin < kBlockC ? Cin : kBlockC;
  dispatch_value<16, 32, 64, 128>(cw <= 16 ? 16 : (cw <= 32 ? 32 : (cw <= 64 ? 64 : 128)), f);
}

}  // namespace
}  // namespace spx

extern "C" {

size_t spx_kpconv_ws_bytes(int M, int K, int Cin, int Cout, int backward) {
  using namespace spx;
  if (M < 0 || K < 1 || K > kMaxPoints || Cin < 16 || Cin > kMaxChannels || Cin % 16 || Cout < 16 || Cout > kMaxChannels ||
      Cout % 16)
    return 0;
  if (!backward) return align_up(packed_pieces(K, Cin, Cout) * 16, 256);
  int chunks, chunk;
  wgrad_split(M, &chunks, &chunk);
  return dy_bytes(M, Cout) + align_up(static_cast<size_t>(chunks) * K * Cin * Cout * sizeof(float), 256);
}

int spx_kpconv_fwd(const void *feats, const int32_t *rows, const float *offsets, const float *kernel_points,
                   const void *weight, int M, int S, int n, const int32_t *n_queries, const int32_t *n_live, int K, int Cin,
                   int Cout, int dtype, float sigma, int normalize, void *out, void *wf, void *ws, size_t ws_bytes,
                   spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_shape(M, S, n, K, Cin, Cout, dtype)) return rc;
  SPX_CHECK(sigma > 0.f, "sigma must be > 0, got %g", static_cast<double>(sigma));
  if (M == 0) return 0;
  SPX_CHECK(rows && offsets && kernel_points && weight && out && ws && (n == 0 || feats),
            "feats / rows / offsets / kernel_points / weight / out / ws is NULL");
  SPX_CHECK(aligned_to(feats, 16) && aligned_to(weight, 16) && aligned_to(out, 16) && aligned_to(wf, 16) &&
            aligned_to(ws, 16) && aligned_to(rows, 4) && aligned_to(offsets, 4) && aligned_to(kernel_points, 4),
            "rows must be aligned to 16 bytes, tables to their elements");
  const size_t pieces = packed_pieces(K, Cin, Cout);
  SPX_CHECK(ws_bytes >= pieces * 16, "workspace too small: %zu < %zu bytes", ws_bytes, pieces * 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kpconv_pack_kernel, dim3(static_cast<unsigned>((pieces + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     static_cast<const uint16_t *>(weight), static_cast<uint4 *>(ws), K, Cin, Cout, static_cast<int>(pieces));
  SPX_LAUNCH_CHECK();
  KpArgs a = {};
  a.feats = feats, a.rows = rows, a.offsets = offsets, a.kp = kernel_points, a.weight = ws, a.M = M, a.S = S, a.n = n;
  a.n_queries = n_queries, a.n_live = n_live, a.K = K, a.Cin = Cin, a.Cout = Cout, a.sigma = sigma;
  a.normalize = normalize ? 1 : 0, a.out = out, a.wf = wf;
  dispatch_block(Cin, [&](auto cbt) {
    constexpr int TQ = decltype(cbt)::value <= 64 ? 32 : 16;
    const dim3 grid((M + TQ - 1) / TQ);
    if (dtype == SPX_BF16) hipLaunchKernelGGL((kpconv_fwd_kernel<true, cbt>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((kpconv_fwd_kernel<false, cbt>), grid, dim3(kBlock), 0, s, a);
  });
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_kpconv_bwd(const void *wf, const int32_t *rows, const float *offsets, const float *kernel_points,
                   const void *weight, const void *d_out, int M, int S, int n, const int32_t *n_queries,
                   const int32_t *n_live, int K, int Cin, int Cout, int dtype, float sigma, int normalize, void *dg,
                   void *dweight, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_shape(M, S, n, K, Cin, Cout, dtype)) return rc;
  SPX_CHECK(sigma > 0.f, "sigma must be > 0, got %g", static_cast<double>(sigma));
  if (M == 0 || (!dg && !dweight)) return 0;
  SPX_CHECK(rows && offsets && kernel_points && weight && d_out, "rows / offsets / kernel_points / weight / d_out is NULL");
  SPX_CHECK(aligned_to(wf, 16) && aligned_to(weight, 16) && aligned_to(d_out, 16) && aligned_to(dg, 16) &&
            aligned_to(dweight, 16) && aligned_to(ws, 16) && aligned_to(rows, 4) && aligned_to(offsets, 4) &&
            aligned_to(kernel_points, 4), "rows must be aligned to 16 bytes, tables to their elements");
  int chunks, chunk;
  wgrad_split(M, &chunks, &chunk);
  const bool scaled = dweight && normalize;       // the weight side reads d_out * norm from the workspace
  if (dweight) {
    SPX_CHECK(wf && ws, "wf / ws is NULL");
    SPX_CHECK(ws_bytes >= spx_kpconv_ws_bytes(M, K, Cin, Cout, 1), "workspace too small: %zu < %zu bytes", ws_bytes,
              spx_kpconv_ws_bytes(M, K, Cin, Cout, 1));
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool bf16 = dtype == SPX_BF16;
  if (dg || scaled) {
    KpArgs a = {};
    a.rows = rows, a.offsets = offsets, a.kp = kernel_points, a.weight = weight, a.dout = d_out, a.M = M, a.S = S, a.n = n;
    a.n_queries = n_queries, a.n_live = n_live, a.K = K, a.Cin = Cin, a.Cout = Cout, a.sigma = sigma;
    a.normalize = normalize ? 1 : 0, a.out = dg, a.dy = scaled ? ws : nullptr;
    dispatch_block(Cin, [&](auto cbt) {
      constexpr int TQ = decltype(cbt)::value <= 64 ? 32 : 16;
      const dim3 grid((M + TQ - 1) / TQ);
      if (bf16) hipLaunchKernelGGL((kpconv_bwd_query_kernel<true, cbt>), grid, dim3(kBlock), 0, s, a);
      else hipLaunchKernelGGL((kpconv_bwd_query_kernel<false, cbt>), grid, dim3(kBlock), 0, s, a);
    });
    SPX_LAUNCH_CHECK();
  }
  if (dweight) {
    const int KC = K * Cin, total = KC * Cout;
    float *partial = reinterpret_cast<float *>(static_cast<char *>(ws) + dy_bytes(M, Cout));
    const WgArgs q = {wf, scaled ? ws : d_out, partial, M, KC, Cout, chunk, n_queries};
    const dim3 grid((KC / 8 + 15) / 16, (Cout / 8 + 15) / 16, chunks);
    if (bf16) hipLaunchKernelGGL(kpconv_wgrad_kernel<true>, grid, dim3(kBlock), 0, s, q);
    else hipLaunchKernelGGL(kpconv_wgrad_kernel<false>, grid, dim3(kBlock), 0, s, q);
    SPX_LAUNCH_CHECK();
    const dim3 sgrid((total + kBlock - 1) / kBlock);
    uint16_t *dw = static_cast<uint16_t *>(dweight);
    if (bf16) hipLaunchKernelGGL(kpconv_wgrad_sum_kernel<true>, sgrid, dim3(kBlock), 0, s, partial, chunks, total, dw);
    else hipLaunchKernelGGL(kpconv_wgrad_sum_kernel<false>, sgrid, dim3(kBlock), 0, s, partial, chunks, total, dw);
    SPX_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
