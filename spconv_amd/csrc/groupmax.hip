// Fused set abstraction over a VoxelNeighbors table (spx_group_linear_max_fwd / _bwd): the grouped linear layer and the
// max over the samples of PointNet++'s SA layer, pointnet2_stack's StackSAModuleMSG and Voxel R-CNN's grouped MLP.
//
//   x[m, s, c] = feats[rows[m, s], c] + sum_d offsets[m, s, d] pos_weight[d, c] + in_bias[c]     fp32, ReLU, rounded once
//   y[m, s, :] = x[m, s, :] @ weight                                                             fp32 sum
//   out[m, co] = max over the valid slots of y[m, s, co], arg[m, co] = the LOWEST slot that attains it
//
// No [M, S, Cin] tensor exists in the forward; the backward keeps arg (M x Cout bytes) and recomputes x from the table.
// Every product runs on v_mfma_f32_16x16x32.  COLUMN BLOCKS: a wave works on NCB blocks of 16 slots at a time (4 while
// the reduction axis is <= 128 wide, 2 beyond: the B fragments of a pass, NCB x steps x 4 VGPRs, stay at 64 registers).
// With cbq = ceil(S / 16) blocks per query a pass holds max(1, NCB / cbq) whole queries (S <= 16: four queries), or one
// chunk of a query whose slots do not fit (S > 16 NCB); every A fragment read from LDS meets NCB MFMAs.
//
//   FORWARD     y^T [Cout x slots] = weight^T @ x^T.  The weight, pre-packed in fragment order by a small launch, is
//               copied into LDS once per workgroup; workgroups are persistent and their waves stride over the passes, with
//               no barrier behind the copy.  B operand: lane (n = lane & 15, g = lane >> 4) loads the 16-byte piece g of a
//               32-channel step of row rows[m, s0 + n], adds the position and bias terms in fp32 (pos_weight / in_bias
//               from LDS), applies the ReLU and rounds: no register transpose.  The wave walks the 16-wide blocks of
//               Cout; an accumulator lane holds 4 channels of ONE slot: invalid slots never enter, a strictly greater
//               value wins across the blocks of a query (lowest slot on ties), then the value goes through a DPP
//               butterfly of maxima over the 16 lanes of the row and the slot through one of minima over the lanes that
//               hold the maximum.  A query in chunks keeps its running (max, slot) in a wave-private LDS row.
//   BACKWARD Q  dX^T [Cin x slots] = weight @ dY^T, the same passes.  The weight goes into LDS in fragment order while
//               it is copied (its Cout axis is contiguous: no pack launch).  The B fragment dY^T is built in registers:
//               8 values of d_out and 8 bytes of arg per lane, kept where arg names the lane's slot.  The ReLU mask comes
//               from the fp32 x recomputed for the lane's 4 channels; the fp32 dX feeds the [4, Cin] position / bias sums
//               (a DPP row sum, then a wave-private LDS row; per workgroup one partial, in wave order) and is rounded
//               into dG [M, S, Cin] as 8-byte stores.  spx_group_bwd turns dG into dfeats.
//   BACKWARD W  dweight [Cin x Cout] = x^T dY over the flat entries e = m * S + s of a host-known chunk of queries: a
//               workgroup owns 128 channels, 64 columns and a chunk; its waves split the entries, 32 per step.  x is
//               gathered and recomputed as 8 pieces per lane and turned in registers (column t of the 8 x 8 block is the
//               A fragment of MFMA t), dY is built per lane from d_out and arg.  The four waves add their accumulators
//               in wave order through one LDS tile; a second launch adds the partials in chunk order, and the [4, Cin]
//               partials of the query side in workgroup order.
//
// Every table entry is range-checked before it addresses anything; loops are bounded by host-known sizes; no spin, grid
// barrier, cooperative launch, memset or atomic: identical run to run.
#include <atomic>

#include "igemm_defs.h"
#include "piece.h"

namespace spx {
namespace {

constexpr int kBlock = 256, kWaves = 4;
constexpr int kMaxSample = 128, kMaxChannels = 256;
constexpr int kCUs = 256, kLdsBytes = 160 * 1024;
constexpr int kWgChunks = 256, kWgMinChunk = 64;  // weight side: at most that many query chunks of at least that size
constexpr int kWgPartial = 1 << 22;               // ... and at most that many fp32 elements of partials (16 MB)
constexpr float kNegInf = -__builtin_inff();

struct GmArgs {
  const void *feats;
  const int32_t *rows;
  const float *offsets, *pos, *bias;              // pos_weight / in_bias: each may be NULL; offsets: NULL without pos_weight
  const void *weight;                             // forward: packed (pack_kernel); backward: [Cin, Cout]
  const void *dout;
  const uint8_t *argin;                           // backward: arg of the forward
  int M, S, n;
  const int32_t *n_queries, *n_live;
  int Cin, Cout, relu;
  void *out;                                      // forward: out; backward: dG or NULL
  uint8_t *arg;                                   // forward: arg or NULL
  float *ppart;                                   // backward: [grid][4][Cin] or NULL
  float *partial;                                 // weight side: [chunks][Cin][Cout]
  int chunk;
};

__device__ __forceinline__ int live_count(const int32_t *dev, int n) {
  const int live = dev ? min(*dev, n) : n;
  return live < 0 ? 0 : live;
}

// how NCB column blocks of 16 slots map to queries: GL blocks per query and pass, QP queries per pass, NCH passes per
// query (QP == 1 whenever NCH > 1)
struct Pass {
  int GL, QP, NCH;
};
__host__ __device__ inline Pass pass_of(int S, int NCB) {
  const int cbq = (S + 15) >> 4;
  Pass p;
  p.GL = cbq < NCB ? cbq : NCB;
  p.QP = cbq <= NCB ? NCB / cbq : 1;
  p.NCH = (cbq + NCB - 1) / NCB;
  return p;
}

// the fp32 pre-activation: one expression for the three kernels that compute it (their ReLU masks are the same set)
__device__ __forceinline__ float xval(float f, const float (&o)[3], float p0, float p1, float p2, float b) {
  return f + fmaf(o[0], p0, fmaf(o[1], p1, fmaf(o[2], p2, b)));
}

// pos_weight / in_bias as [4][Cin] fp32 in LDS (zeros for a missing one)
__device__ __forceinline__ void load_table(float *stab, const GmArgs &a) {
  for (int i = threadIdx.x; i < 4 * a.Cin; i += kBlock) {
    const int d = i / a.Cin, c = i - d * a.Cin;
    stab[i] = d < 3 ? (a.pos ? a.pos[d * a.Cin + c] : 0.f) : (a.bias ? a.bias[c] : 0.f);
  }
}

// x of the 8 channels c0 .. c0 + 7 of a row piece, rounded once
template <bool BF16>
__device__ __forceinline__ uint4 x_piece(const uint4 &raw, const float *stab, int Cin, int c0, const float (&o)[3], bool relu) {
  float p[4][8];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const float4 lo = *reinterpret_cast<const float4 *>(stab + d * Cin + c0);
    const float4 hi = *reinterpret_cast<const float4 *>(stab + d * Cin + c0 + 4);
    p[d][0] = lo.x, p[d][1] = lo.y, p[d][2] = lo.z, p[d][3] = lo.w, p[d][4] = hi.x, p[d][5] = hi.y, p[d][6] = hi.z, p[d][7] = hi.w;
  }
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t v = dword_of4(raw, k);
    float x0 = xval(to_float<BF16>(static_cast<uint16_t>(v)), o, p[0][2 * k], p[1][2 * k], p[2][2 * k], p[3][2 * k]);
    float x1 = xval(to_float<BF16>(static_cast<uint16_t>(v >> 16)), o, p[0][2 * k + 1], p[1][2 * k + 1], p[2][2 * k + 1],
                    p[3][2 * k + 1]);
    if (relu) x0 = fmaxf(x0, 0.f), x1 = fmaxf(x1, 0.f);
    w[k] = pack2<BF16>(x0, x1);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int CTRL> __device__ __forceinline__ int dpp_move(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
// maximum / minimum over the 16 lanes of a DPP row, in every lane: lane ^ 1, lane ^ 2 (quad permutes), then the mirrored
// half row and the mirrored row
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, __builtin_bit_cast(float, dpp_move<0xB1>(__builtin_bit_cast(int, v))));
  v = fmaxf(v, __builtin_bit_cast(float, dpp_move<0x4E>(__builtin_bit_cast(int, v))));
  v = fmaxf(v, __builtin_bit_cast(float, dpp_move<0x141>(__builtin_bit_cast(int, v))));
  return fmaxf(v, __builtin_bit_cast(float, dpp_move<0x140>(__builtin_bit_cast(int, v))));
}
__device__ __forceinline__ int row16_min(int v) {
  v = min(v, dpp_move<0xB1>(v));
  v = min(v, dpp_move<0x4E>(v));
  v = min(v, dpp_move<0x141>(v));
  return min(v, dpp_move<0x140>(v));
}

// column t of the 8 x 8 block of 16-bit elements a lane holds as 8 pieces: element j of the result is element t of x[j]
__device__ __forceinline__ uint4 column_of(const uint4 (&x)[8], int t) {
  const int d = t >> 1, sh = (t & 1) << 4;
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (dword_of4(x[j], d) >> sh) & 0xffffu;
  return make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

// The weight in the fragment order of the forward: piece ((kc * NB + nb) * 64 + lane) holds, for lane (r, g),
// weight[kc * 32 + 8 g .. + 7][nb * 16 + r]; zeros beyond Cin.
__global__ void __launch_bounds__(kBlock)
groupmax_pack_kernel(const uint16_t *__restrict__ w, uint4 *__restrict__ wp, int Cin, int Cout, int total) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int NB = Cout >> 4, lane = idx & 63, r = lane & 15, g = lane >> 4;
  const int kc = (idx >> 6) / NB, nb = (idx >> 6) - kc * NB, c = kc * 32 + 8 * g;
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = c + j < Cin ? w[static_cast<long long>(c + j) * Cout + nb * 16 + r] : 0u;
  wp[idx] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

// KCT: the 32-channel steps of Cin an instance holds (Cin <= 32 KCT)
template <bool BF16, int KCT>
__global__ void __launch_bounds__(kBlock)
groupmax_fwd_kernel(GmArgs a) {
  constexpr int NCB = KCT <= 4 ? 4 : 2;
  extern __shared__ uint4 smem[];
  const int KC = (a.Cin + 31) >> 5, NB = a.Cout >> 4;
  uint4 *sw = smem;                                                     // the packed weight: KC * NB * 64 pieces
  float *stab = reinterpret_cast<float *>(sw + KC * NB * 64);           // [4][Cin]
  float *srun = stab + 4 * a.Cin;                                       // [waves][Cout] running maxima of a query in chunks
  int *sslot = reinterpret_cast<int *>(srun + kWaves * a.Cout);         // [waves][Cout] ... and their slots
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 15, g = lane >> 4;
  const int live = live_count(a.n_live, a.n), nq = live_count(a.n_queries, a.M);
  for (int i = threadIdx.x; i < KC * NB * 64; i += kBlock) sw[i] = static_cast<const uint4 *>(a.weight)[i];
  load_table(stab, a);
  __syncthreads();
  const bool plain = !a.pos && !a.bias && !a.relu;                      // x is the row itself
  const Pass ps = pass_of(a.S, NCB);
  const int units = (a.M + ps.QP - 1) / ps.QP;
  const uint16_t *feats = static_cast<const uint16_t *>(a.feats);
  srun += wave * a.Cout, sslot += wave * a.Cout;
  for (int u = blockIdx.x * kWaves + wave; u < units; u += gridDim.x * kWaves) {
    for (int ch = 0; ch < ps.NCH; ++ch) {
      // ---- the B fragments of the pass: gathered once
      uint4 B[NCB][KCT];
      bool ok[NCB];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const int qi = cb / ps.GL, m = u * ps.QP + qi, sl = (ch * NCB + cb - qi * ps.GL) * 16 + ln;
        int r = -1;
        if (qi < ps.QP && m < nq && sl < a.S) r = a.rows[static_cast<long long>(m) * a.S + sl];
        ok[cb] = static_cast<unsigned>(r) < static_cast<unsigned>(live);
        float o[3] = {0.f, 0.f, 0.f};
        if (ok[cb] && a.offsets) {
          const float *po = a.offsets + (static_cast<long long>(m) * a.S + sl) * 3;
          o[0] = po[0], o[1] = po[1], o[2] = po[2];
        }
        uint4 raw[KCT];
#pragma unroll
        for (int kc = 0; kc < KCT; ++kc) {                              // (the pieces of a row in flight together)
          const int c0 = kc * 32 + 8 * g;
          raw[kc] = make_uint4(0u, 0u, 0u, 0u);
          if (ok[cb] && c0 < a.Cin) raw[kc] = *reinterpret_cast<const uint4 *>(feats + static_cast<long long>(r) * a.Cin + c0);
        }
#pragma unroll
        for (int kc = 0; kc < KCT; ++kc) {
          const int c0 = kc * 32 + 8 * g;
          B[cb][kc] = raw[kc];
          if (!plain && c0 < a.Cin) B[cb][kc] = sel4(ok[cb], x_piece<BF16>(raw[kc], stab, a.Cin, c0, o, a.relu != 0));
        }
      }
      // ---- the blocks of Cout: NCB MFMAs per A fragment, then the max of every query of the pass
      for (int nb = 0; nb < NB; ++nb) {
        f32x4 acc[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < KCT; ++kc) {
          if (kc < KC) {
            const uint4 wa = sw[((kc * NB + nb) << 6) + lane];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma16<BF16>(wa, B[cb][kc], acc[cb]);
          }
        }
        float bv[4] = {kNegInf, kNegInf, kNegInf, kNegInf};
        int bs[4] = {255, 255, 255, 255};
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const int qi = cb / ps.GL, at = cb - qi * ps.GL, m = u * ps.QP + qi;
          if (qi >= ps.QP) break;
          if (at == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[i] = kNegInf, bs[i] = 255;
          }
          const int sl = (ch * NCB + at) * 16 + ln;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (ok[cb] && acc[cb][i] > bv[i]) bv[i] = acc[cb][i], bs[i] = sl;
          if (at != ps.GL - 1) continue;
          // (the query is complete for this pass: value over the row's lanes, then the lowest slot that holds it)
          float v[4];
          int s[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[i] = row16_max(bv[i]);
            s[i] = row16_min(bv[i] == v[i] ? bs[i] : 255);
          }
          if (ln != 0 || m >= a.M) continue;
          const int co = nb * 16 + 4 * g;
          if (ch > 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)                                 // (an earlier chunk holds lower slots: it keeps ties)
              if (!(v[i] > srun[co + i])) v[i] = srun[co + i], s[i] = sslot[co + i];
          }
          if (ch < ps.NCH - 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) srun[co + i] = v[i], sslot[co + i] = s[i];
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (s[i] == 255) v[i] = 0.f;                              // no valid slot: +0
            *reinterpret_cast<uint2 *>(static_cast<uint16_t *>(a.out) + static_cast<long long>(m) * a.Cout + co) =
                make_uint2(pack2<BF16>(v[0], v[1]), pack2<BF16>(v[2], v[3]));
            if (a.arg)
              *reinterpret_cast<uint32_t *>(a.arg + static_cast<long long>(m) * a.Cout + co) =
                  static_cast<uint32_t>(s[0]) | (static_cast<uint32_t>(s[1]) << 8) | (static_cast<uint32_t>(s[2]) << 16) |
                  (static_cast<uint32_t>(s[3]) << 24);
          }
        }
      }
    }
  }
}

// KST: the 32-column steps of Cout an instance holds (Cout <= 32 KST)
template <bool BF16, int KST>
__global__ void __launch_bounds__(kBlock)
groupmax_bwd_query_kernel(GmArgs a) {
  constexpr int NCB = KST <= 4 ? 4 : 2;
  extern __shared__ uint4 smem[];
  const int KS = (a.Cout + 31) >> 5, CB = a.Cin >> 4;
  uint4 *sw = smem;                                                     // the weight in fragment order: KS * CB * 64 pieces
  float *stab = reinterpret_cast<float *>(sw + KS * CB * 64);           // [4][Cin]
  float *ssum = stab + 4 * a.Cin;                                       // [waves][4][Cin]: dpos_weight / din_bias of a wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 15, g = lane >> 4;
  const int live = live_count(a.n_live, a.n), nq = live_count(a.n_queries, a.M);
  const uint16_t *w = static_cast<const uint16_t *>(a.weight);
  for (int i = threadIdx.x; i < a.Cin * KS * 4; i += kBlock) {          // piece p of row c: lane (c & 15, p & 3) of its fragment
    const int c = i / (KS * 4), p = i - c * (KS * 4);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (8 * p < a.Cout) v = *reinterpret_cast<const uint4 *>(w + static_cast<long long>(c) * a.Cout + 8 * p);
    sw[(((p >> 2) * CB + (c >> 4)) << 6) + ((p & 3) << 4) + (c & 15)] = v;
  }
  load_table(stab, a);
  for (int i = threadIdx.x; i < kWaves * 4 * a.Cin; i += kBlock) ssum[i] = 0.f;
  __syncthreads();
  const Pass ps = pass_of(a.S, NCB);
  const int units = (a.M + ps.QP - 1) / ps.QP;
  const uint16_t *feats = static_cast<const uint16_t *>(a.feats), *dout = static_cast<const uint16_t *>(a.dout);
  uint16_t *dg = static_cast<uint16_t *>(a.out);
  float *wsum = ssum + wave * 4 * a.Cin;
  for (int u = blockIdx.x * kWaves + wave; u < units; u += gridDim.x * kWaves) {
    for (int ch = 0; ch < ps.NCH; ++ch) {
      // ---- dY^T of the pass: d_out where arg names the lane's slot
      uint4 B[NCB][KST];
      bool ok[NCB];
      int row[NCB];
      float off[NCB][3];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const int qi = cb / ps.GL, m = u * ps.QP + qi, sl = (ch * NCB + cb - qi * ps.GL) * 16 + ln;
        int r = -1;
        if (qi < ps.QP && m < nq && sl < a.S) r = a.rows[static_cast<long long>(m) * a.S + sl];
        ok[cb] = static_cast<unsigned>(r) < static_cast<unsigned>(live);
        row[cb] = r;
        off[cb][0] = off[cb][1] = off[cb][2] = 0.f;
        if (ok[cb] && a.offsets) {
          const float *po = a.offsets + (static_cast<long long>(m) * a.S + sl) * 3;
          off[cb][0] = po[0], off[cb][1] = po[1], off[cb][2] = po[2];
        }
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) {
          const int co = ks * 32 + 8 * g;
          uint4 d = make_uint4(0u, 0u, 0u, 0u);
          uint2 ar = make_uint2(~0u, ~0u);
          if (ok[cb] && co < a.Cout) {
            d = *reinterpret_cast<const uint4 *>(dout + static_cast<long long>(m) * a.Cout + co);
            ar = *reinterpret_cast<const uint2 *>(a.argin + static_cast<long long>(m) * a.Cout + co);
          }
          uint32_t k[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t b = (j < 2 ? ar.x : ar.y) >> ((j & 1) << 4);
            k[j] = ((b & 0xffu) == static_cast<uint32_t>(sl) ? 0xffffu : 0u) |
                   (((b >> 8) & 0xffu) == static_cast<uint32_t>(sl) ? 0xffff0000u : 0u);
          }
          B[cb][ks] = make_uint4(d.x & k[0], d.y & k[1], d.z & k[2], d.w & k[3]);
        }
      }
      // ---- the blocks of Cin: dX^T, the ReLU mask of the recomputed x, the sums, dG
      for (int cblk = 0; cblk < CB; ++cblk) {
        f32x4 acc[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) {
          if (ks < KS) {
            const uint4 wa = sw[((ks * CB + cblk) << 6) + lane];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma16<BF16>(wa, B[cb][ks], acc[cb]);
          }
        }
        const int c4 = cblk * 16 + 4 * g;
        float p[4][4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const float4 t = *reinterpret_cast<const float4 *>(stab + d * a.Cin + c4);
          p[d][0] = t.x, p[d][1] = t.y, p[d][2] = t.z, p[d][3] = t.w;
        }
        float sum[4][4];
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int i = 0; i < 4; ++i) sum[d][i] = 0.f;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const int qi = cb / ps.GL, m = u * ps.QP + qi, sl = (ch * NCB + cb - qi * ps.GL) * 16 + ln;
          if (qi >= ps.QP) break;
          float dx[4] = {0.f, 0.f, 0.f, 0.f};
          if (ok[cb]) {
            uint2 raw = make_uint2(0u, 0u);
            if (a.relu) raw = *reinterpret_cast<const uint2 *>(feats + static_cast<long long>(row[cb]) * a.Cin + c4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const uint32_t h = (i < 2 ? raw.x : raw.y) >> ((i & 1) << 4);
              const float x = xval(to_float<BF16>(static_cast<uint16_t>(h)), off[cb], p[0][i], p[1][i], p[2][i], p[3][i]);
              dx[i] = (!a.relu || x > 0.f) ? acc[cb][i] : 0.f;
#pragma unroll
              for (int d = 0; d < 3; ++d) sum[d][i] = fmaf(off[cb][d], dx[i], sum[d][i]);
              sum[3][i] += dx[i];
            }
          }
          if (dg && m < a.M && sl < a.S)
            *reinterpret_cast<uint2 *>(dg + (static_cast<long long>(m) * a.S + sl) * a.Cin + c4) =
                make_uint2(pack2<BF16>(dx[0], dx[1]), pack2<BF16>(dx[2], dx[3]));
        }
        if (a.ppart) {
#pragma unroll
          for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float t = row16_sum(sum[d][i]);
              if (ln == 0) wsum[d * a.Cin + c4 + i] += t;
            }
        }
      }
    }
  }
  if (!a.ppart) return;
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * a.Cin; i += kBlock) {                // (wave order: fixed)
    float t = 0.f;
    for (int wv = 0; wv < kWaves; ++wv) t += ssum[wv * 4 * a.Cin + i];
    a.ppart[static_cast<size_t>(blockIdx.x) * 4 * a.Cin + i] = t;
  }
}

template <bool BF16>
__global__ void __launch_bounds__(kBlock)
groupmax_wgrad_kernel(GmArgs a) {
  __shared__ float stile[128 * 64];                                      // the workgroup's fp32 tile, added in wave order
  __shared__ __attribute__((aligned(16))) float stab[4 * kMaxChannels];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 15, g = lane >> 4;
  const int live = live_count(a.n_live, a.n), nq = live_count(a.n_queries, a.M);
  load_table(stab, a);
  __syncthreads();
  const int cbase = blockIdx.x * 128, c0 = cbase + 8 * ln, cobase = blockIdx.y * 64;
  const bool aok = c0 < a.Cin;
  const int mbeg = min(static_cast<int>(blockIdx.z) * a.chunk, nq), mend = min(mbeg + a.chunk, nq);
  const int ebeg = mbeg * a.S, eend = mend * a.S;                        // (M * S * 3 < 2^31)
  const uint16_t *feats = static_cast<const uint16_t *>(a.feats), *dout = static_cast<const uint16_t *>(a.dout);
  f32x4 acc[8][4];
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int e0 = ebeg + wave * 32; e0 < eend; e0 += kWaves * 32) {
    uint4 x[8];
    uint32_t dy[4][8];
    int m = (e0 + 8 * g) / a.S, s = e0 + 8 * g - m * a.S;
#pragma unroll
    for (int j = 0; j < 8; ++j) {                                        // entry e0 + 8 g + j = (m, s)
      const int e = e0 + 8 * g + j;
      const int r = e < eend ? a.rows[e] : -1;
      const bool ok = static_cast<unsigned>(r) < static_cast<unsigned>(live);
      float o[3] = {0.f, 0.f, 0.f};
      if (ok && a.offsets) o[0] = a.offsets[3 * e], o[1] = a.offsets[3 * e + 1], o[2] = a.offsets[3 * e + 2];
      x[j] = make_uint4(0u, 0u, 0u, 0u);
      if (ok && aok)
        x[j] = x_piece<BF16>(*reinterpret_cast<const uint4 *>(feats + static_cast<long long>(r) * a.Cin + c0), stab, a.Cin, c0, o,
                             a.relu != 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int co = cobase + u * 16 + ln;
        dy[u][j] = 0u;
        if (ok && co < a.Cout && a.argin[static_cast<long long>(m) * a.Cout + co] == s)
          dy[u][j] = dout[static_cast<long long>(m) * a.Cout + co];
      }
      if (++s == a.S) s = 0, ++m;
    }
    uint4 yb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      yb[u] = make_uint4(dy[u][0] | (dy[u][1] << 16), dy[u][2] | (dy[u][3] << 16), dy[u][4] | (dy[u][5] << 16),
                         dy[u][6] | (dy[u][7] << 16));
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const uint4 ya = column_of(x, t);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t][u] = mfma16<BF16>(ya, yb[u], acc[t][u]);
    }
  }
  for (int wv = 0; wv < kWaves; ++wv) {                                  // (wave order: fixed)
    if (wave == wv) {
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int i = 0; i < 4; ++i) {                                  // (channel 8 (4 g + i) + t of the block, column 16 u + ln)
            float *cell = stile + (8 * (4 * g + i) + t) * 64 + u * 16 + ln;
            *cell = wv == 0 ? acc[t][u][i] : *cell + acc[t][u][i];
          }
    }
    __syncthreads();
  }
  float *part = a.partial + static_cast<size_t>(blockIdx.z) * a.Cin * a.Cout;
  for (int i = threadIdx.x; i < 128 * 64; i += kBlock) {
    const int c = cbase + (i >> 6), co = cobase + (i & 63);
    if (c < a.Cin && co < a.Cout) part[static_cast<size_t>(c) * a.Cout + co] = stile[i];
  }
}

// dweight = the partials in chunk order, rounded once; behind it dpos_weight / din_bias = the [4, Cin] partials of the
// query side in workgroup order
template <bool BF16>
__global__ void __launch_bounds__(kBlock)
groupmax_sum_kernel(const float *__restrict__ partial, int chunks, int wtotal, uint16_t *__restrict__ dw,
                    const float *__restrict__ ppart, int groups, int Cin, float *__restrict__ dpos, float *__restrict__ dbias) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < wtotal) {
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += partial[static_cast<size_t>(c) * wtotal + i];
    dw[i] = from_float<BF16>(s);
  } else if (i < wtotal + 4 * Cin && ppart) {
    const int j = i - wtotal;
    float s = 0.f;
    for (int q = 0; q < groups; ++q) s += ppart[static_cast<size_t>(q) * 4 * Cin + j];
    if (j < 3 * Cin) {
      if (dpos) dpos[j] = s;
    } else if (dbias) {
      dbias[j - 3 * Cin] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side

int check_shape(int M, int S, int n, int Cin, int Cout, int dtype) {
  SPX_CHECK(dtype == SPX_F16 || dtype == SPX_BF16, "dtype must be f16 or bf16, got %d", dtype);
  SPX_CHECK(Cin >= 16 && Cin <= kMaxChannels && Cin % 16 == 0, "Cin must be a multiple of 16 in 16 .. %d, got %d",
            kMaxChannels, Cin);
  SPX_CHECK(Cout >= 16 && Cout <= kMaxChannels && Cout % 16 == 0, "Cout must be a multiple of 16 in 16 .. %d, got %d",
            kMaxChannels, Cout);
  SPX_CHECK(M >= 0 && n >= 0, "bad query / row counts %d / %d", M, n);
  SPX_CHECK(S >= 1 && S <= kMaxSample, "nsample must be in 1 .. %d, got %d", kMaxSample, S);
  SPX_CHECK(static_cast<long long>(M) * S * 3 < 0x80000000LL, "M * nsample * 3 must stay below 2^31, got %d x %d", M, S);
  return 0;
}

// steps of 32 an instance holds for a reduction axis of C elements: 1, 2, 4 or 8
int steps_of(int C) { return C <= 32 ? 1 : (C <= 64 ? 2 : (C <= 128 ? 4 : 8)); }

size_t fwd_lds(int Cin, int Cout) {
  return static_cast<size_t>((Cin + 31) / 32) * 32 * Cout * 2 + 16 * Cin + static_cast<size_t>(kWaves) * Cout * 8;
}
size_t bwd_lds(int Cin, int Cout) {
  return static_cast<size_t>((Cout + 31) / 32) * 32 * Cin * 2 + 16 * Cin + static_cast<size_t>(kWaves) * 16 * Cin;
}

// persistent workgroups: as many per CU as their LDS allows (at most 4), never more than there are passes for
int grid_of(int M, int S, int steps, size_t lds) {
  const Pass ps = pass_of(S, steps <= 4 ? 4 : 2);
  const int units = (M + ps.QP - 1) / ps.QP, want = (units + kWaves - 1) / kWaves;
  int per = static_cast<int>(kLdsBytes / lds);
  per = per < 1 ? 1 : (per > 4 ? 4 : per);
  return want < kCUs * per ? (want < 1 ? 1 : want) : kCUs * per;
}

// the weight side's split of the queries: host-known sizes only
void wgrad_split(int M, int Cin, int Cout, int *chunks, int *chunk) {
  int cap = kWgPartial / (Cin * Cout);
  cap = cap > kWgChunks ? kWgChunks : cap;
  int c = (M + kWgMinChunk - 1) / kWgMinChunk;
  c = c < 1 ? 1 : (c > cap ? cap : c);
  *chunk = (M + c - 1) / c;
  if (*chunk < 1) *chunk = 1;
  *chunks = c;
}

size_t wpart_bytes(int M, int Cin, int Cout) {
  int chunks, chunk;
  wgrad_split(M, Cin, Cout, &chunks, &chunk);
  return align_up(static_cast<size_t>(chunks) * Cin * Cout * sizeof(float), 256);
}

template <typename K> int launch_lds(K kern, int grid, size_t lds, hipStream_t s, const GmArgs &a, std::atomic<uint64_t> &done) {
  SPX_HIP(ensure_dynamic_lds(reinterpret_cast<const void *>(kern), kLdsBytes, done));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, s, a);
  SPX_LAUNCH_CHECK();
  return 0;
}

template <int ST> int launch_fwd(bool bf16, int grid, size_t lds, hipStream_t s, const GmArgs &a) {
  static std::atomic<uint64_t> done_h{0}, done_b{0};      // one bit per device (common.h: ensure_dynamic_lds)
  return bf16 ? launch_lds(groupmax_fwd_kernel<true, ST>, grid, lds, s, a, done_b)
              : launch_lds(groupmax_fwd_kernel<false, ST>, grid, lds, s, a, done_h);
}
template <int ST> int launch_bwd(bool bf16, int grid, size_t lds, hipStream_t s, const GmArgs &a) {
  static std::atomic<uint64_t> done_h{0}, done_b{0};
  return bf16 ? launch_lds(groupmax_bwd_query_kernel<true, ST>, grid, lds, s, a, done_b)
              : launch_lds(groupmax_bwd_query_kernel<false, ST>, grid, lds, s, a, done_h);
}

}  // namespace
}  // namespace spx

extern "C" {

size_t spx_group_linear_max_ws_bytes(int M, int S, int Cin, int Cout, int backward) {
  using namespace spx;
  if (M < 0 || S < 1 || S > kMaxSample || Cin < 16 || Cin > kMaxChannels || Cin % 16 || Cout < 16 || Cout > kMaxChannels ||
      Cout % 16)
    return 0;
  if (!backward) return align_up(static_cast<size_t>((Cin + 31) / 32) * 32 * Cout * 2, 256);
  const int grid = grid_of(M, S, steps_of(Cout), bwd_lds(Cin, Cout));
  return wpart_bytes(M, Cin, Cout) + align_up(static_cast<size_t>(grid) * 4 * Cin * sizeof(float), 256);
}

int spx_group_linear_max_fwd(const void *feats, const int32_t *rows, const float *offsets, const void *weight,
                             const float *pos_weight, const float *in_bias, int M, int S, int n, const int32_t *n_queries,
                             const int32_t *n_live, int Cin, int Cout, int dtype, int relu_in, void *out, uint8_t *arg,
                             void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_shape(M, S, n, Cin, Cout, dtype)) return rc;
  if (M == 0) return 0;
  SPX_CHECK(rows && weight && out && ws && (n == 0 || feats), "feats / rows / weight / out / ws is NULL");
  SPX_CHECK(!pos_weight || offsets, "pos_weight needs the offsets of the table");
  SPX_CHECK(aligned_to(feats, 16) && aligned_to(weight, 16) && aligned_to(out, 16) && aligned_to(ws, 16) &&
            aligned_to(arg, 4) && aligned_to(rows, 4) && aligned_to(offsets, 4) && aligned_to(pos_weight, 4) &&
            aligned_to(in_bias, 4), "rows must be aligned to 16 bytes, tables to their elements");
  const int pieces = (Cin + 31) / 32 * (Cout / 16) * 64;
  SPX_CHECK(ws_bytes >= static_cast<size_t>(pieces) * 16, "workspace too small: %zu < %zu bytes", ws_bytes,
            static_cast<size_t>(pieces) * 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(groupmax_pack_kernel, dim3((pieces + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                     static_cast<const uint16_t *>(weight), static_cast<uint4 *>(ws), Cin, Cout, pieces);
  SPX_LAUNCH_CHECK();
  GmArgs a = {};
  a.feats = feats, a.rows = rows, a.offsets = pos_weight ? offsets : nullptr, a.pos = pos_weight, a.bias = in_bias, a.weight = ws;
  a.M = M, a.S = S, a.n = n, a.n_queries = n_queries, a.n_live = n_live, a.Cin = Cin, a.Cout = Cout;
  a.relu = relu_in ? 1 : 0, a.out = out, a.arg = arg;
  const size_t lds = fwd_lds(Cin, Cout);
  const int steps = steps_of(Cin), grid = grid_of(M, S, steps, lds);
  int rc = 0;
  dispatch_value<1, 2, 4, 8>(steps, [&](auto st) { rc = launch_fwd<decltype(st)::value>(dtype == SPX_BF16, grid, lds, s, a); });
  return rc;
}

int spx_group_linear_max_bwd(const void *feats, const int32_t *rows, const float *offsets, const void *weight,
                             const float *pos_weight, const float *in_bias, const uint8_t *arg, const void *d_out, int M,
                             int S, int n, const int32_t *n_queries, const int32_t *n_live, int Cin, int Cout, int dtype,
                             int relu_in, void *dg, void *dweight, float *dpos, float *dbias, void *ws, size_t ws_bytes,
                             spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_shape(M, S, n, Cin, Cout, dtype)) return rc;
  if (M == 0 || (!dg && !dweight && !dpos && !dbias)) return 0;
  SPX_CHECK(rows && weight && arg && d_out && (n == 0 || feats), "feats / rows / weight / arg / d_out is NULL");
  SPX_CHECK(!pos_weight || offsets, "pos_weight needs the offsets of the table");
  SPX_CHECK(!dpos || offsets, "dpos needs the offsets of the table");
  SPX_CHECK(aligned_to(feats, 16) && aligned_to(weight, 16) && aligned_to(d_out, 16) && aligned_to(dg, 16) &&
            aligned_to(dweight, 16) && aligned_to(ws, 16) && aligned_to(arg, 8) && aligned_to(rows, 4) &&
            aligned_to(offsets, 4) && aligned_to(pos_weight, 4) && aligned_to(in_bias, 4) && aligned_to(dpos, 4) &&
            aligned_to(dbias, 4), "rows must be aligned to 16 bytes, arg to 8, tables to their elements");
  const bool sums = dpos || dbias, bf16 = dtype == SPX_BF16;
  if (dweight || sums) {
    SPX_CHECK(ws, "ws is NULL");
    SPX_CHECK(ws_bytes >= spx_group_linear_max_ws_bytes(M, S, Cin, Cout, 1), "workspace too small: %zu < %zu bytes", ws_bytes,
              spx_group_linear_max_ws_bytes(M, S, Cin, Cout, 1));
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  GmArgs a = {};
  a.feats = feats, a.rows = rows, a.offsets = pos_weight ? offsets : nullptr, a.pos = pos_weight, a.bias = in_bias, a.weight = weight;
  a.dout = d_out, a.argin = arg, a.M = M, a.S = S, a.n = n, a.n_queries = n_queries, a.n_live = n_live;
  a.Cin = Cin, a.Cout = Cout, a.relu = relu_in ? 1 : 0;
  float *partial = static_cast<float *>(ws);
  float *ppart = sums ? reinterpret_cast<float *>(static_cast<char *>(ws) + wpart_bytes(M, Cin, Cout)) : nullptr;
  const size_t lds = bwd_lds(Cin, Cout);
  const int steps = steps_of(Cout), grid = grid_of(M, S, steps, lds);
  if (dg || sums) {
    GmArgs q = a;
    q.out = dg, q.ppart = ppart;
    int rc = 0;
    dispatch_value<1, 2, 4, 8>(steps, [&](auto st) { rc = launch_bwd<decltype(st)::value>(bf16, grid, lds, s, q); });
    if (rc) return rc;
  }
  int chunks = 0, chunk = 0;
  if (dweight) {
    wgrad_split(M, Cin, Cout, &chunks, &chunk);
    GmArgs q = a;
    q.partial = partial, q.chunk = chunk;
    const dim3 wgrid((Cin + 127) / 128, (Cout + 63) / 64, chunks);
    if (bf16) hipLaunchKernelGGL(groupmax_wgrad_kernel<true>, wgrid, dim3(kBlock), 0, s, q);
    else hipLaunchKernelGGL(groupmax_wgrad_kernel<false>, wgrid, dim3(kBlock), 0, s, q);
    SPX_LAUNCH_CHECK();
  }
  const int wtotal = dweight ? Cin * Cout : 0, total = wtotal + (sums ? 4 * Cin : 0);
  if (total == 0) return 0;
  const dim3 sgrid((total + kBlock - 1) / kBlock);
  uint16_t *dw = static_cast<uint16_t *>(dweight);
  if (bf16) hipLaunchKernelGGL(groupmax_sum_kernel<true>, sgrid, dim3(kBlock), 0, s, partial, chunks, wtotal, dw, ppart, grid, Cin, dpos, dbias);
  else hipLaunchKernelGGL(groupmax_sum_kernel<false>, sgrid, dim3(kBlock), 0, s, partial, chunks, wtotal, dw, ppart, grid, Cin, dpos, dbias);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
