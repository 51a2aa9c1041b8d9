// Serialised patch attention (spx_patch_attn_fwd, spx_patch_attn_bwd): the attention of the serialised point / voxel
// transformers (Point Transformer V3, OctFormer, FlatFormer-style blocks) over the patches of a PatchPlan, read
// THROUGH the plan -- no patch-ordered copy of Q, K or V, no score matrix in memory.
//
//   split     a workgroup of four waves owns 64 slots of one patch (16 per wave) and one HEAD GROUP: 64 / D heads, i.e.
//             64 consecutive elements = 128 bytes of a row's Q, K or V section.  It walks the patch in blocks of 32
//             slots; a block's rows are fetched once (thread t: slot t / 8, 16-byte piece t % 8) into registers while
//             the block before is worked on, and stored into one of two LDS stages (one barrier per block).
//   layouts   everything is computed TRANSPOSED, so that a lane keeps one column for the whole walk:
//             S^T = K Q^T with v_mfma_f32_16x16x32: A = 16 walked slots x D from a row-major LDS tile, B = the wave's 16
//             own slots straight from global memory into registers, once.  Lane (j = lane & 15, g = lane >> 4) then
//             holds, of own slot j, the walked slots 16 t + 4 g + r of the two tiles t = 0, 1 (r = 0 .. 3): eight numbers
//             that ARE the B operand of the second product (reduction index 8 g + 4 t + r) under a permuted slot order.
//             Its A operand comes from a TRANSPOSED LDS tile [element][slot]: two 8-byte reads (slots 4 g .. 4 g + 3 of
//             each tile) mirror the permutation.  P never leaves the registers.  D = 16 runs the x32 instruction with a
//             zero upper half.
//   forward   online softmax in fp32 (log2 domain): the maximum of an own slot is reduced over its four lanes, the sum
//             stays a per-lane partial until the epilogue; O^T = V^T P^T accumulates per (head, 16 elements).
//   backward  delta = rowsum(dO * O) (a pre-pass, one thread per (row, head)); a dQ kernel (own slots = queries, walks
//             keys, dQ^T = K^T dS^T) and a dK/dV kernel (own slots = keys, walks the canonical queries, dV^T = dO^T P,
//             dK^T = Q^T dS), both recomputing P from the saved log-sum-exp: S is computed twice, and nothing is
//             added across workgroups -- no atomics, no waiting.  dK / dV go per SLOT in fp32 to the workspace; a last
//             launch writes a row's dK / dV as ws[row_slot] + ws[row_slot2] (the rule of spx_patch_rows_bwd) and zeroes
//             the dead rows.
// Every plan entry is range-checked before it addresses anything.  Grids and loop bounds are host-known.
#include "igemm_defs.h"
#include "piece.h"

namespace spx {
namespace {

constexpr int kOwn = 64;                         // slots a workgroup owns
constexpr int kWalk = 32;                        // slots per walked block
constexpr int kHW = 64;                          // elements of a section a workgroup handles (64 / D heads)
constexpr int kRmStride = (kHW + 8) * 2;         // bytes between the rows of a row-major tile: 16 rows on 16 bank slots
constexpr int kTrStride = (kWalk + 4) * 2;       // bytes between the element rows of a transposed tile
constexpr int kRmBytes = kWalk * kRmStride;
constexpr int kTrBytes = kHW * kTrStride;
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

struct AttnArgs {
  const uint16_t *qkv;                           // [n, 3, H, D]
  const uint16_t *out;                           // [n, H, D]    (backward)
  const uint16_t *d_out;                         // [n, H, D]    (backward)
  const int32_t *patch_rows, *patch_rows_canon, *n_patches;
  int n, P_cap, K, H;
  float scale;
  uint16_t *out_w;                               // forward: out; dQ kernel: dqkv
  float *lse;                                    // [P_cap * K, H]
  float *delta;                                  // [n, H]
  float *dkv;                                    // [P_cap * K, 2, H, D]
};

__device__ __forceinline__ int checked_row(const int32_t *__restrict__ table, long long slot, int n) {
  const int r = table[slot];
  return static_cast<unsigned>(r) < static_cast<unsigned>(n) ? r : -1;      // (checked, not trusted)
}

__device__ __forceinline__ uint4 load16(const uint16_t *p, bool ok) {
  return ok ? *reinterpret_cast<const uint4 *>(p) : make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ void stage_rm(char *tile, int slot, int pc, const uint4 &v) {
  *reinterpret_cast<uint4 *>(tile + slot * kRmStride + pc * 16) = v;
}

__device__ __forceinline__ void stage_tr(char *tile, int slot, int pc, const uint4 &v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t w = dword_of4(v, e >> 1);
    *reinterpret_cast<uint16_t *>(tile + (pc * 8 + e) * kTrStride + slot * 2) =
        static_cast<uint16_t>((e & 1) ? (w >> 16) : (w & 0xffffu));
  }
}

// A operand of a product over the elements: 8 elements from `col` of walked slot `slot`
__device__ __forceinline__ uint4 frag_rm(const char *tile, int slot, int col) {
  return *reinterpret_cast<const uint4 *>(tile + slot * kRmStride + col * 2);
}

// A operand of a product over the walked slots: element row e, slots 4 g .. 4 g + 3 of both 16-slot tiles
__device__ __forceinline__ uint4 frag_tr(const char *tile, int e, int g) {
  const uint2 a = *reinterpret_cast<const uint2 *>(tile + e * kTrStride + g * 8);
  const uint2 b = *reinterpret_cast<const uint2 *>(tile + e * kTrStride + 32 + g * 8);
  return make_uint4(a.x, a.y, b.x, b.y);
}

template <bool BF16>
__device__ __forceinline__ uint4 pack8(const float (&x)[8]) {
  return make_uint4(pack2<BF16>(x[0], x[1]), pack2<BF16>(x[2], x[3]), pack2<BF16>(x[4], x[5]), pack2<BF16>(x[6], x[7]));
}

__device__ __forceinline__ float quad_max(float v) {      // over the four lanes j, j + 16, j + 32, j + 48
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// What the three walking kernels share: who the workgroup and the lane are.
template <int D>
struct Who {
  static constexpr int HG = kHW / D, DC = (D + 31) / 32, DT = D / 16;
  int lane, wave, j, g, p, hg, nh, HD, own0, sl, pc;
  long long base;                                // first slot of the patch
  bool live, wave_on, pc_on;
  __device__ __forceinline__ Who(const AttnArgs &a) {
    const int tid = threadIdx.x, nob = (a.K + kOwn - 1) / kOwn;
    lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    p = blockIdx.x / nob;
    hg = blockIdx.y;
    HD = a.H * D;
    nh = min(HG, a.H - hg * HG);
    own0 = (blockIdx.x - p * nob) * kOwn + wave * 16;
    wave_on = own0 < a.K;                        // (K is a multiple of 32: a 16-slot tile lies inside or outside)
    live = p < min(*a.n_patches, a.P_cap);
    base = static_cast<long long>(p) * a.K;
    sl = tid >> 3, pc = tid & 7;                 // the thread's part of a stage: slot of the block, 16-byte piece
    pc_on = hg * kHW + pc * 8 < HD;
  }
  // element offset of piece pc of section sec in row `row` of qkv
  __device__ __forceinline__ size_t at(int row, int sec) const {
    return static_cast<size_t>(row) * 3 * HD + static_cast<size_t>(sec) * HD + hg * kHW;
  }
  // the lane's B operands of own row `row`: elements 8 g .. 8 g + 7 of every 32-element chunk of every head
  __device__ __forceinline__ void own_frags(const uint16_t *__restrict__ rowp, bool ok, uint4 (&f)[HG][DC]) const {
#pragma unroll
    for (int hh = 0; hh < HG; ++hh)
#pragma unroll
      for (int c = 0; c < DC; ++c)
        f[hh][c] = load16(rowp + hh * D + 32 * c + 8 * g, ok && hh < nh && (D >= 32 || g < 2));
  }
};

template <bool BF16, int D>
__device__ __forceinline__ f32x4 dot_tile(const char *tile, int slot, int hh, int g, const uint4 (&own)[(D + 31) / 32]) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < (D + 31) / 32; ++c) {
    uint4 a = make_uint4(0u, 0u, 0u, 0u);
    if (D >= 32 || g < 2) a = frag_rm(tile, slot, hh * D + 32 * c + 8 * g);
    s = mfma16<BF16>(a, own[c], s);
  }
  return s;
}

// ---------------------------------------------------------------------------------------------------- forward
template <bool BF16, int D>
__global__ void __launch_bounds__(256) attn_fwd_kernel(AttnArgs a) {
  using W = Who<D>;
  constexpr int HG = W::HG, DC = W::DC, DT = W::DT;
  constexpr int kStage = kRmBytes + kTrBytes + kWalk * 4;
  __shared__ __attribute__((aligned(16))) char lds[2][kStage];
  const W w(a);
  if (!w.live) return;
  const int j = w.j, g = w.g;
  int qrow = -1;
  if (w.wave_on) qrow = checked_row(a.patch_rows_canon, w.base + w.own0 + j, a.n);
  uint4 qf[HG][DC];
  w.own_frags(a.qkv + w.at(qrow < 0 ? 0 : qrow, 0), qrow >= 0, qf);

  float m[HG], l[HG];
  f32x4 o[HG][DT];
#pragma unroll
  for (int hh = 0; hh < HG; ++hh) {
    m[hh] = -INFINITY;
    l[hh] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[hh][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sl2 = a.scale * kLog2e;
  const int nblk = a.K / kWalk;
  uint4 kr, vr;
  int krow;
  auto fetch = [&](int blk) {
    krow = checked_row(a.patch_rows, w.base + blk * kWalk + w.sl, a.n);
    const bool ok = krow >= 0 && w.pc_on;
    const uint16_t *rp = a.qkv + w.at(krow < 0 ? 0 : krow, 1) + w.pc * 8;
    kr = load16(rp, ok);
    vr = load16(rp + w.HD, ok);
  };
  auto stash = [&](int buf) {
    stage_rm(lds[buf], w.sl, w.pc, kr);
    stage_tr(lds[buf] + kRmBytes, w.sl, w.pc, vr);
    if (w.pc == 0) reinterpret_cast<int *>(lds[buf] + kRmBytes + kTrBytes)[w.sl] = krow >= 0 ? 1 : 0;
  };
  fetch(0);
  stash(0);
  __syncthreads();
  for (int blk = 0; blk < nblk; ++blk) {
    const int buf = blk & 1;
    if (blk + 1 < nblk) fetch(blk + 1);
    if (w.wave_on) {
      const char *krm = lds[buf], *vtr = lds[buf] + kRmBytes;
      const int *kval = reinterpret_cast<const int *>(lds[buf] + kRmBytes + kTrBytes);
      const int4 v0 = *reinterpret_cast<const int4 *>(kval + 4 * g), v1 = *reinterpret_cast<const int4 *>(kval + 16 + 4 * g);
      const bool kv[8] = {v0.x != 0, v0.y != 0, v0.z != 0, v0.w != 0, v1.x != 0, v1.y != 0, v1.z != 0, v1.w != 0};
#pragma unroll
      for (int hh = 0; hh < HG; ++hh) {
        if (hh < w.nh) {
          float x[8];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const f32x4 s = dot_tile<BF16, D>(krm, 16 * t + j, hh, g, qf[hh]);
#pragma unroll
            for (int r = 0; r < 4; ++r) x[4 * t + r] = kv[4 * t + r] ? s[r] * sl2 : -INFINITY;
          }
          float bm = x[0];
#pragma unroll
          for (int i = 1; i < 8; ++i) bm = fmaxf(bm, x[i]);
          const float mnew = fmaxf(m[hh], quad_max(bm));
          const float muse = mnew == -INFINITY ? 0.f : mnew;      // (no valid key yet: every exponent below is -inf)
          const float alpha = __builtin_amdgcn_exp2f(m[hh] - muse);
          m[hh] = mnew;
          float ps = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            x[i] = __builtin_amdgcn_exp2f(x[i] - muse);
            ps += x[i];
          }
          l[hh] = l[hh] * alpha + ps;
          const uint4 pb = pack8<BF16>(x);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) o[hh][dt][r] *= alpha;
            o[hh][dt] = mfma16<BF16>(frag_tr(vtr, hh * D + 16 * dt + j, g), pb, o[hh][dt]);
          }
        }
      }
    }
    if (blk + 1 < nblk) stash(buf ^ 1);
    __syncthreads();
  }
  if (!w.wave_on) return;
#pragma unroll
  for (int hh = 0; hh < HG; ++hh) {
    if (hh < w.nh) {
      const float lt = quad_sum(l[hh]);
      const float inv = lt > 0.f ? 1.f / lt : 0.f;
      if (qrow >= 0) {
        const int h = w.hg * HG + hh;
        uint16_t *op = a.out_w + static_cast<size_t>(qrow) * w.HD + h * D + 4 * g;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          *reinterpret_cast<uint2 *>(op + 16 * dt) = make_uint2(pack2<BF16>(o[hh][dt][0] * inv, o[hh][dt][1] * inv),
                                                                pack2<BF16>(o[hh][dt][2] * inv, o[hh][dt][3] * inv));
        if (g == 0)
          a.lse[static_cast<size_t>(w.base + w.own0 + j) * a.H + h] =
              lt > 0.f ? (m[hh] + __builtin_amdgcn_logf(lt)) * kLn2 : 0.f;
      }
    }
  }
}

// rows of `out` (pieces of 16 bytes) without a canonical slot: zeros
__global__ void __launch_bounds__(256)
attn_dead_rows_kernel(const int32_t *__restrict__ row_slot, long long slots, long long total, int pieces,
                      uint4 *__restrict__ out) {
  for (long long item = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * 256) {
    const long long r = row_of(item, total, pieces);
    if (static_cast<unsigned long long>(static_cast<long long>(row_slot[r])) >= static_cast<unsigned long long>(slots))
      out[item] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// ---------------------------------------------------------------------------------------------------- backward
// delta[row, h] = sum_d dO * O in fp32, one thread per (row, head); dead rows are never read
template <bool BF16, int D>
__global__ void __launch_bounds__(256)
attn_delta_kernel(const uint16_t *__restrict__ out, const uint16_t *__restrict__ d_out, long long total,
                  float *__restrict__ delta) {
  for (long long item = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * 256) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < D / 8; ++c) {
      const uint4 x = *reinterpret_cast<const uint4 *>(out + item * D + 8 * c);
      const uint4 y = *reinterpret_cast<const uint4 *>(d_out + item * D + 8 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t xw = dword_of4(x, e), yw = dword_of4(y, e);
        acc += to_float<BF16>(static_cast<uint16_t>(xw & 0xffffu)) * to_float<BF16>(static_cast<uint16_t>(yw & 0xffffu));
        acc += to_float<BF16>(static_cast<uint16_t>(xw >> 16)) * to_float<BF16>(static_cast<uint16_t>(yw >> 16));
      }
    }
    delta[item] = acc;
  }
}

// own slots = queries; walks the keys.  Stage: K row-major (S^T), K transposed (dQ^T), V row-major (dP^T), validity.
template <bool BF16, int D>
__global__ void __launch_bounds__(256) attn_dq_kernel(AttnArgs a) {
  using W = Who<D>;
  constexpr int HG = W::HG, DC = W::DC, DT = W::DT;
  constexpr int kStage = 2 * kRmBytes + kTrBytes + kWalk * 4;
  __shared__ __attribute__((aligned(16))) char lds[2][kStage];
  const W w(a);
  if (!w.live) return;
  const int j = w.j, g = w.g;
  int qrow = -1;
  if (w.wave_on) qrow = checked_row(a.patch_rows_canon, w.base + w.own0 + j, a.n);
  const int qr0 = qrow < 0 ? 0 : qrow;
  uint4 qf[HG][DC], dof[HG][DC];
  w.own_frags(a.qkv + w.at(qr0, 0), qrow >= 0, qf);
  w.own_frags(a.d_out + static_cast<size_t>(qr0) * w.HD + w.hg * kHW, qrow >= 0, dof);
  float lse2[HG], dl[HG];
  f32x4 dq[HG][DT];
#pragma unroll
  for (int hh = 0; hh < HG; ++hh) {
    const bool ok = qrow >= 0 && hh < w.nh;
    const int h = w.hg * HG + (ok ? hh : 0);
    lse2[hh] = ok ? a.lse[static_cast<size_t>(w.base + w.own0 + j) * a.H + h] * kLog2e : INFINITY;
    dl[hh] = ok ? a.delta[static_cast<size_t>(qr0) * a.H + h] : 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[hh][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sl2 = a.scale * kLog2e;
  const int nblk = a.K / kWalk;
  uint4 kr, vr;
  int krow;
  auto fetch = [&](int blk) {
    krow = checked_row(a.patch_rows, w.base + blk * kWalk + w.sl, a.n);
    const bool ok = krow >= 0 && w.pc_on;
    const uint16_t *rp = a.qkv + w.at(krow < 0 ? 0 : krow, 1) + w.pc * 8;
    kr = load16(rp, ok);
    vr = load16(rp + w.HD, ok);
  };
  auto stash = [&](int buf) {
    stage_rm(lds[buf], w.sl, w.pc, kr);
    stage_rm(lds[buf] + kRmBytes, w.sl, w.pc, vr);
    stage_tr(lds[buf] + 2 * kRmBytes, w.sl, w.pc, kr);
    if (w.pc == 0) reinterpret_cast<int *>(lds[buf] + 2 * kRmBytes + kTrBytes)[w.sl] = krow >= 0 ? 1 : 0;
  };
  fetch(0);
  stash(0);
  __syncthreads();
  for (int blk = 0; blk < nblk; ++blk) {
    const int buf = blk & 1;
    if (blk + 1 < nblk) fetch(blk + 1);
    if (w.wave_on) {
      const char *krm = lds[buf], *vrm = lds[buf] + kRmBytes, *ktr = lds[buf] + 2 * kRmBytes;
      const int *kval = reinterpret_cast<const int *>(lds[buf] + 2 * kRmBytes + kTrBytes);
      const int4 v0 = *reinterpret_cast<const int4 *>(kval + 4 * g), v1 = *reinterpret_cast<const int4 *>(kval + 16 + 4 * g);
      const bool kv[8] = {v0.x != 0, v0.y != 0, v0.z != 0, v0.w != 0, v1.x != 0, v1.y != 0, v1.z != 0, v1.w != 0};
#pragma unroll
      for (int hh = 0; hh < HG; ++hh) {
        if (hh < w.nh) {
          float ds[8];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const f32x4 s = dot_tile<BF16, D>(krm, 16 * t + j, hh, g, qf[hh]);
            const f32x4 dp = dot_tile<BF16, D>(vrm, 16 * t + j, hh, g, dof[hh]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float pr = kv[4 * t + r] ? __builtin_amdgcn_exp2f(s[r] * sl2 - lse2[hh]) : 0.f;
              ds[4 * t + r] = pr * (dp[r] - dl[hh]);
            }
          }
          const uint4 db = pack8<BF16>(ds);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
            dq[hh][dt] = mfma16<BF16>(frag_tr(ktr, hh * D + 16 * dt + j, g), db, dq[hh][dt]);
        }
      }
    }
    if (blk + 1 < nblk) stash(buf ^ 1);
    __syncthreads();
  }
  if (!w.wave_on || qrow < 0) return;
#pragma unroll
  for (int hh = 0; hh < HG; ++hh) {
    if (hh < w.nh) {
      uint16_t *op = a.out_w + w.at(qrow, 0) + hh * D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        *reinterpret_cast<uint2 *>(op + 16 * dt) =
            make_uint2(pack2<BF16>(dq[hh][dt][0] * a.scale, dq[hh][dt][1] * a.scale),
                       pack2<BF16>(dq[hh][dt][2] * a.scale, dq[hh][dt][3] * a.scale));
    }
  }
}

// own slots = keys; walks the canonical queries.  Stage: Q and dO row-major (S, dP) and transposed (dK^T, dV^T), and
// per (head, query) the log-sum-exp (+inf for a slot that is no query: its P is zero) and delta.
template <bool BF16, int D>
__global__ void __launch_bounds__(256) attn_dkv_kernel(AttnArgs a) {
  using W = Who<D>;
  constexpr int HG = W::HG, DC = W::DC, DT = W::DT;
  constexpr int kTiles = 2 * kRmBytes + 2 * kTrBytes;
  constexpr int kStage = kTiles + 2 * HG * kWalk * 4;
  __shared__ __attribute__((aligned(16))) char lds[2][kStage];
  const W w(a);
  if (!w.live) return;
  const int j = w.j, g = w.g, tid = threadIdx.x;
  int krow = -1;
  if (w.wave_on) krow = checked_row(a.patch_rows, w.base + w.own0 + j, a.n);
  uint4 kf[HG][DC], vf[HG][DC];
  w.own_frags(a.qkv + w.at(krow < 0 ? 0 : krow, 1), krow >= 0, kf);
  w.own_frags(a.qkv + w.at(krow < 0 ? 0 : krow, 2), krow >= 0, vf);
  f32x4 dk[HG][DT], dv[HG][DT];
#pragma unroll
  for (int hh = 0; hh < HG; ++hh)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dk[hh][dt] = dv[hh][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = a.scale * kLog2e;
  const int nblk = a.K / kWalk;
  uint4 qr, dor;
  float lr = INFINITY, dr = 0.f;
  auto fetch = [&](int blk) {
    const int row = checked_row(a.patch_rows_canon, w.base + blk * kWalk + w.sl, a.n);
    const bool ok = row >= 0 && w.pc_on;
    const int r0 = row < 0 ? 0 : row;
    qr = load16(a.qkv + w.at(r0, 0) + w.pc * 8, ok);
    dor = load16(a.d_out + static_cast<size_t>(r0) * w.HD + w.hg * kHW + w.pc * 8, ok);
    if (tid < HG * kWalk) {                      // (head tid / 32, query tid % 32)
      const int hh = tid / kWalk, q = tid % kWalk, h = w.hg * HG + hh;
      const long long slot = w.base + blk * kWalk + q;
      const int qrow = checked_row(a.patch_rows_canon, slot, a.n);
      const bool on = qrow >= 0 && hh < w.nh;
      lr = on ? a.lse[static_cast<size_t>(slot) * a.H + h] * kLog2e : INFINITY;
      dr = on ? a.delta[static_cast<size_t>(qrow) * a.H + h] : 0.f;
    }
  };
  auto stash = [&](int buf) {
    stage_rm(lds[buf], w.sl, w.pc, qr);
    stage_rm(lds[buf] + kRmBytes, w.sl, w.pc, dor);
    stage_tr(lds[buf] + 2 * kRmBytes, w.sl, w.pc, qr);
    stage_tr(lds[buf] + 2 * kRmBytes + kTrBytes, w.sl, w.pc, dor);
    if (tid < HG * kWalk) {
      reinterpret_cast<float *>(lds[buf] + kTiles)[tid] = lr;
      reinterpret_cast<float *>(lds[buf] + kTiles)[HG * kWalk + tid] = dr;
    }
  };
  fetch(0);
  stash(0);
  __syncthreads();
  for (int blk = 0; blk < nblk; ++blk) {
    const int buf = blk & 1;
    if (blk + 1 < nblk) fetch(blk + 1);
    if (w.wave_on) {
      const char *qrm = lds[buf], *dorm = lds[buf] + kRmBytes, *qtr = lds[buf] + 2 * kRmBytes,
                 *dotr = lds[buf] + 2 * kRmBytes + kTrBytes;
      const float *lq = reinterpret_cast<const float *>(lds[buf] + kTiles), *dlq = lq + HG * kWalk;
#pragma unroll
      for (int hh = 0; hh < HG; ++hh) {
        if (hh < w.nh) {
          float pr[8], ds[8];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const f32x4 s = dot_tile<BF16, D>(qrm, 16 * t + j, hh, g, kf[hh]);
            const f32x4 dp = dot_tile<BF16, D>(dorm, 16 * t + j, hh, g, vf[hh]);
            const float4 L = *reinterpret_cast<const float4 *>(lq + hh * kWalk + 16 * t + 4 * g);
            const float4 Dl = *reinterpret_cast<const float4 *>(dlq + hh * kWalk + 16 * t + 4 * g);
            const float Lr[4] = {L.x, L.y, L.z, L.w}, Dr[4] = {Dl.x, Dl.y, Dl.z, Dl.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              pr[4 * t + r] = __builtin_amdgcn_exp2f(s[r] * sl2 - Lr[r]);
              ds[4 * t + r] = pr[4 * t + r] * (dp[r] - Dr[r]);
            }
          }
          const uint4 pb = pack8<BF16>(pr), db = pack8<BF16>(ds);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            dv[hh][dt] = mfma16<BF16>(frag_tr(dotr, hh * D + 16 * dt + j, g), pb, dv[hh][dt]);
            dk[hh][dt] = mfma16<BF16>(frag_tr(qtr, hh * D + 16 * dt + j, g), db, dk[hh][dt]);
          }
        }
      }
    }
    if (blk + 1 < nblk) stash(buf ^ 1);
    __syncthreads();
  }
  if (!w.wave_on || krow < 0) return;
#pragma unroll
  for (int hh = 0; hh < HG; ++hh) {
    if (hh < w.nh) {
      float *op = a.dkv + static_cast<size_t>(w.base + w.own0 + j) * 2 * w.HD + (w.hg * HG + hh) * D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        *reinterpret_cast<float4 *>(op + 16 * dt) = make_float4(dk[hh][dt][0] * a.scale, dk[hh][dt][1] * a.scale,
                                                                dk[hh][dt][2] * a.scale, dk[hh][dt][3] * a.scale);
        *reinterpret_cast<float4 *>(op + w.HD + 16 * dt) =
            make_float4(dv[hh][dt][0], dv[hh][dt][1], dv[hh][dt][2], dv[hh][dt][3]);
      }
    }
  }
}

// One item per (row, 4 elements of dqkv): the K and V sections take ws[row_slot] + ws[row_slot2], canonical term first,
// added in fp32 and rounded once; a dead row gets zeros in all three sections (a live row's Q section is the dQ kernel's).
template <bool BF16>
__global__ void __launch_bounds__(256)
attn_rows_kernel(const float *__restrict__ dkv, const int32_t *__restrict__ row_slot, const int32_t *__restrict__ row_slot2,
                 long long slots, long long total, int HD, uint16_t *__restrict__ dqkv) {
  const int pieces = 3 * HD / 4;
  for (long long item = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * 256) {
    const long long r = row_of(item, total, pieces);
    const int e = static_cast<int>(item - r * pieces) * 4;
    long long s1 = row_slot[r], s2 = row_slot2[r];
    if (static_cast<unsigned long long>(s1) >= static_cast<unsigned long long>(slots)) s1 = -1;      // (checked)
    if (static_cast<unsigned long long>(s2) >= static_cast<unsigned long long>(slots)) s2 = -1;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
    if (e < HD) {
      if (s1 >= 0) continue;
    } else {
      if (s1 >= 0) {
        const float4 x = *reinterpret_cast<const float4 *>(dkv + s1 * 2 * HD + (e - HD));
        x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w;
      }
      if (s2 >= 0) {
        const float4 y = *reinterpret_cast<const float4 *>(dkv + s2 * 2 * HD + (e - HD));
        x0 += y.x, x1 += y.y, x2 += y.z, x3 += y.w;
      }
    }
    *reinterpret_cast<uint2 *>(dqkv + item * 4) = make_uint2(pack2<BF16>(x0, x1), pack2<BF16>(x2, x3));
  }
}

// 0 = ok: the checks that need no pointer
int check_attn(int n, int P_cap, int K, int H, int D, int dt) {
  SPX_CHECK(D == 16 || D == 32 || D == 64, "head size must be 16, 32 or 64, got %d", D);
  SPX_CHECK(K >= 32 && K % 32 == 0, "patch_size must be a multiple of 32, got %d", K);
  SPX_CHECK(dt == SPX_F16 || dt == SPX_BF16, "dtype must be f16 or bf16, got %d", dt);
  SPX_CHECK(n >= 0 && P_cap >= 0 && H >= 1, "bad sizes: n %d, P_cap %d, H %d", n, P_cap, H);
  SPX_CHECK(static_cast<long long>(H) * D <= 1 << 20, "H * D too large");
  SPX_CHECK(static_cast<long long>(P_cap) * K < 0x80000000LL, "P_cap * K must stay below 2^31");
  SPX_CHECK((static_cast<long long>(P_cap) * ((K + kOwn - 1) / kOwn)) < 0x7fffffffLL && (H * D + kHW - 1) / kHW <= 65535,
            "too many workgroups");
  return 0;
}

struct AttnWs {
  float *delta, *dkv;
  size_t bytes;
  AttnWs(void *ws, int n, int P_cap, int K, int H, int D) {
    Carver c(ws);
    delta = c.take<float>(static_cast<size_t>(n > 0 ? n : 1) * H);
    dkv = c.take<float>(static_cast<size_t>(P_cap) * K * 2 * H * D + 1);
    bytes = c.off;
  }
};

template <typename F>
void with_attn_instance(int dt, int D, F &&f) {
  dispatch_value<16, 32, 64>(D, [&](auto d) {
    if (dt == SPX_BF16) f(std::true_type{}, d);
    else f(std::false_type{}, d);
  });
}

}  // namespace
}  // namespace spx

extern "C" {

size_t spx_patch_attn_ws_bytes(int n, int P_cap, int K, int H, int D) {
  if (n < 0 || P_cap < 0 || K < 32 || K % 32 || H < 1 || !(D == 16 || D == 32 || D == 64) ||
      static_cast<long long>(P_cap) * K >= 0x80000000LL || static_cast<long long>(H) * D > 1 << 20)
    return 0;
  return spx::AttnWs(nullptr, n, P_cap, K, H, D).bytes;
}

int spx_patch_attn_fwd(const void *qkv, const int32_t *patch_rows, const int32_t *patch_rows_canon, const int32_t *row_slot,
                       const int32_t *n_patches_dev, int n, int P_cap, int K, int H, int D, int dt, float scale, void *out,
                       float *lse, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_attn(n, P_cap, K, H, D, dt)) return rc;
  if (n == 0) return 0;
  SPX_CHECK(qkv && patch_rows && patch_rows_canon && row_slot && n_patches_dev && out && lse, "null pointer");
  SPX_CHECK(aligned_to(qkv, 16) && aligned_to(out, 16) && aligned_to(lse, 4), "qkv / out not aligned to 16 bytes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  AttnArgs a = {};
  a.qkv = static_cast<const uint16_t *>(qkv);
  a.patch_rows = patch_rows, a.patch_rows_canon = patch_rows_canon, a.n_patches = n_patches_dev;
  a.n = n, a.P_cap = P_cap, a.K = K, a.H = H, a.scale = scale;
  a.out_w = static_cast<uint16_t *>(out);
  a.lse = lse;
  const int HD = H * D, pieces = HD / 8;
  const long long total = static_cast<long long>(n) * pieces;
  hipLaunchKernelGGL(attn_dead_rows_kernel, dim3(stream_blocks(total, 256)), dim3(256), 0, s, row_slot,
                     static_cast<long long>(P_cap) * K, total, pieces, static_cast<uint4 *>(out));
  if (P_cap > 0) {
    const dim3 grid(static_cast<unsigned>(P_cap) * ((K + kOwn - 1) / kOwn), (HD + kHW - 1) / kHW);
    with_attn_instance(dt, D, [&](auto bf, auto d) {
      hipLaunchKernelGGL((attn_fwd_kernel<bf, d>), grid, dim3(256), 0, s, a);
    });
  }
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_patch_attn_bwd(const void *qkv, const void *out, const float *lse, const void *d_out, const int32_t *patch_rows,
                       const int32_t *patch_rows_canon, const int32_t *row_slot, const int32_t *row_slot2,
                       const int32_t *n_patches_dev, int n, int P_cap, int K, int H, int D, int dt, float scale, void *dqkv,
                       void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_attn(n, P_cap, K, H, D, dt)) return rc;
  if (n == 0) return 0;
  SPX_CHECK(qkv && out && lse && d_out && patch_rows && patch_rows_canon && row_slot && row_slot2 && n_patches_dev && dqkv,
            "null pointer");
  SPX_CHECK(aligned_to(qkv, 16) && aligned_to(out, 16) && aligned_to(d_out, 16) && aligned_to(dqkv, 16) &&
                aligned_to(lse, 4), "qkv / out / d_out / dqkv not aligned to 16 bytes");
  AttnWs w(ws, n, P_cap, K, H, D);
  SPX_CHECK(ws && ws_bytes >= w.bytes && aligned_to(ws, 16), "workspace too small or misaligned: %zu < %zu", ws_bytes,
            w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  AttnArgs a = {};
  a.qkv = static_cast<const uint16_t *>(qkv);
  a.out = static_cast<const uint16_t *>(out);
  a.d_out = static_cast<const uint16_t *>(d_out);
  a.patch_rows = patch_rows, a.patch_rows_canon = patch_rows_canon, a.n_patches = n_patches_dev;
  a.n = n, a.P_cap = P_cap, a.K = K, a.H = H, a.scale = scale;
  a.out_w = static_cast<uint16_t *>(dqkv);
  a.lse = const_cast<float *>(lse);
  a.delta = w.delta, a.dkv = w.dkv;
  const int HD = H * D;
  const long long heads = static_cast<long long>(n) * H, total = static_cast<long long>(n) * (3 * HD / 4);
  with_attn_instance(dt, D, [&](auto bf, auto d) {
    hipLaunchKernelGGL((attn_delta_kernel<bf, d>), dim3(stream_blocks(heads, 256)), dim3(256), 0, s, a.out, a.d_out, heads,
                       a.delta);
    if (P_cap > 0) {
      const dim3 grid(static_cast<unsigned>(P_cap) * ((K + kOwn - 1) / kOwn), (HD + kHW - 1) / kHW);
      hipLaunchKernelGGL((attn_dq_kernel<bf, d>), grid, dim3(256), 0, s, a);
      hipLaunchKernelGGL((attn_dkv_kernel<bf, d>), grid, dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL((attn_rows_kernel<bf>), dim3(stream_blocks(total, 256)), dim3(256), 0, s, a.dkv, row_slot, row_slot2,
                       static_cast<long long>(P_cap) * K, total, HD, a.out_w);
  });
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
