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
//   bias      the BIAS instances of the three walking kernels (spx_patch_attn_bias_fwd / _bwd) add Point Transformer V3's
//             relative position bias to the logit: sum over the three axes of table[axis][clamp(c_query - c_key)].  The
//             head group's part of the table sits in LDS as [axis][bin][head of the group], times log2 e, so one read
//             serves every head of a pair and the bias joins the log2-domain logit as the addend of one fma.  A lane
//             keeps its own slot's coordinates in registers; a walked block's travel through the stages next to the
//             validity words.  The dQ kernel runs twice: a first walk takes delta = sum P dP (so a query's dS add up to
//             zero), the second is the dQ walk.  The table's gradient is its dS: every wave adds it into a bin array
//             of its own in LDS, the workgroup adds its four arrays in wave order and stores one partial table, and a
//             last launch adds the partials of the live workgroups in a fixed order.  No global atomics.
// Every plan entry is range-checked before it addresses anything.  Grids and loop bounds are host-known.
#include <type_traits>

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

struct AttnBiasArgs : AttnArgs {
  const float *table;                            // [3 * R, H], R = 2 * pos_bnd + 1
  const int32_t *coords;                         // [n, 3]
  int pos_bnd;
  float *dtab_part;                              // [P_cap * ceil(K / 64), 3 * R, Hp], Hp = H rounded up to whole head groups
};
template <bool BIAS>
using ArgsOf = std::conditional_t<BIAS, AttnBiasArgs, AttnArgs>;

constexpr int kCoordBytes = 3 * kWalk * 4;       // a walked block's coordinates in a stage: [axis][slot]
extern __shared__ __attribute__((aligned(16))) char attn_dyn_lds[];      // BIAS: the table, then the dQ kernel's bin arrays

// floats one copy of the head group's table takes in LDS, a multiple of four
__host__ __device__ constexpr int table_floats(int pos_bnd, int HG) { return (3 * (2 * pos_bnd + 1) * HG + 3) & ~3; }

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

// The relative position bias of the BIAS instances: the one copy of its arithmetic, shared by the three walking kernels.
template <int D>
struct Bias {
  static constexpr int HG = kHW / D;
  struct alignas(4 * HG) Heads { float v[HG]; };
  float *tab;                                    // LDS [3 R][HG]: the head group's table times log2 e
  int R, pb, own[3];
  // every thread of the workgroup stages the table (the caller's first barrier publishes it); the lane fetches the
  // coordinates of its own slot's row, which the caller has range-checked
  __device__ __forceinline__ void init(const AttnBiasArgs &a, const Who<D> &w, int own_row) {
    tab = reinterpret_cast<float *>(attn_dyn_lds);
    pb = a.pos_bnd, R = 2 * pb + 1;
    for (int i = threadIdx.x; i < 3 * R * HG; i += 256) {
      const int hh = i % HG;
      tab[i] = hh < w.nh ? a.table[static_cast<size_t>(i / HG) * a.H + w.hg * HG + hh] * kLog2e : 0.f;
    }
    row_coords(a, own_row, own);
  }
  __device__ __forceinline__ static void row_coords(const AttnBiasArgs &a, int row, int (&c)[3]) {
#pragma unroll
    for (int x = 0; x < 3; ++x) c[x] = row >= 0 ? a.coords[static_cast<size_t>(row) * 3 + x] : 0;
  }
  __device__ __forceinline__ static void stash_coords(char *stage_coords, int slot, const int (&c)[3]) {
#pragma unroll
    for (int x = 0; x < 3; ++x) reinterpret_cast<int *>(stage_coords)[x * kWalk + slot] = c[x];
  }
  // the lane's eight pairs (walked slots 16 t + 4 g + r at index 4 t + r): bin of axis x in bits 8 x .. 8 x + 6.
  // The difference is query minus key; it wraps instead of overflowing, and the clamp brings it into the table.
  template <bool OWN_IS_QUERY>
  __device__ __forceinline__ void bins(const char *stage_coords, int g, int (&b)[8]) const {
    const int *cw = reinterpret_cast<const int *>(stage_coords);
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = 0;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const int4 c0 = *reinterpret_cast<const int4 *>(cw + x * kWalk + 4 * g),
                 c1 = *reinterpret_cast<const int4 *>(cw + x * kWalk + 16 + 4 * g);
      const int c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const unsigned q = static_cast<unsigned>(OWN_IS_QUERY ? own[x] : c[i]), k = static_cast<unsigned>(OWN_IS_QUERY ? c[i] : own[x]);
        b[i] |= (min(max(static_cast<int>(q - k), -pb), pb) + pb) << (8 * x);
      }
    }
  }
  __device__ __forceinline__ int entry(int bins, int x) const { return (x * R + ((bins >> (8 * x)) & 0xff)) * HG; }
  // the bias of one pair for every head of the group, in the log2 domain: three LDS reads, added in axis order
  __device__ __forceinline__ void of(int bins, float (&out)[HG]) const {
    const Heads t0 = *reinterpret_cast<const Heads *>(tab + entry(bins, 0)), t1 = *reinterpret_cast<const Heads *>(tab + entry(bins, 1)),
                t2 = *reinterpret_cast<const Heads *>(tab + entry(bins, 2));
#pragma unroll
    for (int hh = 0; hh < HG; ++hh) out[hh] = (t0.v[hh] + t1.v[hh]) + t2.v[hh];
  }
  // Up to two heads per group, the biases of a block's eight pairs are read ahead of the loop over the heads.  With four
  // (D = 16) they would hold 32 registers through that loop and cost a workgroup or two per CU: there a head reads its
  // own three words of the same entries when it needs them.  The sum is the same either way.
  static constexpr bool kAhead = HG < 4;
  template <bool OWN_IS_QUERY>
  __device__ __forceinline__ void block(const char *stage_coords, int g, int (&b)[8], float (&out)[8][HG]) const {
    bins<OWN_IS_QUERY>(stage_coords, g, b);
    if constexpr (kAhead) {
#pragma unroll
      for (int i = 0; i < 8; ++i) of(b[i], out[i]);
    }
  }
  __device__ __forceinline__ float at(int bins, const float (&ahead)[HG], int hh) const {
    if constexpr (kAhead) return ahead[hh];
    else return (tab[entry(bins, 0) + hh] + tab[entry(bins, 1) + hh]) + tab[entry(bins, 2) + hh];
  }
};

// the log2-domain logit of a pair: one fma in every kernel, so the backward's P matches the forward's lse
template <bool BIAS, int D, int HG>
__device__ __forceinline__ float logit2(float s, float sl2, const Bias<D> &rb, int bins, const float (&ahead)[HG], int hh) {
  if constexpr (BIAS) return __builtin_fmaf(s, sl2, rb.at(bins, ahead, hh));
  else return s * sl2;
}

// ---------------------------------------------------------------------------------------------------- forward
template <bool BF16, int D, bool BIAS>
__global__ void __launch_bounds__(256) attn_fwd_kernel(ArgsOf<BIAS> a) {
  using W = Who<D>;
  constexpr int HG = W::HG, DC = W::DC, DT = W::DT;
  constexpr int kFlags = kRmBytes + kTrBytes, kCoords = kFlags + kWalk * 4;
  constexpr int kStage = kCoords + (BIAS ? kCoordBytes : 0);
  __shared__ __attribute__((aligned(16))) char lds[2][kStage];
  const W w(a);
  if (!w.live) return;
  const int j = w.j, g = w.g;
  int qrow = -1;
  if (w.wave_on) qrow = checked_row(a.patch_rows_canon, w.base + w.own0 + j, a.n);
  uint4 qf[HG][DC];
  w.own_frags(a.qkv + w.at(qrow < 0 ? 0 : qrow, 0), qrow >= 0, qf);
  [[maybe_unused]] Bias<D> rb;
  if constexpr (BIAS) rb.init(a, w, qrow);

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
  [[maybe_unused]] int kc[3];
  auto fetch = [&](int blk) {
    krow = checked_row(a.patch_rows, w.base + blk * kWalk + w.sl, a.n);
    const bool ok = krow >= 0 && w.pc_on;
    const uint16_t *rp = a.qkv + w.at(krow < 0 ? 0 : krow, 1) + w.pc * 8;
    kr = load16(rp, ok);
    vr = load16(rp + w.HD, ok);
    if constexpr (BIAS)
      if (w.pc == 0) rb.row_coords(a, krow, kc);
  };
  auto stash = [&](int buf) {
    stage_rm(lds[buf], w.sl, w.pc, kr);
    stage_tr(lds[buf] + kRmBytes, w.sl, w.pc, vr);
    if (w.pc == 0) {
      reinterpret_cast<int *>(lds[buf] + kFlags)[w.sl] = krow >= 0 ? 1 : 0;
      if constexpr (BIAS) rb.stash_coords(lds[buf] + kCoords, w.sl, kc);
    }
  };
  fetch(0);
  stash(0);
  __syncthreads();
  for (int blk = 0; blk < nblk; ++blk) {
    const int buf = blk & 1;
    if (blk + 1 < nblk) fetch(blk + 1);
    if (w.wave_on) {
      const char *krm = lds[buf], *vtr = lds[buf] + kRmBytes;
      const int *kval = reinterpret_cast<const int *>(lds[buf] + kFlags);
      const int4 v0 = *reinterpret_cast<const int4 *>(kval + 4 * g), v1 = *reinterpret_cast<const int4 *>(kval + 16 + 4 * g);
      const bool kv[8] = {v0.x != 0, v0.y != 0, v0.z != 0, v0.w != 0, v1.x != 0, v1.y != 0, v1.z != 0, v1.w != 0};
      [[maybe_unused]] int bin[8];
      [[maybe_unused]] float bias[8][HG];
      if constexpr (BIAS) rb.template block<true>(lds[buf] + kCoords, g, bin, bias);
#pragma unroll
      for (int hh = 0; hh < HG; ++hh) {
        if (hh < w.nh) {
          float x[8];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const f32x4 s = dot_tile<BF16, D>(krm, 16 * t + j, hh, g, qf[hh]);
#pragma unroll
            for (int r = 0; r < 4; ++r) x[4 * t + r] = kv[4 * t + r] ? logit2<BIAS>(s[r], sl2, rb, bin[4 * t + r], bias[4 * t + r], hh) : -INFINITY;
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
// BIAS runs it twice.  PASS 0 only takes delta = sum_j P dP, from the very P and dP that PASS 1 forms dS of, so a query's
// dS add up to zero as they must: delta = rowsum(dO * out) carries the rounding of the 16-bit out as an error common to
// all dS of a query, and a bin of the table adds it over thousands of pairs.  PASS 0 writes delta for PASS 1 and for the
// dK/dV kernel (one writer per (row, head)); the delta launch is not run.
template <bool BF16, int D, bool BIAS, int PASS = 1>
__global__ void __launch_bounds__(256) attn_dq_kernel(ArgsOf<BIAS> a) {
  static_assert(BIAS || PASS == 1, "the unbiased backward takes delta from its own launch");
  constexpr int pass = PASS;
  using W = Who<D>;
  constexpr int HG = W::HG, DC = W::DC, DT = W::DT;
  constexpr int kFlags = 2 * kRmBytes + kTrBytes, kCoords = kFlags + kWalk * 4;
  constexpr int kStage = kCoords + (BIAS ? kCoordBytes : 0);
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
  // BIAS: behind the table in LDS lie four arrays of its layout, one per wave, which take the wave's dS per bin
  [[maybe_unused]] Bias<D> rb;
  [[maybe_unused]] float *wave_bins = nullptr;
  if constexpr (BIAS) {
    rb.init(a, w, qrow);
    if constexpr (pass == 1) {
      const int tf = table_floats(a.pos_bnd, HG);
      for (int i = threadIdx.x; i < 4 * tf; i += 256) rb.tab[tf + i] = 0.f;
      wave_bins = rb.tab + tf * (1 + w.wave);
    }
  }
  // BIAS: a difference beyond pos_bnd lands in the first or the last bin of its axis, and where patches are wide most
  // pairs do: a lane adds those dS in registers (edge[head][axis][side]) and only the bins between go to LDS, where the
  // colliding lanes of one add are taken one after the other.
  [[maybe_unused]] float edge[HG][3][2] = {};
  float lse2[HG], dl[HG];
  f32x4 dq[HG][DT];
#pragma unroll
  for (int hh = 0; hh < HG; ++hh) {
    const bool ok = qrow >= 0 && hh < w.nh;
    const int h = w.hg * HG + (ok ? hh : 0);
    lse2[hh] = ok ? a.lse[static_cast<size_t>(w.base + w.own0 + j) * a.H + h] * kLog2e : INFINITY;
    dl[hh] = ok && pass == 1 ? a.delta[static_cast<size_t>(qr0) * a.H + h] : 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[hh][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float sl2 = a.scale * kLog2e;
  const int nblk = a.K / kWalk;
  uint4 kr, vr;
  int krow;
  [[maybe_unused]] int kc[3];
  auto fetch = [&](int blk) {
    krow = checked_row(a.patch_rows, w.base + blk * kWalk + w.sl, a.n);
    const bool ok = krow >= 0 && w.pc_on;
    const uint16_t *rp = a.qkv + w.at(krow < 0 ? 0 : krow, 1) + w.pc * 8;
    kr = load16(rp, ok);
    vr = load16(rp + w.HD, ok);
    if constexpr (BIAS)
      if (w.pc == 0) rb.row_coords(a, krow, kc);
  };
  auto stash = [&](int buf) {
    stage_rm(lds[buf], w.sl, w.pc, kr);
    stage_rm(lds[buf] + kRmBytes, w.sl, w.pc, vr);
    if constexpr (pass == 1) stage_tr(lds[buf] + 2 * kRmBytes, w.sl, w.pc, kr);
    if (w.pc == 0) {
      reinterpret_cast<int *>(lds[buf] + kFlags)[w.sl] = krow >= 0 ? 1 : 0;
      if constexpr (BIAS) rb.stash_coords(lds[buf] + kCoords, w.sl, kc);
    }
  };
  fetch(0);
  stash(0);
  __syncthreads();
  for (int blk = 0; blk < nblk; ++blk) {
    const int buf = blk & 1;
    if (blk + 1 < nblk) fetch(blk + 1);
    if (w.wave_on) {
      const char *krm = lds[buf], *vrm = lds[buf] + kRmBytes, *ktr = lds[buf] + 2 * kRmBytes;
      const int *kval = reinterpret_cast<const int *>(lds[buf] + kFlags);
      const int4 v0 = *reinterpret_cast<const int4 *>(kval + 4 * g), v1 = *reinterpret_cast<const int4 *>(kval + 16 + 4 * g);
      const bool kv[8] = {v0.x != 0, v0.y != 0, v0.z != 0, v0.w != 0, v1.x != 0, v1.y != 0, v1.z != 0, v1.w != 0};
      [[maybe_unused]] int bin[8];
      [[maybe_unused]] float bias[8][HG];
      if constexpr (BIAS) rb.template block<true>(lds[buf] + kCoords, g, bin, bias);
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
              const float pr =
                  kv[4 * t + r] ? __builtin_amdgcn_exp2f(logit2<BIAS>(s[r], sl2, rb, bin[4 * t + r], bias[4 * t + r], hh) - lse2[hh]) : 0.f;
              ds[4 * t + r] = pass == 0 ? pr * dp[r] : pr * (dp[r] - dl[hh]);
            }
          }
          if constexpr (pass == 0) {             // (a lane's partial of delta; the four lanes of a slot are added below)
#pragma unroll
            for (int i = 0; i < 8; ++i) dl[hh] += ds[i];
          } else {
            if constexpr (BIAS) {                // dTable: the fp32 dS, before it is rounded for the dQ product
#pragma unroll
              for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                  const int b = (bin[i] >> (8 * x)) & 0xff;
                  edge[hh][x][0] += b == 0 ? ds[i] : 0.f;
                  edge[hh][x][1] += b == 2 * rb.pb ? ds[i] : 0.f;
                  if (b != 0 && b != 2 * rb.pb)
                    __hip_atomic_fetch_add(wave_bins + rb.entry(bin[i], x) + hh, ds[i], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            const uint4 db = pack8<BF16>(ds);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
              dq[hh][dt] = mfma16<BF16>(frag_tr(ktr, hh * D + 16 * dt + j, g), db, dq[hh][dt]);
          }
        }
      }
    }
    if (blk + 1 < nblk) stash(buf ^ 1);
    __syncthreads();
  }
  if constexpr (pass == 0) {
#pragma unroll
    for (int hh = 0; hh < HG; ++hh) {
      dl[hh] = quad_sum(dl[hh]);
      if (g == 0 && qrow >= 0 && hh < w.nh) a.delta[static_cast<size_t>(qrow) * a.H + w.hg * HG + hh] = dl[hh];
    }
    return;
  }
  if constexpr (BIAS && pass == 1) {
    // the edge bins of the wave's array were never added to: they take the sum of the lanes' registers, a butterfly of
    // fixed order.  Behind the barrier the workgroup's partial table is its four arrays added in wave order, stored
    // whole (a wave beyond K and the heads beyond H left zeros)
#pragma unroll
    for (int hh = 0; hh < HG; ++hh)
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int side = 0; side < 2; ++side) {
          float v = edge[hh][x][side];
#pragma unroll
          for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
          if (w.lane == 0) wave_bins[(x * rb.R + side * 2 * rb.pb) * HG + hh] = v;
        }
    __syncthreads();
    const int tf = table_floats(a.pos_bnd, HG), Hp = gridDim.y * HG;
    float *part = a.dtab_part + static_cast<size_t>(blockIdx.x) * 3 * rb.R * Hp + w.hg * HG;
    for (int i = threadIdx.x; i < 3 * rb.R * HG; i += 256) {
      const float *b = rb.tab + tf + i;
      part[static_cast<size_t>(i / HG) * Hp + i % HG] = ((b[0] + b[tf]) + b[2 * tf]) + b[3 * tf];
    }
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

// dTable [3 R, H] = the partial tables of the live workgroups (patches below the device-side count), added in a fixed
// order: 1024 threads take 16 entries x 64 contiguous chunks of workgroups, a thread adds its chunk in ascending
// workgroup index, and the chunks are added in ascending order.  Written whole; a bin no pair reaches is +0.
__global__ void __launch_bounds__(1024)
attn_dtable_kernel(const float *__restrict__ part, const int32_t *__restrict__ n_patches, int P_cap, int nob, int entries,
                   int Hp, int H, float *__restrict__ dtab) {
  __shared__ float red[64][16];
  const int el = threadIdx.x & 15, chunk = threadIdx.x >> 4, e = blockIdx.x * 16 + el;
  const int live = min(max(*n_patches, 0), P_cap) * nob, per = (live + 63) / 64;
  float acc = 0.f;
  if (e < entries)
    for (int wg = chunk * per; wg < min(live, (chunk + 1) * per); ++wg) acc += part[static_cast<size_t>(wg) * entries + e];
  red[chunk][el] = acc;
  __syncthreads();
  if (chunk != 0 || e >= entries || e % Hp >= H) return;
  float total = 0.f;
  for (int c = 0; c < 64; ++c) total += red[c][el];
  dtab[static_cast<size_t>(e / Hp) * H + e % Hp] = total;
}

// own slots = keys; walks the canonical queries.  Stage: Q and dO row-major (S, dP) and transposed (dK^T, dV^T), and
// per (head, query) the log-sum-exp (+inf for a slot that is no query: its P is zero) and delta.
template <bool BF16, int D, bool BIAS>
__global__ void __launch_bounds__(256) attn_dkv_kernel(ArgsOf<BIAS> a) {
  using W = Who<D>;
  constexpr int HG = W::HG, DC = W::DC, DT = W::DT;
  constexpr int kTiles = 2 * kRmBytes + 2 * kTrBytes, kCoords = kTiles + 2 * HG * kWalk * 4;
  constexpr int kStage = kCoords + (BIAS ? kCoordBytes : 0);
  __shared__ __attribute__((aligned(16))) char lds[2][kStage];
  const W w(a);
  if (!w.live) return;
  const int j = w.j, g = w.g, tid = threadIdx.x;
  int krow = -1;
  if (w.wave_on) krow = checked_row(a.patch_rows, w.base + w.own0 + j, a.n);
  uint4 kf[HG][DC], vf[HG][DC];
  w.own_frags(a.qkv + w.at(krow < 0 ? 0 : krow, 1), krow >= 0, kf);
  w.own_frags(a.qkv + w.at(krow < 0 ? 0 : krow, 2), krow >= 0, vf);
  [[maybe_unused]] Bias<D> rb;
  if constexpr (BIAS) rb.init(a, w, krow);
  f32x4 dk[HG][DT], dv[HG][DT];
#pragma unroll
  for (int hh = 0; hh < HG; ++hh)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dk[hh][dt] = dv[hh][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = a.scale * kLog2e;
  const int nblk = a.K / kWalk;
  uint4 qr, dor;
  float lr = INFINITY, dr = 0.f;
  [[maybe_unused]] int qc[3];
  auto fetch = [&](int blk) {
    const int row = checked_row(a.patch_rows_canon, w.base + blk * kWalk + w.sl, a.n);
    const bool ok = row >= 0 && w.pc_on;
    const int r0 = row < 0 ? 0 : row;
    qr = load16(a.qkv + w.at(r0, 0) + w.pc * 8, ok);
    dor = load16(a.d_out + static_cast<size_t>(r0) * w.HD + w.hg * kHW + w.pc * 8, ok);
    if constexpr (BIAS)
      if (w.pc == 0) rb.row_coords(a, row, qc);
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
    if constexpr (BIAS)
      if (w.pc == 0) rb.stash_coords(lds[buf] + kCoords, w.sl, qc);
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
      [[maybe_unused]] int bin[8];
      [[maybe_unused]] float bias[8][HG];
      if constexpr (BIAS) rb.template block<false>(lds[buf] + kCoords, g, bin, bias);
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
              pr[4 * t + r] = __builtin_amdgcn_exp2f(logit2<BIAS>(s[r], sl2, rb, bin[4 * t + r], bias[4 * t + r], hh) - Lr[r]);
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

// the bias arguments of a call, or none
struct BiasHost {
  const float *table;
  const int32_t *coords;
  int pos_bnd;
  float *d_table, *part;
};

// bytes of the partial tables of a biased backward: one table of [3 R, Hp] per workgroup column of the dQ grid
size_t dtable_ws_bytes(int P_cap, int K, int H, int D, int pos_bnd) {
  const size_t Hp = static_cast<size_t>((H * D + kHW - 1) / kHW) * (kHW / D);
  return align_up((static_cast<size_t>(P_cap) * ((K + kOwn - 1) / kOwn) * 3 * (2 * pos_bnd + 1) * Hp + 1) * sizeof(float), 256);
}

int check_bias(const BiasHost &b, int P_cap, int K, int H, int D) {
  SPX_CHECK(b.pos_bnd >= 1 && b.pos_bnd <= 63, "pos_bnd must lie in 1 .. 63, got %d", b.pos_bnd);
  SPX_CHECK(dtable_ws_bytes(P_cap, K, H, D, b.pos_bnd) < (static_cast<size_t>(1) << 40), "bias workspace too large");
  return 0;
}

// LDS behind the static stages: the table (and, in the dQ kernel, the four waves' bin arrays)
size_t bias_lds_bytes(int pos_bnd, int D, int copies) { return static_cast<size_t>(table_floats(pos_bnd, kHW / D)) * 4 * copies; }

int attn_fwd(const void *qkv, const int32_t *patch_rows, const int32_t *patch_rows_canon, const int32_t *row_slot,
             const int32_t *n_patches_dev, int n, int P_cap, int K, int H, int D, int dt, float scale, void *out, float *lse,
             const BiasHost *bias, spx_stream_t stream) {
  if (int rc = check_attn(n, P_cap, K, H, D, dt)) return rc;
  if (bias)
    if (int rc = check_bias(*bias, P_cap, K, H, D)) return rc;
  if (n == 0) return 0;
  SPX_CHECK(qkv && patch_rows && patch_rows_canon && row_slot && n_patches_dev && out && lse, "null pointer");
  SPX_CHECK(aligned_to(qkv, 16) && aligned_to(out, 16) && aligned_to(lse, 4), "qkv / out not aligned to 16 bytes");
  SPX_CHECK(!bias || (bias->table && bias->coords && aligned_to(bias->table, 4) && aligned_to(bias->coords, 4)),
            "rel_bias / coords null or misaligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  AttnBiasArgs a = {};
  a.qkv = static_cast<const uint16_t *>(qkv);
  a.patch_rows = patch_rows, a.patch_rows_canon = patch_rows_canon, a.n_patches = n_patches_dev;
  a.n = n, a.P_cap = P_cap, a.K = K, a.H = H, a.scale = scale;
  a.out_w = static_cast<uint16_t *>(out);
  a.lse = lse;
  if (bias) a.table = bias->table, a.coords = bias->coords, a.pos_bnd = bias->pos_bnd;
  const int HD = H * D, pieces = HD / 8;
  const long long total = static_cast<long long>(n) * pieces;
  hipLaunchKernelGGL(attn_dead_rows_kernel, dim3(stream_blocks(total, 256)), dim3(256), 0, s, row_slot,
                     static_cast<long long>(P_cap) * K, total, pieces, static_cast<uint4 *>(out));
  if (P_cap > 0) {
    const dim3 grid(static_cast<unsigned>(P_cap) * ((K + kOwn - 1) / kOwn), (HD + kHW - 1) / kHW);
    with_attn_instance(dt, D, [&](auto bf, auto d) {
      if (bias)
        hipLaunchKernelGGL((attn_fwd_kernel<bf, d, true>), grid, dim3(256), bias_lds_bytes(a.pos_bnd, D, 1), s, a);
      else
        hipLaunchKernelGGL((attn_fwd_kernel<bf, d, false>), grid, dim3(256), 0, s, static_cast<const AttnArgs &>(a));
    });
  }
  SPX_LAUNCH_CHECK();
  return 0;
}

int attn_bwd(const void *qkv, const void *out, const float *lse, const void *d_out, const int32_t *patch_rows,
             const int32_t *patch_rows_canon, const int32_t *row_slot, const int32_t *row_slot2, const int32_t *n_patches_dev,
             int n, int P_cap, int K, int H, int D, int dt, float scale, void *dqkv, void *ws, size_t ws_bytes,
             const BiasHost *bias, size_t part_bytes, spx_stream_t stream) {
  if (int rc = check_attn(n, P_cap, K, H, D, dt)) return rc;
  if (bias)
    if (int rc = check_bias(*bias, P_cap, K, H, D)) return rc;
  if (n == 0) return 0;
  SPX_CHECK(qkv && out && lse && d_out && patch_rows && patch_rows_canon && row_slot && row_slot2 && n_patches_dev && dqkv,
            "null pointer");
  SPX_CHECK(aligned_to(qkv, 16) && aligned_to(out, 16) && aligned_to(d_out, 16) && aligned_to(dqkv, 16) &&
                aligned_to(lse, 4), "qkv / out / d_out / dqkv not aligned to 16 bytes");
  AttnWs w(ws, n, P_cap, K, H, D);
  SPX_CHECK(ws && ws_bytes >= w.bytes && aligned_to(ws, 16), "workspace too small or misaligned: %zu < %zu", ws_bytes,
            w.bytes);
  if (bias) {
    SPX_CHECK(bias->table && bias->coords && bias->d_table && aligned_to(bias->table, 4) && aligned_to(bias->coords, 4) &&
                  aligned_to(bias->d_table, 4), "rel_bias / coords / d_rel_bias null or misaligned");
    SPX_CHECK(bias->part && aligned_to(bias->part, 16) && part_bytes >= dtable_ws_bytes(P_cap, K, H, D, bias->pos_bnd),
              "bias workspace too small or misaligned: %zu < %zu", part_bytes, dtable_ws_bytes(P_cap, K, H, D, bias->pos_bnd));
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  AttnBiasArgs a = {};
  a.qkv = static_cast<const uint16_t *>(qkv);
  a.out = static_cast<const uint16_t *>(out);
  a.d_out = static_cast<const uint16_t *>(d_out);
  a.patch_rows = patch_rows, a.patch_rows_canon = patch_rows_canon, a.n_patches = n_patches_dev;
  a.n = n, a.P_cap = P_cap, a.K = K, a.H = H, a.scale = scale;
  a.out_w = static_cast<uint16_t *>(dqkv);
  a.lse = const_cast<float *>(lse);
  a.delta = w.delta, a.dkv = w.dkv;
  if (bias) a.table = bias->table, a.coords = bias->coords, a.pos_bnd = bias->pos_bnd, a.dtab_part = bias->part;
  const int HD = H * D, nob = (K + kOwn - 1) / kOwn, nhg = (HD + kHW - 1) / kHW;
  const long long heads = static_cast<long long>(n) * H, total = static_cast<long long>(n) * (3 * HD / 4);
  with_attn_instance(dt, D, [&](auto bf, auto d) {
    if (!bias)
      hipLaunchKernelGGL((attn_delta_kernel<bf, d>), dim3(stream_blocks(heads, 256)), dim3(256), 0, s, a.out, a.d_out, heads,
                         a.delta);
    if (P_cap > 0) {
      const dim3 grid(static_cast<unsigned>(P_cap) * nob, nhg);
      if (bias) {
        hipLaunchKernelGGL((attn_dq_kernel<bf, d, true, 0>), grid, dim3(256), bias_lds_bytes(a.pos_bnd, D, 1), s, a);
        hipLaunchKernelGGL((attn_dq_kernel<bf, d, true, 1>), grid, dim3(256), bias_lds_bytes(a.pos_bnd, D, 5), s, a);
        hipLaunchKernelGGL((attn_dkv_kernel<bf, d, true>), grid, dim3(256), bias_lds_bytes(a.pos_bnd, D, 1), s, a);
      } else {
        hipLaunchKernelGGL((attn_dq_kernel<bf, d, false>), grid, dim3(256), 0, s, static_cast<const AttnArgs &>(a));
        hipLaunchKernelGGL((attn_dkv_kernel<bf, d, false>), grid, dim3(256), 0, s, static_cast<const AttnArgs &>(a));
      }
    }
    hipLaunchKernelGGL((attn_rows_kernel<bf>), dim3(stream_blocks(total, 256)), dim3(256), 0, s, a.dkv, row_slot, row_slot2,
                       static_cast<long long>(P_cap) * K, total, HD, a.out_w);
  });
  if (bias) {
    const int Hp = nhg * (kHW / D), entries = 3 * (2 * a.pos_bnd + 1) * Hp;
    hipLaunchKernelGGL(attn_dtable_kernel, dim3((entries + 15) / 16), dim3(1024), 0, s, a.dtab_part, n_patches_dev, P_cap, nob,
                       entries, Hp, H, bias->d_table);
  }
  SPX_LAUNCH_CHECK();
  return 0;
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

size_t spx_patch_attn_bias_ws_bytes(int P_cap, int K, int H, int D, int pos_bnd) {
  if (spx_patch_attn_ws_bytes(0, P_cap, K, H, D) == 0 || pos_bnd < 1 || pos_bnd > 63) return 0;
  return spx::dtable_ws_bytes(P_cap, K, H, D, pos_bnd);
}

int spx_patch_attn_fwd(const void *qkv, const int32_t *patch_rows, const int32_t *patch_rows_canon, const int32_t *row_slot,
                       const int32_t *n_patches_dev, int n, int P_cap, int K, int H, int D, int dt, float scale, void *out,
                       float *lse, spx_stream_t stream) {
  return spx::attn_fwd(qkv, patch_rows, patch_rows_canon, row_slot, n_patches_dev, n, P_cap, K, H, D, dt, scale, out, lse,
                       nullptr, stream);
}

int spx_patch_attn_bwd(const void *qkv, const void *out, const float *lse, const void *d_out, const int32_t *patch_rows,
                       const int32_t *patch_rows_canon, const int32_t *row_slot, const int32_t *row_slot2,
                       const int32_t *n_patches_dev, int n, int P_cap, int K, int H, int D, int dt, float scale, void *dqkv,
                       void *ws, size_t ws_bytes, spx_stream_t stream) {
  return spx::attn_bwd(qkv, out, lse, d_out, patch_rows, patch_rows_canon, row_slot, row_slot2, n_patches_dev, n, P_cap, K, H,
                       D, dt, scale, dqkv, ws, ws_bytes, nullptr, 0, stream);
}

int spx_patch_attn_bias_fwd(const void *qkv, const int32_t *patch_rows, const int32_t *patch_rows_canon,
                            const int32_t *row_slot, const int32_t *n_patches_dev, const float *rel_bias,
                            const int32_t *coords, int n, int P_cap, int K, int H, int D, int dt, float scale, int pos_bnd,
                            void *out, float *lse, spx_stream_t stream) {
  const spx::BiasHost b = {rel_bias, coords, pos_bnd, nullptr, nullptr};
  return spx::attn_fwd(qkv, patch_rows, patch_rows_canon, row_slot, n_patches_dev, n, P_cap, K, H, D, dt, scale, out, lse, &b,
                       stream);
}

int spx_patch_attn_bias_bwd(const void *qkv, const void *out, const float *lse, const void *d_out, const int32_t *patch_rows,
                            const int32_t *patch_rows_canon, const int32_t *row_slot, const int32_t *row_slot2,
                            const int32_t *n_patches_dev, const float *rel_bias, const int32_t *coords, int n, int P_cap, int K,
                            int H, int D, int dt, float scale, int pos_bnd, void *dqkv, float *d_rel_bias, void *ws,
                            size_t ws_bytes, void *bias_ws, size_t bias_ws_bytes, spx_stream_t stream) {
  const spx::BiasHost b = {rel_bias, coords, pos_bnd, d_rel_bias, static_cast<float *>(bias_ws)};
  return spx::attn_bwd(qkv, out, lse, d_out, patch_rows, patch_rows_canon, row_slot, row_slot2, n_patches_dev, n, P_cap, K, H,
                       D, dt, scale, dqkv, ws, ws_bytes, &b, bias_ws_bytes, stream);
}

}  // extern "C"
