// Selective scan (Mamba's S6 recurrence) and the short causal depthwise convolution in front of it, over RAGGED
// sequences of rows read through an order (spx_selective_scan_fwd / _bwd, spx_causal_conv_rows_fwd / _bwd): the hot
// path of the state-space backbones that serialise voxels along a curve.  Rows stay in row order, channel-last, as a
// Linear leaves them; no padded [B, Dm, L] copy exists.
//
// Matrix instructions do not fit: the recurrence is elementwise in (row, channel, state).  Per row and channel the
// forward issues 16 exp2 and 16 * 4 multiply-adds and moves 3 elements (u, delta, z) in and one out; the bound is the
// issue of exp2 and FMAs, not the gather (DESIGN 3.42 has the counts).
//
//   CHUNKS      the sequential dimension is long (100 000 rows) and the parallel one short (scenes x channels), so a
//               sequence is cut into chunks of kChunk positions that start on sequence boundaries: at most n / kChunk +
//               S, host-known.  scan_table_kernel (one workgroup) writes {first position, length, sequence} per chunk
//               and the count in use; every later grid covers the capacity and exits early beyond the count.
//   FORWARD     scan_walk_kernel<.., kEnd>: one wave per (chunk, 64 channels), a channel per lane, 16 states in
//               registers, from a zero state: leaves sum dt and the end states (the chunk's decay is exp(A * sum dt): no
//               product of exponentials is stored).  scan_carry_kernel: a thread per (sequence, channel, state) walks
//               the chunks in order and replaces each end state by the chunk's ENTRY state.  scan_walk_kernel<.., kOut>:
//               the same walk from the entry state, writing y.
//   ROWS        a chunk's rows are found through `order` once (lane t holds the row of step t, broadcast by readlane);
//               a wave's load of u / delta / z is one contiguous 128-byte row piece (2 bytes a lane), kRowsAhead rows'
//               loads are issued together ahead of the dependent chain; B[r, g, :] and C[r, g, :] are uniform over the
//               wave and are read as broadcasts.  (Not staged through LDS: with a channel per lane a row piece IS the
//               wave's register, and eight waves a SIMD hide the gather.)
//   BACKWARD    scan_walk_kernel<.., kAdj>: the chunk's adjoint from zero, walked back (needs no state).  The carry in
//               reverse gives every chunk the adjoint that enters it from the later chunks.  scan_bwd_kernel: a
//               workgroup per (chunk, group) walks the group's channels eight at a time, a lane per (channel, state):
//               16 states are one DPP row, so the sums over states (du, ddelta, the recomputed y of dz) are row
//               reductions in registers.  The chunk is recomputed forward from its entry state with every h_t kept in
//               VGPRs (kChunk of them), then walked back with g_t = C_t dy'_t + a_{t+1} g_{t+1}.  Per-channel values
//               (dt, u, dy') are staged as fp32 in LDS by 16-byte row pieces and read as broadcasts.  dB / dC are
//               summed over a group's channels across lanes, then per wave in LDS, over the channel steps in order, and
//               stored once: one workgroup owns a group.  dA, dD and ddelta_bias leave one fp32 partial per chunk (dA in
//               the slot its lane read the adjoint from); reduce_cols_kernel adds them in a fixed order.
//   DEAD ROWS   dead_rows_kernel zeroes the rows of the positions of no sequence ahead of each walk.
//   CONVOLUTION conv_fwd_kernel: a thread per (position, 16-byte piece), W taps gathered through the order.  Backward:
//               conv_bwd_pre_kernel writes d_pre per POSITION (fp32) and one partial of dweight / dbias per workgroup,
//               conv_bwd_x_kernel gathers dx from it, reduce_cols_kernel adds the partials.
//
// Every order entry is range-checked before it addresses anything, offsets are clamped; loops are bounded by kChunk, by
// the chunk capacity or by S; no spin, grid barrier, cooperative launch, memset or atomic.
#include <cmath>

#include "piece.h"

namespace spx {
namespace {

constexpr int kChunk = SPX_SCAN_CHUNK;
constexpr int kStates = SPX_SCAN_STATES;
constexpr int kChBlock = 64;                      // channels of a forward workgroup (one wave)
constexpr int kMaxDm = 2048;
constexpr int kRowsAhead = 4;                     // rows whose loads are issued together in the forward walks
constexpr int kBwdCh = 8;                         // channels of one step of the backward workgroup
constexpr int kBwdThreads = kBwdCh * kStates;     // 128: a lane per (channel, state)
constexpr int kBwdWaves = kBwdThreads / kWave;
constexpr int kRedCols = 16, kRedLanes = 16;      // reduce_cols_kernel: 16 columns x 16 partial-row lanes
constexpr int kConvRows = 128, kConvLanes = 4;    // positions of a conv_bwd_pre workgroup, position lanes per channel
constexpr int kMaxW = 4;
constexpr float kLog2e = 1.4426950408889634f;
constexpr int kEnd = 0, kOut = 1, kAdj = 2;       // roles of scan_walk_kernel

static_assert(kChunk == kWave, "lane t of a forward wave holds the row of step t");

struct Seq {                                      // how positions become rows
  const int32_t *order, *offsets;
  int n, S, step;
};

struct Ws {                                       // the carve of the scan's workspace
  int32_t *hdr;                                   // [0]: chunks in use
  int32_t *seq_chunk0;                            // [S + 1]: first chunk of every sequence
  int4 *table;                                    // [cap]: {first position walked, length, sequence, -}
  float *sumdt;                                   // [cap, Dm]
  float *H;                                       // [cap, 16, Dm]: end states, then entry states
  float *Gs;                                      // [cap, 16, Dm]: adjoints, then the dA partials
  float *pD;                                      // [cap, 2, Dm]: partials of dD and ddelta_bias
  size_t bytes;
};

inline int scan_cap(int n, int S) { return n / kChunk + S; }

inline Ws carve_scan(void *ws, int n, int S, int Dm) {
  const size_t cap = static_cast<size_t>(scan_cap(n, S));
  Carver c(ws);
  Ws w;
  w.hdr = c.take<int32_t>(64);
  w.seq_chunk0 = c.take<int32_t>(static_cast<size_t>(S) + 1);
  w.table = c.take<int4>(cap);
  w.sumdt = c.take<float>(cap * Dm);
  w.H = c.take<float>(cap * kStates * Dm);
  w.Gs = c.take<float>(cap * kStates * Dm);
  w.pD = c.take<float>(cap * 2 * Dm);
  w.bytes = c.off;
  return w;
}

struct ScanArgs {
  const void *u, *delta, *z, *B, *C, *dout;
  const float *A, *D, *bias;
  Seq seq;
  int Dm, G, softplus;
  const int32_t *hdr;
  const int4 *table;
  float *sumdt, *H, *Gs, *pD;
  void *y, *du, *ddelta, *dz, *dB, *dC;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// [beg, end) of sequence s, inside [0, n] and ordered whatever offsets holds
__device__ __forceinline__ void seq_range(const int32_t *__restrict__ offsets, int s, int n, int &beg, int &end) {
  beg = clampi(offsets[s], 0, n);
  end = clampi(offsets[s + 1], beg, n);
}

// row of position p, -1 when the position or its entry is out of range
__device__ __forceinline__ int row_at(const Seq &q, int p) {
  if (static_cast<unsigned>(p) >= static_cast<unsigned>(q.n)) return -1;
  const int r = q.order ? q.order[p] : p;
  return static_cast<unsigned>(r) < static_cast<unsigned>(q.n) ? r : -1;
}

// sequence of position p by bisection over the clamped offsets, -1 for a position of no sequence
__device__ __forceinline__ int seq_of(const Seq &q, int p, int &beg, int &end) {
  int lo = 0, hi = q.S;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (clampi(q.offsets[mid + 1], 0, q.n) <= p) lo = mid + 1;
    else hi = mid;
  }
  beg = end = 0;
  if (lo >= q.S) return -1;
  seq_range(q.offsets, lo, q.n, beg, end);
  return (p >= beg && p < end) ? lo : -1;
}

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }
// a step's decay exp(dt * A): 16-bit rows, the hot path, take one multiply and v_exp_f32 on A * log2(e) (its 2 ulp are far
// below their roundoff); fp32 rows take the product and the exponential in double, rounded once: with the library's
// fp32 exp two gradients of 384 missed the fp32 criterion by 2 and 4 %
template <int DT> __device__ __forceinline__ float a_scaled(float A) { return DT == SPX_F32 ? A : A * kLog2e; }
template <int DT> __device__ __forceinline__ float decay(float dt, float As) {
  if constexpr (DT == SPX_F32) return static_cast<float>(exp(static_cast<double>(dt) * static_cast<double>(As)));
  else return exp2_fast(dt * As);
}
// per (row, channel), a sixteenth of the per-state work: fp32 rows evaluate them in double and round once, so the fp32
// criterion sees the recurrence's rounding and not the library's
template <int DT> __device__ __forceinline__ float sigmoid(float x) {
  if constexpr (DT == SPX_F32) return static_cast<float>(1.0 / (1.0 + exp(-static_cast<double>(x))));
  else return 1.f / (1.f + expf(-x));
}
template <int DT> __device__ __forceinline__ float dt_of(float raw, int softplus) {
  if (!(softplus && raw <= 20.f)) return raw;
  if constexpr (DT == SPX_F32) return static_cast<float>(log1p(exp(static_cast<double>(raw))));
  else return log1pf(expf(raw));
}

// sum += v.  COMP (fp32 rows): Kahan's compensated form, `low` carrying what the additions so far rounded away
template <bool COMP> __device__ __forceinline__ void acc_add(float &sum, float &low, float v) {
  if constexpr (COMP) {
    const float y = v - low, t = sum + y;
    low = (t - sum) - y;
    sum = t;
  } else {
    sum += v;
  }
}

// sum over the 16 lanes of a DPP row (the states of one channel)
__device__ __forceinline__ float row_sum(float x) {
  x += __shfl_xor(x, 8);
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 2);
  x += __shfl_xor(x, 1);
  return x;
}

// ---------------------------------------------------------------------------------------------- chunk table

__global__ void __launch_bounds__(256)
scan_table_kernel(const int32_t *__restrict__ offsets, int S, int n, int step, int cap, int32_t *hdr, int32_t *seq_chunk0,
                  int4 *table) {
  __shared__ int s_tot[256];
  __shared__ int s_total;
  const int tid = threadIdx.x, per = (S + 255) / 256;
  const int s0 = min(S, tid * per), s1 = min(S, s0 + per);
  int cnt = 0;
  for (int s = s0; s < s1; ++s) {
    int beg, end;
    seq_range(offsets, s, n, beg, end);
    cnt += (end - beg + kChunk - 1) / kChunk;
  }
  s_tot[tid] = cnt;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) {
      const int t = s_tot[i];
      s_tot[i] = min(run, cap);
      run = min(run + t, cap);                    // (offsets that overlap could exceed the capacity: clamped)
    }
    s_total = run;
    hdr[0] = run;
    seq_chunk0[S] = run;
  }
  __syncthreads();
  int base = s_tot[tid];
  for (int s = s0; s < s1; ++s) {
    int beg, end;
    seq_range(offsets, s, n, beg, end);
    seq_chunk0[s] = base;
    base = min(base + (end - beg + kChunk - 1) / kChunk, cap);
  }
  __syncthreads();                                // (the block's own global stores are visible behind the barrier)
  const int total = s_total;
  for (int c = tid; c < cap; c += 256) {
    int4 e = make_int4(0, 0, -1, 0);
    if (c < total) {
      int lo = 0, hi = S - 1;                     // the sequence whose chunks hold c: first s with seq_chunk0[s + 1] > c
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seq_chunk0[mid + 1] <= c) lo = mid + 1;
        else hi = mid;
      }
      int beg, end;
      seq_range(offsets, lo, n, beg, end);
      const int j = c - seq_chunk0[lo], done = j * kChunk;
      const int len = clampi(end - beg - done, 0, kChunk);
      e = make_int4(step > 0 ? beg + done : end - 1 - done, len, lo, j);
    }
    table[c] = e;
  }
}

// ---------------------------------------------------------------------------------------------- dead rows

constexpr int kDeadOuts = 5;
struct DeadArgs {
  void *out[kDeadOuts];
  int pieces[kDeadOuts];                          // 16-byte pieces of a row of each output, 0: none
  int max_pieces;
  Seq seq;
};

__global__ void __launch_bounds__(256)
dead_rows_kernel(DeadArgs a) {
  const int n = a.seq.n;
  const int lo = clampi(a.seq.offsets[0], 0, n), hi = clampi(a.seq.offsets[a.seq.S], lo, n);
  const long long total = static_cast<long long>(lo + (n - hi)) * a.max_pieces;
  for (long long item = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * 256) {
    const int q = static_cast<int>(item / a.max_pieces), pc = static_cast<int>(item - static_cast<long long>(q) * a.max_pieces);
    const int r = row_at(a.seq, q < lo ? q : hi + (q - lo));
    if (r < 0) continue;
#pragma unroll
    for (int o = 0; o < kDeadOuts; ++o)
      if (pc < a.pieces[o])
        static_cast<uint4 *>(a.out[o])[static_cast<long long>(r) * a.pieces[o] + pc] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// ---------------------------------------------------------------------------------------------- forward walks

// One wave per (chunk, 64 channels), a channel per lane, 16 states in registers.
//   kEnd  from a zero state: sum dt and the end states
//   kOut  from the entry state: y
//   kAdj  walked back from a zero adjoint: G = a_first g_first, the adjoint of the chunk's entry state
template <int DT, int ROLE>
__global__ void __launch_bounds__(kWave)
scan_walk_kernel(ScanArgs a) {
  using E = Elem<DT>;
  using T = typename E::S;
  constexpr int V = 16 / static_cast<int>(sizeof(T)), NP = kStates / V;      // 16-byte pieces of a row of B or C
  using Pc = Piece<T, V>;
  const int nb = a.Dm / kChBlock;
  const int c = blockIdx.x / nb, cb = blockIdx.x - c * nb;
  if (c >= a.hdr[0]) return;
  const int4 e = a.table[c];
  const int len = clampi(e.y, 0, kChunk), lane = threadIdx.x;
  const int d = cb * kChBlock + lane, g = (cb * kChBlock) / (a.Dm / a.G);       // (g is uniform over the wave)
  const int myrow = lane < len ? row_at(a.seq, e.x + a.seq.step * lane) : -1;
  const T *__restrict__ u = static_cast<const T *>(a.u), *__restrict__ delta = static_cast<const T *>(a.delta);
  const T *__restrict__ z = static_cast<const T *>(a.z), *__restrict__ dout = static_cast<const T *>(a.dout);
  const Pc *__restrict__ Bp = static_cast<const Pc *>(a.B), *__restrict__ Cp = static_cast<const Pc *>(a.C);
  float A2[kStates], h[kStates];
  const long long slot = (static_cast<long long>(c) * kStates) * a.Dm + d;
#pragma unroll
  for (int k = 0; k < kStates; ++k) {
    A2[k] = a_scaled<DT>(a.A[d * kStates + k]);
    h[k] = ROLE == kOut ? a.H[slot + static_cast<long long>(k) * a.Dm] : 0.f;
  }
  const float Dd = a.D ? a.D[d] : 0.f, bias = a.bias ? a.bias[d] : 0.f;
  float sdt = 0.f;
  for (int t0 = 0; t0 < len; t0 += kRowsAhead) {
    int r[kRowsAhead];
    float dt[kRowsAhead], x[kRowsAhead], zz[kRowsAhead];
    Pc pb[kRowsAhead][NP], pc[kRowsAhead][NP];    // B (kAdj: unused) and C of the row, the same for every lane
#pragma unroll
    for (int i = 0; i < kRowsAhead; ++i) {        // (the loads of kRowsAhead rows issued together)
      const int t = ROLE == kAdj ? len - 1 - (t0 + i) : t0 + i;
      r[i] = (t0 + i < len) ? __builtin_amdgcn_readfirstlane(__shfl(myrow, t)) : -1;
      dt[i] = 0.f, x[i] = 0.f, zz[i] = 0.f;
      if (r[i] < 0) continue;
      const long long at = static_cast<long long>(r[i]) * a.Dm + d;
      const long long bat = (static_cast<long long>(r[i]) * a.G + g) * NP;
      dt[i] = E::up(delta[at]);
      x[i] = E::up((ROLE == kAdj ? dout : u)[at]);
      if (ROLE != kEnd && z) zz[i] = E::up(z[at]);
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        if (ROLE != kAdj) pb[i][j] = Bp[bat + j];
        if (ROLE != kEnd) pc[i][j] = Cp[bat + j];
      }
    }
#pragma unroll
    for (int i = 0; i < kRowsAhead; ++i) {
      if (r[i] < 0) continue;                     // (uniform: a position that is skipped leaves the state alone)
      const float dti = dt_of<DT>(dt[i] + bias, a.softplus);
      if (ROLE == kAdj) {
        const float dyp = z ? x[i] * zz[i] * sigmoid<DT>(zz[i]) : x[i];
#pragma unroll
        for (int k = 0; k < kStates; ++k)
          h[k] = decay<DT>(dti, A2[k]) * fmaf(E::up(pc[i][k / V].e[k % V]), dyp, h[k]);
      } else {
        const float dtu = dti * x[i];
        sdt += dti;
#pragma unroll
        for (int k = 0; k < kStates; ++k)
          h[k] = fmaf(decay<DT>(dti, A2[k]), h[k], dtu * E::up(pb[i][k / V].e[k % V]));
        if (ROLE == kOut) {
          float y = 0.f;
#pragma unroll
          for (int k = 0; k < kStates; ++k) y = fmaf(E::up(pc[i][k / V].e[k % V]), h[k], y);
          y = fmaf(Dd, x[i], y);
          if (z) y *= zz[i] * sigmoid<DT>(zz[i]);
          static_cast<T *>(a.y)[static_cast<long long>(r[i]) * a.Dm + d] = E::down(y);
        }
      }
    }
  }
  if (ROLE == kOut) return;
  float *dst = ROLE == kEnd ? a.H : a.Gs;
#pragma unroll
  for (int k = 0; k < kStates; ++k) dst[slot + static_cast<long long>(k) * a.Dm] = h[k];
  if (ROLE == kEnd) a.sumdt[static_cast<long long>(c) * a.Dm + d] = sdt;
}

// A thread per (sequence, state, channel) walks the chunks of its sequence: X[c] becomes what entered chunk c, the
// running value leaves it as exp(A sum dt_c) * running + X[c].  back: from the last chunk to the first (the adjoint).
__global__ void __launch_bounds__(256)
scan_carry_kernel(const int32_t *__restrict__ seq_chunk0, const float *__restrict__ A, const float *__restrict__ sumdt,
                  float *X, int Dm, int cap, int back) {
  const int per = (kStates * Dm + 255) / 256;     // workgroups of a sequence
  const int s = blockIdx.x / per, col = (blockIdx.x - s * per) * 256 + threadIdx.x;
  if (col >= kStates * Dm) return;
  const int k = col / Dm, d = col - k * Dm;
  const int c0 = clampi(seq_chunk0[s], 0, cap), c1 = clampi(seq_chunk0[s + 1], c0, cap);
  const float Ak = A[d * kStates + k];
  const long long stride = static_cast<long long>(kStates) * Dm;
  float run = 0.f;
  constexpr int kBatch = 8;
  for (int j0 = 0; j0 < c1 - c0; j0 += kBatch) {
    float e[kBatch], sd[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {            // (the loads do not depend on the chain: issued together)
      const int j = j0 + i, c = back ? c1 - 1 - j : c0 + j;
      e[i] = 0.f, sd[i] = 0.f;
      if (j < c1 - c0) e[i] = X[c * stride + col], sd[i] = sumdt[static_cast<long long>(c) * Dm + d];
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int j = j0 + i, c = back ? c1 - 1 - j : c0 + j;
      if (j >= c1 - c0) break;
      X[c * stride + col] = run;
      run = fmaf(expf(Ak * sd[i]), run, e[i]);
    }
  }
}

// ---------------------------------------------------------------------------------------------- backward walk

template <int DT>
__global__ void __launch_bounds__(kBwdThreads)
scan_bwd_kernel(ScanArgs a) {
  using E = Elem<DT>;
  using T = typename E::S;
  constexpr int V = 16 / static_cast<int>(sizeof(T)), PPR = kBwdCh / V;   // pieces of a row of one channel step
  using Pc = Piece<T, V>;
  __shared__ float s_dt[kChunk][kBwdCh], s_u[kChunk][kBwdCh], s_dyp[kChunk][kBwdCh];
  __shared__ float s_y[kChunk][kBwdCh], s_du[kChunk][kBwdCh], s_dd[kChunk][kBwdCh];
  __shared__ float s_B[kChunk][kStates], s_C[kChunk][kStates];
  __shared__ float s_dB[kBwdWaves][kChunk][kStates], s_dC[kBwdWaves][kChunk][kStates];
  constexpr bool kComp = DT == SPX_F32;           // fp32 rows: sums over channels and positions cost one rounding
  __shared__ float s_lB[kComp ? kBwdWaves : 1][kChunk][kStates], s_lC[kComp ? kBwdWaves : 1][kChunk][kStates];
  __shared__ int s_row[kChunk];
  const int c = blockIdx.x / a.G, g = blockIdx.x - c * a.G;
  if (c >= a.hdr[0]) return;
  const int4 e = a.table[c];
  const int len = clampi(e.y, 0, kChunk), tid = threadIdx.x;
  const int ch = tid / kStates, k = tid % kStates, wave = tid / kWave, lane = tid % kWave;
  const int cpg = a.Dm / a.G;
  const T *__restrict__ u = static_cast<const T *>(a.u), *__restrict__ delta = static_cast<const T *>(a.delta);
  const T *__restrict__ z = static_cast<const T *>(a.z), *__restrict__ dout = static_cast<const T *>(a.dout);
  if (tid < kChunk) s_row[tid] = tid < len ? row_at(a.seq, e.x + a.seq.step * tid) : -1;
  for (int i = tid; i < kBwdWaves * kChunk * kStates; i += kBwdThreads) {
    (&s_dB[0][0][0])[i] = 0.f, (&s_dC[0][0][0])[i] = 0.f;
    if constexpr (kComp) (&s_lB[0][0][0])[i] = 0.f, (&s_lC[0][0][0])[i] = 0.f;
  }
  __syncthreads();
  for (int i = tid; i < len * kStates; i += kBwdThreads) {
    const int t = i / kStates, kk = i % kStates, r = s_row[t];
    const long long at = (static_cast<long long>(r) * a.G + g) * kStates + kk;
    s_B[t][kk] = r >= 0 ? E::up(static_cast<const T *>(a.B)[at]) : 0.f;
    s_C[t][kk] = r >= 0 ? E::up(static_cast<const T *>(a.C)[at]) : 0.f;
  }
  for (int d0 = g * cpg; d0 < (g + 1) * cpg; d0 += kBwdCh) {
    const int d = d0 + ch;
    __syncthreads();                              // (the rows of the step before are written out)
    for (int i = tid; i < len * PPR; i += kBwdThreads) {
      const int t = i / PPR, pc = i - t * PPR, r = s_row[t], col = d0 + pc * V;
      Pc pd = {}, pu = {}, po = {}, pz = {};
      if (r >= 0) {
        const long long at = static_cast<long long>(r) * a.Dm + col;
        pd = *reinterpret_cast<const Pc *>(delta + at);
        pu = *reinterpret_cast<const Pc *>(u + at);
        po = *reinterpret_cast<const Pc *>(dout + at);
        if (z) pz = *reinterpret_cast<const Pc *>(z + at);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {               // (a position that is skipped: dt = 0 leaves the state alone)
        const float zz = E::up(pz.e[j]), dy = E::up(po.e[j]);
        s_dt[t][pc * V + j] = r >= 0 ? dt_of<DT>(E::up(pd.e[j]) + (a.bias ? a.bias[col + j] : 0.f), a.softplus) : 0.f;
        s_u[t][pc * V + j] = E::up(pu.e[j]);
        s_dyp[t][pc * V + j] = z ? dy * zz * sigmoid<DT>(zz) : dy;
      }
    }
    __syncthreads();
    // the chunk forward from its entry state, every h_t kept
    const float Ak = a.A[d * kStates + k], A2 = a_scaled<DT>(Ak), Dd = a.D ? a.D[d] : 0.f;
    const long long slot = (static_cast<long long>(c) * kStates + k) * a.Dm + d;
    const float hin = a.H[slot];
    float hist[kChunk], h = hin;
#pragma unroll
    for (int t = 0; t < kChunk; ++t) {
      hist[t] = 0.f;
      if (t < len) {
        const float dt = s_dt[t][ch], uu = s_u[t][ch];
        h = fmaf(decay<DT>(dt, A2), h, dt * uu * s_B[t][k]);
        hist[t] = h;
        if (z) {
          const float y = row_sum(s_C[t][k] * h);
          if (k == 0) s_y[t][ch] = fmaf(Dd, uu, y);
        }
      }
    }
    // and back: gk is the adjoint of h_t
    float gk = a.Gs[slot], dA = 0.f, dD = 0.f, db = 0.f, lA = 0.f, lD = 0.f, lb = 0.f;
#pragma unroll
    for (int t = kChunk - 1; t >= 0; --t) {
      if (t < len) {
        const float dt = s_dt[t][ch], uu = s_u[t][ch], dyp = s_dyp[t][ch], Bk = s_B[t][k], Ck = s_C[t][k];
        gk = fmaf(Ck, dyp, gk);
        const float ak = decay<DT>(dt, A2), hprev = t > 0 ? hist[t - 1] : hin;
        const float gah = gk * ak * hprev;
        const float S1 = row_sum(gk * Bk), S2 = row_sum(gah * Ak);
        acc_add<kComp>(dA, lA, gah * dt);
        float vb = gk * dt * uu, vc = dyp * hist[t];
        vb += __shfl_xor(vb, 16), vc += __shfl_xor(vc, 16);          // (over the four channels of the wave)
        vb += __shfl_xor(vb, 32), vc += __shfl_xor(vc, 32);
        if (lane < kStates) {
          acc_add<kComp>(s_dB[wave][t][k], s_lB[kComp ? wave : 0][t][k], vb);
          acc_add<kComp>(s_dC[wave][t][k], s_lC[kComp ? wave : 0][t][k], vc);
        }
        if (k == 0) {
          const float sp = a.softplus ? -expm1f(-dt) : 1.f;                  // (1 - exp(-dt) = sigmoid(raw))
          const float dd = s_row[t] >= 0 ? fmaf(uu, S1, S2) * sp : 0.f;
          s_du[t][ch] = fmaf(dt, S1, Dd * dyp);
          s_dd[t][ch] = dd;
          acc_add<kComp>(dD, lD, dyp * uu);
          acc_add<kComp>(db, lb, dd);
        }
        gk *= ak;
      }
    }
    a.Gs[slot] = dA;                              // (the slot this lane read its adjoint from)
    if (k == 0) {
      a.pD[(static_cast<long long>(c) * 2) * a.Dm + d] = dD;
      a.pD[(static_cast<long long>(c) * 2 + 1) * a.Dm + d] = db;
    }
    __syncthreads();
    for (int i = tid; i < len * PPR; i += kBwdThreads) {
      const int t = i / PPR, pc = i - t * PPR, r = s_row[t];
      if (r < 0) continue;
      const long long at = static_cast<long long>(r) * a.Dm + d0 + pc * V;
      Pc ou, od;
#pragma unroll
      for (int j = 0; j < V; ++j) ou.e[j] = E::down(s_du[t][pc * V + j]), od.e[j] = E::down(s_dd[t][pc * V + j]);
      *reinterpret_cast<Pc *>(static_cast<T *>(a.du) + at) = ou;
      *reinterpret_cast<Pc *>(static_cast<T *>(a.ddelta) + at) = od;
      if (z) {
        const Pc pz = *reinterpret_cast<const Pc *>(z + at), po = *reinterpret_cast<const Pc *>(dout + at);
        Pc oz;
#pragma unroll
        for (int j = 0; j < V; ++j) {             // d(z sigmoid(z)) = sigmoid(z) (1 + z (1 - sigmoid(z)))
          const float zz = E::up(pz.e[j]), sg = sigmoid<DT>(zz);
          oz.e[j] = E::down(E::up(po.e[j]) * s_y[t][pc * V + j] * sg * fmaf(zz, 1.f - sg, 1.f));
        }
        *reinterpret_cast<Pc *>(static_cast<T *>(a.dz) + at) = oz;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < len * kStates; i += kBwdThreads) {
    const int t = i / kStates, kk = i % kStates, r = s_row[t];
    if (r < 0) continue;
    const long long at = (static_cast<long long>(r) * a.G + g) * kStates + kk;
    float sb = 0.f, sc = 0.f;
#pragma unroll
    for (int w = 0; w < kBwdWaves; ++w) sb += s_dB[w][t][kk], sc += s_dC[w][t][kk];
    static_cast<T *>(a.dB)[at] = E::down(sb);
    static_cast<T *>(a.dC)[at] = E::down(sc);
  }
}

// out[(col % Dm) * R + col / Dm] = sum over the rows c < count of part[c * stride + col], for the columns [0, cols):
// 16 lanes take the rows 16 apart each, their sums are added in lane order.  count = min(*count_dev, count_host).
__global__ void __launch_bounds__(kRedCols * kRedLanes)
reduce_cols_kernel(const float *__restrict__ part, long long stride, int cols, const int32_t *__restrict__ count_dev,
                   int count_host, int Dm, int R, float *out) {
  __shared__ float s[kRedLanes][kRedCols];
  const int cl = threadIdx.x % kRedCols, ln = threadIdx.x / kRedCols, col = blockIdx.x * kRedCols + cl;
  const int count = count_dev ? clampi(*count_dev, 0, count_host) : count_host;
  float acc = 0.f;
  if (col < cols) {
#pragma unroll 4
    for (int c = ln; c < count; c += kRedLanes) acc += part[c * stride + col];
  }
  s[ln][cl] = acc;
  __syncthreads();
  if (ln != 0 || col >= cols) return;
  float sum = 0.f;
#pragma unroll
  for (int l = 0; l < kRedLanes; ++l) sum += s[l][cl];
  out[(col % Dm) * R + col / Dm] = sum;
}

// ---------------------------------------------------------------------------------------------- convolution

struct ConvArgs {
  const void *x, *w, *b, *dout;
  int w_f32, b_f32;
  Seq seq;
  int Dm, W, act;
  void *out;                                      // forward: out; backward: dx
  float *dpre, *part;                             // [n, Dm] by position; [blocks, W + 1, Dm]
};

template <int DT> __device__ __forceinline__ float param_at(const void *p, int f32, long long i) {
  return f32 ? static_cast<const float *>(p)[i] : Elem<DT>::up(static_cast<const typename Elem<DT>::S *>(p)[i]);
}

template <int DT>
__global__ void __launch_bounds__(256)
conv_fwd_kernel(ConvArgs a) {
  using E = Elem<DT>;
  using T = typename E::S;
  constexpr int V = 16 / static_cast<int>(sizeof(T));
  using Pc = Piece<T, V>;
  const int pieces = a.Dm / V;
  const long long total = static_cast<long long>(a.seq.n) * pieces;
  const T *__restrict__ x = static_cast<const T *>(a.x);
  for (long long item = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * 256) {
    const int p = static_cast<int>(row_of(item, total, pieces)), d0 = static_cast<int>(item - static_cast<long long>(p) * pieces) * V;
    const int r = row_at(a.seq, p);
    if (r < 0) continue;
    int beg, end;
    const int s = seq_of(a.seq, p, beg, end);
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = (s >= 0 && a.b) ? param_at<DT>(a.b, a.b_f32, d0 + j) : 0.f;
    if (s >= 0) {
      for (int t = 0; t < a.W; ++t) {             // (ascending tap)
        const int q = p - a.seq.step * (a.W - 1 - t);
        const int rq = (q >= beg && q < end) ? row_at(a.seq, q) : -1;
        if (rq < 0) continue;
        const Pc px = *reinterpret_cast<const Pc *>(x + static_cast<long long>(rq) * a.Dm + d0);
#pragma unroll
        for (int j = 0; j < V; ++j)
          acc[j] = fmaf(param_at<DT>(a.w, a.w_f32, static_cast<long long>(d0 + j) * a.W + t), E::up(px.e[j]), acc[j]);
      }
    }
    Pc o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.e[j] = E::down((a.act && s >= 0) ? acc[j] * sigmoid<DT>(acc[j]) : acc[j]);
    *reinterpret_cast<Pc *>(static_cast<T *>(a.out) + static_cast<long long>(r) * a.Dm + d0) = o;
  }
}

// d_pre of kConvRows positions x 64 channels (a channel per lane, four position lanes), and the workgroup's partial of
// dweight [W, 64] and dbias [64]
template <int DT>
__global__ void __launch_bounds__(kConvLanes * kChBlock)
conv_bwd_pre_kernel(ConvArgs a) {
  using E = Elem<DT>;
  using T = typename E::S;
  __shared__ float s_acc[kConvLanes][kMaxW + 1][kChBlock];
  const int nb = a.Dm / kChBlock;
  const int blk = blockIdx.x / nb, cb = blockIdx.x - blk * nb;
  const int ch = threadIdx.x % kChBlock, pl = threadIdx.x / kChBlock, d = cb * kChBlock + ch;
  const T *__restrict__ x = static_cast<const T *>(a.x), *__restrict__ dout = static_cast<const T *>(a.dout);
  float w[kMaxW], acc[kMaxW + 1];
#pragma unroll
  for (int t = 0; t < kMaxW; ++t) w[t] = t < a.W ? param_at<DT>(a.w, a.w_f32, static_cast<long long>(d) * a.W + t) : 0.f;
#pragma unroll
  for (int t = 0; t <= kMaxW; ++t) acc[t] = 0.f;
  const float bias = a.b ? param_at<DT>(a.b, a.b_f32, d) : 0.f;
  const int p0 = blk * kConvRows, p1 = min(a.seq.n, p0 + kConvRows);
  for (int p = p0 + pl; p < p1; p += kConvLanes) {
    int beg, end;
    const int s = seq_of(a.seq, p, beg, end), r = row_at(a.seq, p);
    float dp = 0.f;
    if (s >= 0 && r >= 0) {
      float xv[kMaxW], pre = bias;
#pragma unroll
      for (int t = 0; t < kMaxW; ++t) {
        xv[t] = 0.f;
        if (t >= a.W) continue;
        const int q = p - a.seq.step * (a.W - 1 - t);
        const int rq = (q >= beg && q < end) ? row_at(a.seq, q) : -1;
        if (rq >= 0) xv[t] = E::up(x[static_cast<long long>(rq) * a.Dm + d]);
        pre = fmaf(w[t], xv[t], pre);
      }
      dp = E::up(dout[static_cast<long long>(r) * a.Dm + d]);
      if (a.act) {
        const float sg = sigmoid<DT>(pre);
        dp *= sg * fmaf(pre, 1.f - sg, 1.f);
      }
#pragma unroll
      for (int t = 0; t < kMaxW; ++t) acc[t] = fmaf(dp, xv[t], acc[t]);
      acc[kMaxW] += dp;
    }
    a.dpre[static_cast<long long>(p) * a.Dm + d] = dp;
  }
#pragma unroll
  for (int t = 0; t <= kMaxW; ++t) s_acc[pl][t][ch] = acc[t];
  __syncthreads();
  if (pl != 0) return;
  for (int t = 0; t <= a.W; ++t) {                // (rows 0 .. W - 1: dweight, row W: dbias)
    const int src = t < a.W ? t : kMaxW;
    float sum = 0.f;
#pragma unroll
    for (int l = 0; l < kConvLanes; ++l) sum += s_acc[l][src][ch];
    a.part[(static_cast<long long>(blk) * (a.W + 1) + t) * a.Dm + d] = sum;
  }
}

template <int DT>
__global__ void __launch_bounds__(256)
conv_bwd_x_kernel(ConvArgs a) {
  using E = Elem<DT>;
  using T = typename E::S;
  constexpr int V = 16 / static_cast<int>(sizeof(T));
  using Pc = Piece<T, V>;
  const int pieces = a.Dm / V;
  const long long total = static_cast<long long>(a.seq.n) * pieces;
  for (long long item = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * 256) {
    const int p = static_cast<int>(row_of(item, total, pieces)), d0 = static_cast<int>(item - static_cast<long long>(p) * pieces) * V;
    const int r = row_at(a.seq, p);
    if (r < 0) continue;
    int beg, end;
    const int s = seq_of(a.seq, p, beg, end);
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    if (s >= 0) {
      for (int t = a.W - 1; t >= 0; --t) {        // x of p is tap t of the position W - 1 - t further along the walk
        const int q = p + a.seq.step * (a.W - 1 - t);
        if (q < beg || q >= end) continue;
        const float *dp = a.dpre + static_cast<long long>(q) * a.Dm + d0;
#pragma unroll
        for (int j = 0; j < V; ++j)
          acc[j] = fmaf(param_at<DT>(a.w, a.w_f32, static_cast<long long>(d0 + j) * a.W + t), dp[j], acc[j]);
      }
    }
    Pc o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.e[j] = E::down(acc[j]);
    *reinterpret_cast<Pc *>(static_cast<T *>(a.out) + static_cast<long long>(r) * a.Dm + d0) = o;
  }
}

// ------------------------------------------------------------------------------------------------ host side

int check_rows_shape(int n, int S, int Dm, int dtype) {
  SPX_CHECK(dtype == SPX_F32 || dtype == SPX_F16 || dtype == SPX_BF16, "dtype must be f32, f16 or bf16, got %d", dtype);
  SPX_CHECK(Dm >= kChBlock && Dm % kChBlock == 0 && Dm <= kMaxDm, "Dm must be a multiple of %d, at most %d, got %d",
            kChBlock, kMaxDm, Dm);
  SPX_CHECK(n >= 0 && S >= 1, "bad row / sequence counts %d / %d", n, S);
  SPX_CHECK(static_cast<long long>(n) * Dm < 0x80000000LL, "n * Dm must stay below 2^31, got %d x %d", n, Dm);
  return 0;
}

int check_scan_shape(int n, int S, int Dm, int G, int dtype, int step) {
  if (int rc = check_rows_shape(n, S, Dm, dtype)) return rc;
  SPX_CHECK(G >= 1 && Dm % G == 0 && (Dm / G) % kChBlock == 0, "G must divide Dm into multiples of %d channels, got G = %d, "
            "Dm = %d", kChBlock, G, Dm);
  SPX_CHECK(step == 1 || step == -1, "step is +1 or -1, got %d", step);
  SPX_CHECK(static_cast<long long>(scan_cap(n, S)) * kStates * Dm < 0x7fffffff00LL, "workspace too large");
  return 0;
}

int launch_dead_rows(const Seq &q, std::initializer_list<void *> outs, std::initializer_list<int> row_bytes, hipStream_t s) {
  DeadArgs a = {};
  a.seq = q;
  int i = 0;
  for (void *o : outs) a.out[i++] = o;
  i = 0;
  for (int b : row_bytes) {
    a.pieces[i] = a.out[i] ? b / 16 : 0;
    a.max_pieces = a.pieces[i] > a.max_pieces ? a.pieces[i] : a.max_pieces;
    ++i;
  }
  const dim3 grid(stream_blocks(static_cast<long long>(q.n) * a.max_pieces, 256));
  hipLaunchKernelGGL(dead_rows_kernel, grid, dim3(256), 0, s, a);
  SPX_LAUNCH_CHECK();
  return 0;
}

int launch_reduce(const float *part, long long stride, int cols, const int32_t *count_dev, int count_host, int Dm, int R,
                  float *out, hipStream_t s) {
  hipLaunchKernelGGL(reduce_cols_kernel, dim3((cols + kRedCols - 1) / kRedCols), dim3(kRedCols * kRedLanes), 0, s, part,
                     stride, cols, count_dev, count_host, Dm, R, out);
  SPX_LAUNCH_CHECK();
  return 0;
}

ScanArgs scan_args(const void *u, const void *delta, const float *A, const void *B, const void *C, const float *D,
                   const void *z, const float *bias, const Seq &q, int Dm, int G, int softplus, const Ws &w) {
  ScanArgs a = {};
  a.u = u, a.delta = delta, a.z = z, a.B = B, a.C = C, a.A = A, a.D = D, a.bias = bias, a.seq = q, a.Dm = Dm, a.G = G;
  a.softplus = softplus, a.hdr = w.hdr, a.table = w.table, a.sumdt = w.sumdt, a.H = w.H, a.Gs = w.Gs, a.pD = w.pD;
  return a;
}

}  // namespace
}  // namespace spx

extern "C" {

size_t spx_selective_scan_ws_bytes(int n, int S, int Dm, int G) {
  using namespace spx;
  if (n < 0 || S < 1 || Dm < kChBlock || Dm % kChBlock != 0 || Dm > kMaxDm || G < 1 || Dm % G != 0 ||
      (Dm / G) % kChBlock != 0 || static_cast<long long>(n) * Dm >= 0x80000000LL)
    return 0;
  return carve_scan(nullptr, n, S, Dm).bytes;
}

int spx_selective_scan_fwd(const void *u, const void *delta, const float *A, const void *B, const void *C, const float *D,
                           const void *z, const float *delta_bias, const int32_t *order, const int32_t *offsets, int n,
                           int S, int Dm, int G, int dtype, int softplus, int step, void *y, void *ws, size_t ws_bytes,
                           spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_scan_shape(n, S, Dm, G, dtype, step)) return rc;
  const Ws w = carve_scan(ws, n, S, Dm);
  SPX_CHECK(ws_bytes >= w.bytes, "workspace holds %zu bytes, %zu are needed", ws_bytes, w.bytes);
  if (n == 0) return 0;
  SPX_CHECK(u && delta && A && B && C && offsets && y && ws, "u / delta / A / B / C / offsets / y / ws is NULL");
  SPX_CHECK(aligned_to(u, 16) && aligned_to(delta, 16) && aligned_to(z, 16) && aligned_to(y, 16) && aligned_to(B, 16) &&
            aligned_to(C, 16) && aligned_to(ws, 256) && aligned_to(A, 4) && aligned_to(D, 4) && aligned_to(delta_bias, 4) &&
            aligned_to(order, 4) && aligned_to(offsets, 4), "rows must be aligned to 16 bytes, ws to 256, tables to 4");
  const Seq q = {order, offsets, n, S, step};
  const int cap = scan_cap(n, S), eb = elem_bytes(dtype);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ScanArgs a = scan_args(u, delta, A, B, C, D, z, delta_bias, q, Dm, G, softplus, w);
  a.y = y;
  hipLaunchKernelGGL(scan_table_kernel, dim3(1), dim3(256), 0, s, offsets, S, n, step, cap, w.hdr, w.seq_chunk0, w.table);
  SPX_LAUNCH_CHECK();
  if (int rc = launch_dead_rows(q, {y}, {Dm * eb}, s)) return rc;
  const dim3 grid(static_cast<unsigned>(cap) * (Dm / kChBlock));
  const dim3 carry(static_cast<unsigned>((kStates * Dm + 255) / 256) * S);
  dispatch_value<SPX_F32, SPX_F16, SPX_BF16>(dtype, [&](auto dt) {
    hipLaunchKernelGGL((scan_walk_kernel<dt, kEnd>), grid, dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(scan_carry_kernel, carry, dim3(256), 0, s, w.seq_chunk0, A, w.sumdt, w.H, Dm, cap, 0);
    hipLaunchKernelGGL((scan_walk_kernel<dt, kOut>), grid, dim3(kWave), 0, s, a);
  });
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_selective_scan_bwd(const void *u, const void *delta, const float *A, const void *B, const void *C, const float *D,
                           const void *z, const float *delta_bias, const void *d_out, const int32_t *order,
                           const int32_t *offsets, int n, int S, int Dm, int G, int dtype, int softplus, int step, void *du,
                           void *ddelta, float *dA, void *dB, void *dC, float *dD, void *dz, float *ddelta_bias, void *ws,
                           size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_scan_shape(n, S, Dm, G, dtype, step)) return rc;
  const Ws w = carve_scan(ws, n, S, Dm);
  SPX_CHECK(ws_bytes >= w.bytes, "workspace holds %zu bytes, %zu are needed", ws_bytes, w.bytes);
  if (n == 0) return 0;
  SPX_CHECK(u && delta && A && B && C && d_out && offsets && du && ddelta && dA && dB && dC && ws,
            "u / delta / A / B / C / d_out / offsets / du / ddelta / dA / dB / dC / ws is NULL");
  SPX_CHECK((z != nullptr) == (dz != nullptr) && (!dD || D) && (!ddelta_bias || delta_bias),
            "dz comes with z, dD with D, ddelta_bias with delta_bias");
  SPX_CHECK(aligned_to(u, 16) && aligned_to(delta, 16) && aligned_to(z, 16) && aligned_to(d_out, 16) && aligned_to(B, 16) &&
            aligned_to(C, 16) && aligned_to(du, 16) && aligned_to(ddelta, 16) && aligned_to(dz, 16) && aligned_to(dB, 16) &&
            aligned_to(dC, 16) && aligned_to(ws, 256) && aligned_to(A, 4) && aligned_to(D, 4) && aligned_to(delta_bias, 4) &&
            aligned_to(dA, 4) && aligned_to(dD, 4) && aligned_to(ddelta_bias, 4) && aligned_to(order, 4) &&
            aligned_to(offsets, 4), "rows must be aligned to 16 bytes, ws to 256, tables to 4");
  const Seq q = {order, offsets, n, S, step};
  const int cap = scan_cap(n, S), eb = elem_bytes(dtype);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ScanArgs a = scan_args(u, delta, A, B, C, D, z, delta_bias, q, Dm, G, softplus, w);
  a.dout = d_out, a.du = du, a.ddelta = ddelta, a.dz = dz, a.dB = dB, a.dC = dC;
  if (int rc = launch_dead_rows(q, {du, ddelta, dz, dB, dC}, {Dm * eb, Dm * eb, Dm * eb, G * kStates * eb, G * kStates * eb}, s))
    return rc;
  const dim3 grid(static_cast<unsigned>(cap) * (Dm / kChBlock));
  const dim3 carry(static_cast<unsigned>((kStates * Dm + 255) / 256) * S);
  dispatch_value<SPX_F32, SPX_F16, SPX_BF16>(dtype, [&](auto dt) {
    hipLaunchKernelGGL((scan_walk_kernel<dt, kAdj>), grid, dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(scan_carry_kernel, carry, dim3(256), 0, s, w.seq_chunk0, A, w.sumdt, w.Gs, Dm, cap, 1);
    hipLaunchKernelGGL((scan_bwd_kernel<dt>), dim3(static_cast<unsigned>(cap) * G), dim3(kBwdThreads), 0, s, a);
  });
  SPX_LAUNCH_CHECK();
  const long long stride = static_cast<long long>(kStates) * Dm;
  if (int rc = launch_reduce(w.Gs, stride, kStates * Dm, w.hdr, cap, Dm, kStates, dA, s)) return rc;
  if (dD)
    if (int rc = launch_reduce(w.pD, 2LL * Dm, Dm, w.hdr, cap, Dm, 1, dD, s)) return rc;
  if (ddelta_bias)
    if (int rc = launch_reduce(w.pD + Dm, 2LL * Dm, Dm, w.hdr, cap, Dm, 1, ddelta_bias, s)) return rc;
  return 0;
}

size_t spx_causal_conv_rows_ws_bytes(int n, int Dm, int W) {
  using namespace spx;
  if (n < 0 || Dm < kChBlock || Dm % kChBlock != 0 || Dm > kMaxDm || W < 2 || W > kMaxW ||
      static_cast<long long>(n) * Dm >= 0x80000000LL)
    return 0;
  const size_t blocks = (static_cast<size_t>(n) + kConvRows - 1) / kConvRows;
  return align_up(static_cast<size_t>(n) * Dm * sizeof(float), 256) + align_up(blocks * (W + 1) * Dm * sizeof(float), 256);
}

namespace {
int check_conv(int n, int S, int Dm, int W, int dtype, int w_dt, int b_dt, int act, int step) {
  using namespace spx;
  if (int rc = check_rows_shape(n, S, Dm, dtype)) return rc;
  SPX_CHECK(W >= 2 && W <= kMaxW, "the width must be in 2 .. %d, got %d", kMaxW, W);
  SPX_CHECK((w_dt == dtype || w_dt == SPX_F32) && (b_dt == dtype || b_dt == SPX_F32),
            "weight and bias are f32 or of the rows' dtype, got %d and %d", w_dt, b_dt);
  SPX_CHECK(act == 0 || act == 1, "act is 0 (none) or 1 (SiLU), got %d", act);
  SPX_CHECK(step == 1 || step == -1, "step is +1 or -1, got %d", step);
  return 0;
}
}  // namespace

int spx_causal_conv_rows_fwd(const void *x, const void *weight, int w_dt, const void *bias, int b_dt, const int32_t *order,
                             const int32_t *offsets, int n, int S, int Dm, int W, int dtype, int act, int step, void *out,
                             spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_conv(n, S, Dm, W, dtype, w_dt, b_dt, act, step)) return rc;
  if (n == 0) return 0;
  SPX_CHECK(x && weight && offsets && out, "x / weight / offsets / out is NULL");
  SPX_CHECK(aligned_to(x, 16) && aligned_to(out, 16) && aligned_to(weight, 4) && aligned_to(bias, 4) && aligned_to(order, 4) &&
            aligned_to(offsets, 4), "rows must be aligned to 16 bytes, tables to 4");
  ConvArgs a = {};
  a.x = x, a.w = weight, a.b = bias, a.w_f32 = w_dt == SPX_F32, a.b_f32 = b_dt == SPX_F32;
  a.seq = {order, offsets, n, S, step}, a.Dm = Dm, a.W = W, a.act = act, a.out = out;
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_value<SPX_F32, SPX_F16, SPX_BF16>(dtype, [&](auto dt) {
    const dim3 grid(stream_blocks(static_cast<long long>(n) * (Dm * elem_bytes(dtype) / 16), 256));
    hipLaunchKernelGGL((conv_fwd_kernel<dt>), grid, dim3(256), 0, s, a);
  });
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_causal_conv_rows_bwd(const void *x, const void *weight, int w_dt, const void *bias, int b_dt, const void *d_out,
                             const int32_t *order, const int32_t *offsets, int n, int S, int Dm, int W, int dtype, int act,
                             int step, void *dx, float *dweight, float *dbias, void *ws, size_t ws_bytes,
                             spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_conv(n, S, Dm, W, dtype, w_dt, b_dt, act, step)) return rc;
  const size_t need = spx_causal_conv_rows_ws_bytes(n, Dm, W);
  SPX_CHECK(ws_bytes >= need, "workspace holds %zu bytes, %zu are needed", ws_bytes, need);
  if (n == 0) return 0;
  SPX_CHECK(x && weight && d_out && offsets && dx && dweight && ws, "x / weight / d_out / offsets / dx / dweight / ws is NULL");
  SPX_CHECK(aligned_to(x, 16) && aligned_to(d_out, 16) && aligned_to(dx, 16) && aligned_to(ws, 256) && aligned_to(weight, 4) &&
            aligned_to(bias, 4) && aligned_to(dweight, 4) && aligned_to(dbias, 4) && aligned_to(order, 4) &&
            aligned_to(offsets, 4), "rows must be aligned to 16 bytes, ws to 256, tables to 4");
  const int blocks = (n + kConvRows - 1) / kConvRows;
  Carver carve(ws);
  ConvArgs a = {};
  a.x = x, a.w = weight, a.b = bias, a.dout = d_out, a.w_f32 = w_dt == SPX_F32, a.b_f32 = b_dt == SPX_F32;
  a.seq = {order, offsets, n, S, step}, a.Dm = Dm, a.W = W, a.act = act, a.out = dx;
  a.dpre = carve.take<float>(static_cast<size_t>(n) * Dm);
  a.part = carve.take<float>(static_cast<size_t>(blocks) * (W + 1) * Dm);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_value<SPX_F32, SPX_F16, SPX_BF16>(dtype, [&](auto dt) {
    hipLaunchKernelGGL((conv_bwd_pre_kernel<dt>), dim3(static_cast<unsigned>(blocks) * (Dm / kChBlock)),
                       dim3(kConvLanes * kChBlock), 0, s, a);
    const dim3 grid(stream_blocks(static_cast<long long>(n) * (Dm * elem_bytes(dtype) / 16), 256));
    hipLaunchKernelGGL((conv_bwd_x_kernel<dt>), grid, dim3(256), 0, s, a);
  });
  SPX_LAUNCH_CHECK();
  const long long stride = static_cast<long long>(W + 1) * Dm;
  if (int rc = launch_reduce(a.part, stride, W * Dm, nullptr, blocks, Dm, W, dweight, s)) return rc;
  if (dbias)
    if (int rc = launch_reduce(a.part + static_cast<long long>(W) * Dm, stride, Dm, nullptr, blocks, Dm, 1, dbias, s)) return rc;
  return 0;
}

}  // extern "C"
