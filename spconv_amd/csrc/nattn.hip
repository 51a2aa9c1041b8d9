// Neighbour attention and neighbour aggregation over a VoxelNeighbors table (spx_neighbor_attn_fwd / _bwd): every
// query attends over ITS OWN key set, the rows its table names -- Voxel Transformer's local / dilated attention,
// Stratified Transformer's and Swin3D's attention_step1 / attention_step2, Point Transformer's pointops.aggregation,
// attention-pooled RoI grids.  No grouped [M, S, C] row is ever written.
//
// Matrix instructions do not fit: a query shares its keys with no other query, so Q K^T and P V are batched
// matrix-VECTOR products (one row of Q against S gathered rows), and an MFMA tile would hold one useful row of 16 or
// 32.  The bound is the gather, 2 * S * C elements per query, so the design keeps 16-byte row pieces in flight.
//
//   WORK UNIT   (query m, head h), owned by LG = D / piece lanes (piece = 16 bytes: 8 elements at 16 bits, 4 at fp32;
//               LG = 1 .. 32).  Adjacent units are adjacent heads of one query, so the lanes of a wave fetch one
//               contiguous stretch of a key row; a query may span waves (heads are independent: C = 48, 96, 192 cost
//               nothing).  The head's dot product is a xor-shuffle sum inside the lane group.
//   FORWARD     q piece in registers; the workgroup's slice of `rows` staged through LDS
//               with coalesced loads (in chunks of `sc` slots when the slice is larger than the stage); key slots walked
//               kAhead at a time, the k and v pieces of all of them in flight together; online softmax in fp32 in the
//               log2 domain, the running maximum -inf until the first key; fp32 accumulators, one rounding, one 16-byte
//               store per lane.  With P != NULL the logits are parked in P and normalised in a last pass by the lane
//               that parked them (slot s belongs to lane s mod LG of its unit: a thread re-reads its own stores only).
//               The bias is read from global memory directly: one unit reads each element once, LDS would add nothing.
//   BACKWARD Q  the same split.  Walk 1 gathers v: dP[s] = dO . v_s (parked in dS), delta = sum P dP in fp32.  Walk 2
//               gathers k: dS = P (dP - delta), written (= dbias), dq = scale * sum dS k_s.
//   BACKWARD K  items (row r, head h) lane groups over the transposed list (segment_of of piece.h): for the entries e of
//               r in ascending order, m = e / S: dk += dS[e, h] q[m, h], dv += P[e, h] dO[m, h]; dk scaled once at the
//               end.  One writer per output element, no atomics: identical run to run.
//   AGGREGATE   the same three kernels with AGG = true: the weights are given (w in place of P, per group), there is no
//               q, k or softmax; backward Q writes dw = dO . v_s, backward K writes dv.
//
// Every table entry and list entry is range-checked before it addresses anything; loops are bounded by S or by the
// segment; no spin, grid barrier, cooperative launch, memset or atomic.
#include <cmath>

#include "piece.h"

namespace spx {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxSample = 128;
constexpr int kMaxChannels = 512;
constexpr int kStage = 4096;                      // int32 entries of `rows` a workgroup stages in LDS (16 KB)
constexpr float kLog2e = 1.4426950408889634f;
constexpr int kModeAttention = 0, kModeAggregate = 1;

struct QueryArgs {                                // the forward and the query side of the backward
  const void *q, *k, *v, *dout;
  long long ldk, ldv;                             // row strides of k and v, in elements
  const int32_t *rows;
  const float *bias;
  const void *w;                                  // AGG: the weights [M, S, H], fp32 (w_f32) or the rows' type
  int w_f32;
  int M, S, n;
  const int32_t *n_live;
  int H, sc;                                      // sc: slots per staged chunk (nq * sc <= kStage)
  float scale;
  void *out;                                      // forward: out; backward: dq
  float *P;                                       // forward: written (or NULL); backward: read
  void *ds;                                       // backward: dS fp32, or dw in w's type (AGG)
};

struct KeyArgs {
  const void *q, *dout;
  const float *ds;
  const void *P;                                  // P fp32, or w (AGG)
  int w_f32;
  const int32_t *offsets, *list;
  int M, S, n;
  const int32_t *n_live;
  int H;
  float scale;
  void *dk, *dv;
};

__device__ __forceinline__ int live_rows(const int32_t *n_live, int n) {
  const int live = n_live ? min(*n_live, n) : n;
  return live < 0 ? 0 : live;
}

template <int LG> __device__ __forceinline__ float group_sum(float x) {
#pragma unroll
  for (int o = LG >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

template <int DT, int V>
__device__ __forceinline__ float dot_piece(const float (&a)[V], const Piece<typename Elem<DT>::S, V> &b) {
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < V; ++j) d += a[j] * Elem<DT>::up(b.e[j]);
  return d;
}

// sum += a * b.  COMP: Kahan's compensated form, `low` carrying what the additions so far rounded away
template <bool COMP> __device__ __forceinline__ void add_term(float &sum, float &low, float a, float b) {
  if constexpr (COMP) {
    const float y = fmaf(a, b, -low), t = sum + y;
    low = (t - sum) - y;
    sum = t;
  } else {
    sum = fmaf(a, b, sum);
  }
}

template <int DT> __device__ __forceinline__ float load_weight(const void *w, int w_f32, long long i) {
  return w_f32 ? static_cast<const float *>(w)[i] : Elem<DT>::up(static_cast<const typename Elem<DT>::S *>(w)[i]);
}

// The queries a workgroup's units belong to and one unit's place among them.
struct Units {
  bool active;
  int m0, nq, m, h, sub;
};

template <int LGS> __device__ __forceinline__ Units units_of(int M, int H) {
  constexpr int LG = 1 << LGS, UPB = kBlock / LG;
  const long long total = static_cast<long long>(M) * H;
  const long long u0 = static_cast<long long>(blockIdx.x) * UPB, u = u0 + (threadIdx.x >> LGS);
  const long long last = (u0 + UPB < total ? u0 + UPB : total) - 1;
  Units t;
  t.active = u < total;
  t.m0 = static_cast<int>(u0 / H);
  t.nq = static_cast<int>(last / H) - t.m0 + 1;
  t.m = t.active ? static_cast<int>(u / H) : t.m0;
  t.h = t.active ? static_cast<int>(u - static_cast<long long>(t.m) * H) : 0;
  t.sub = threadIdx.x & (LG - 1);
  return t;
}

// slots [s0, s0 + sc) of the workgroup's queries into LDS, coalesced; returns the unit's own slice
__device__ __forceinline__ const int32_t *stage_rows(int32_t *srows, const int32_t *__restrict__ rows, const Units &t, int S,
                                                     int s0, int sc) {
  __syncthreads();
  const int cnt = min(t.nq * sc, kStage);
  for (int i = threadIdx.x; i < cnt; i += kBlock) {
    const int qi = i / sc;
    srows[i] = rows[static_cast<long long>(t.m0 + qi) * S + s0 + (i - qi * sc)];
  }
  __syncthreads();
  return srows + (t.m - t.m0) * sc;
}

// the rows of kAhead slots, -1 for what is no key: outside [0, live), beyond the chunk, an idle unit
__device__ __forceinline__ void batch_rows(const int32_t *mine, int j0, int sc, bool active, int live, int (&r)[kAhead]) {
#pragma unroll
  for (int u = 0; u < kAhead; ++u) {
    r[u] = (active && j0 + u < sc) ? mine[j0 + u] : -1;
    if (static_cast<unsigned>(r[u]) >= static_cast<unsigned>(live)) r[u] = -1;
  }
}

template <int DT, int LGS, bool AGG>
__global__ void __launch_bounds__(kBlock)
nattn_fwd_kernel(QueryArgs a) {
  using E = Elem<DT>;
  using T = typename E::S;
  constexpr int V = 16 / static_cast<int>(sizeof(T)), LG = 1 << LGS, D = LG * V;
  using Pc = Piece<T, V>;
  __shared__ int32_t srows[kStage];
  const Units t = units_of<LGS>(a.M, a.H);
  const int live = live_rows(a.n_live, a.n);
  const int C = a.H * D, col = t.h * D + t.sub * V;
  const long long e0 = static_cast<long long>(t.m) * a.S;
  const T *k = static_cast<const T *>(a.k), *v = static_cast<const T *>(a.v);
  constexpr bool kComp = DT == SPX_F32;             // fp32 rows: compensated sums, so S terms cost one rounding
  float qf[V], acc[V], low[V], llow = 0.f;
#pragma unroll
  for (int j = 0; j < V; ++j) qf[j] = 0.f, acc[j] = 0.f, low[j] = 0.f;
  if constexpr (!AGG) {
    if (t.active) {
      const Pc qp = *reinterpret_cast<const Pc *>(static_cast<const T *>(a.q) + static_cast<long long>(t.m) * C + col);
#pragma unroll
      for (int j = 0; j < V; ++j) qf[j] = E::up(qp.e[j]);
    }
  }
  const float f = a.scale * kLog2e;                // (the logit enters the log2 domain in one fused multiply-add)
  float mx = -INFINITY, l = 0.f;
  for (int s0 = 0; s0 < a.S; s0 += a.sc) {
    const int sc = min(a.sc, a.S - s0);
    const int32_t *mine = stage_rows(srows, a.rows, t, a.S, s0, sc);
    for (int j0 = 0; j0 < sc; j0 += kAhead) {
      int r[kAhead];
      Pc kp[kAhead], vp[kAhead];
      float b[kAhead];
      batch_rows(mine, j0, sc, t.active, live, r);
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {          // (the pieces of kAhead slots in flight together)
        const long long i = (e0 + s0 + j0 + u) * a.H + t.h;
        kp[u] = Pc{}, vp[u] = Pc{}, b[u] = 0.f;
        if (r[u] < 0) continue;
        vp[u] = *reinterpret_cast<const Pc *>(v + static_cast<long long>(r[u]) * a.ldv + col);
        if constexpr (AGG) {
          b[u] = load_weight<DT>(a.w, a.w_f32, i);
        } else {
          kp[u] = *reinterpret_cast<const Pc *>(k + static_cast<long long>(r[u]) * a.ldk + col);
          if (a.bias) b[u] = a.bias[i];
        }
      }
      if constexpr (AGG) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
#pragma unroll
          for (int j = 0; j < V; ++j) add_term<kComp>(acc[j], low[j], b[u], E::up(vp[u].e[j]));
      } else {
        float x[kAhead], mnew = mx;
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          const float d = group_sum<LG>(dot_piece<DT, V>(qf, kp[u]));
          x[u] = r[u] >= 0 ? fmaf(d, f, b[u] * kLog2e) : -INFINITY;
          mnew = fmaxf(mnew, x[u]);
        }
        const bool none = mnew == -INFINITY;      // no key so far: nothing to rescale, nothing to add
        const float alpha = none ? 1.f : exp2f(mx - mnew);
        l *= alpha, llow *= alpha;
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] *= alpha, low[j] *= alpha;
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          const float p = (r[u] >= 0 && !none) ? exp2f(x[u] - mnew) : 0.f;
          add_term<kComp>(l, llow, p, 1.f);
#pragma unroll
          for (int j = 0; j < V; ++j) add_term<kComp>(acc[j], low[j], p, E::up(vp[u].e[j]));
          const int s = s0 + j0 + u;
          if (a.P && t.active && j0 + u < sc && (s & (LG - 1)) == t.sub) a.P[(e0 + s) * a.H + t.h] = x[u];
        }
        mx = mnew;
      }
    }
  }
  if (!t.active) return;
  const float den = (AGG || l == 0.f) ? 1.f : l;   // (a query without a key: acc is +0; one correctly rounded divide)
  Pc o;
#pragma unroll
  for (int j = 0; j < V; ++j) o.e[j] = E::down(acc[j] / den);
  *reinterpret_cast<Pc *>(static_cast<T *>(a.out) + static_cast<long long>(t.m) * C + col) = o;
  if constexpr (!AGG) {
    if (a.P)
      for (int s = t.sub; s < a.S; s += LG) {     // (this lane's own stores: the logits become probabilities)
        const long long i = (e0 + s) * a.H + t.h;
        const float x = a.P[i];
        a.P[i] = x == -INFINITY ? 0.f : exp2f(x - mx) / den;
      }
  }
}

template <int DT, int LGS, bool AGG>
__global__ void __launch_bounds__(kBlock)
nattn_bwd_query_kernel(QueryArgs a) {
  using E = Elem<DT>;
  using T = typename E::S;
  constexpr int V = 16 / static_cast<int>(sizeof(T)), LG = 1 << LGS, D = LG * V;
  using Pc = Piece<T, V>;
  __shared__ int32_t srows[kStage];
  const Units t = units_of<LGS>(a.M, a.H);
  const int live = live_rows(a.n_live, a.n);
  const int C = a.H * D, col = t.h * D + t.sub * V;
  const long long e0 = static_cast<long long>(t.m) * a.S;
  const T *k = static_cast<const T *>(a.k), *v = static_cast<const T *>(a.v);
  float *ds = static_cast<float *>(a.ds);
  float dof[V], acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) dof[j] = 0.f, acc[j] = 0.f;
  if (t.active) {
    const Pc dp = *reinterpret_cast<const Pc *>(static_cast<const T *>(a.dout) + static_cast<long long>(t.m) * C + col);
#pragma unroll
    for (int j = 0; j < V; ++j) dof[j] = E::up(dp.e[j]);
  }
  // walk 1: v.  dP[s] = dO . v_s; AGG: that is dw; else parked in dS, delta = sum P dP
  float delta = 0.f;
  for (int s0 = 0; s0 < a.S; s0 += a.sc) {
    const int sc = min(a.sc, a.S - s0);
    const int32_t *mine = stage_rows(srows, a.rows, t, a.S, s0, sc);
    for (int j0 = 0; j0 < sc; j0 += kAhead) {
      int r[kAhead];
      Pc vp[kAhead];
      float p[kAhead];
      batch_rows(mine, j0, sc, t.active, live, r);
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        vp[u] = Pc{}, p[u] = 0.f;
        if (r[u] < 0) continue;
        vp[u] = *reinterpret_cast<const Pc *>(v + static_cast<long long>(r[u]) * a.ldv + col);
        if constexpr (!AGG) p[u] = a.P[(e0 + s0 + j0 + u) * a.H + t.h];
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const float dP = group_sum<LG>(dot_piece<DT, V>(dof, vp[u]));     // (+0 for a slot that is no key)
        delta += p[u] * dP;
        const int s = s0 + j0 + u;
        if (!(t.active && j0 + u < sc && (s & (LG - 1)) == t.sub)) continue;
        const long long i = (e0 + s) * a.H + t.h;
        if constexpr (!AGG) ds[i] = dP;
        else if (a.w_f32) ds[i] = dP;
        else static_cast<T *>(a.ds)[i] = E::down(dP);
      }
    }
  }
  if constexpr (AGG) return;
  // walk 2: k.  dS = P (dP - delta), dq = scale * sum dS k_s
  const int lane0 = (threadIdx.x & (kWave - 1)) & ~(LG - 1);
  for (int s0 = 0; s0 < a.S; s0 += a.sc) {
    const int sc = min(a.sc, a.S - s0);
    const int32_t *mine = stage_rows(srows, a.rows, t, a.S, s0, sc);
    for (int j0 = 0; j0 < sc; j0 += kAhead) {
      int r[kAhead];
      Pc kp[kAhead];
      float p[kAhead], dP[kAhead];
      batch_rows(mine, j0, sc, t.active, live, r);
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int s = s0 + j0 + u;
        const long long i = (e0 + s) * a.H + t.h;
        const bool own = t.active && j0 + u < sc && (s & (LG - 1)) == t.sub;
        kp[u] = Pc{}, p[u] = 0.f;
        dP[u] = own ? ds[i] : 0.f;                // (this lane's own store of walk 1)
        if (r[u] < 0) continue;
        kp[u] = *reinterpret_cast<const Pc *>(k + static_cast<long long>(r[u]) * a.ldk + col);
        p[u] = a.P[i];
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int s = s0 + j0 + u;
        const float dPs = __shfl(dP[u], lane0 + (s & (LG - 1)));
        const float dS = r[u] >= 0 ? p[u] * (dPs - delta) : 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += dS * E::up(kp[u].e[j]);
        if (t.active && j0 + u < sc && (s & (LG - 1)) == t.sub) ds[(e0 + s) * a.H + t.h] = dS;
      }
    }
  }
  if (!t.active) return;
  Pc o;
#pragma unroll
  for (int j = 0; j < V; ++j) o.e[j] = E::down(acc[j] * a.scale);
  *reinterpret_cast<Pc *>(static_cast<T *>(a.out) + static_cast<long long>(t.m) * C + col) = o;
}

template <int DT, int LGS, bool AGG>
__global__ void __launch_bounds__(kBlock)
nattn_bwd_key_kernel(KeyArgs a) {
  using E = Elem<DT>;
  using T = typename E::S;
  constexpr int V = 16 / static_cast<int>(sizeof(T)), LG = 1 << LGS, D = LG * V;
  using Pc = Piece<T, V>;
  const long long total = (static_cast<long long>(a.n) * a.H) << LGS;
  const int live = live_rows(a.n_live, a.n);
  const int entries = a.M * a.S, C = a.H * D;
  const T *q = static_cast<const T *>(a.q), *dout = static_cast<const T *>(a.dout);
  for (long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * kBlock) {
    const long long unit = item >> LGS;
    const int r = static_cast<int>(unit / a.H), h = static_cast<int>(unit - static_cast<long long>(r) * a.H);
    const Segment g = segment_of((static_cast<long long>(r) << LGS) | (item & (LG - 1)), LGS, live, a.offsets, entries);
    const int col = h * D + g.sub * V;
    constexpr bool kComp = DT == SPX_F32;           // (a row that hundreds of entries name: compensated in fp32)
    float ak[V], av[V], lk[V], lv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) ak[j] = 0.f, av[j] = 0.f, lk[j] = 0.f, lv[j] = 0.f;
    for (int j0 = g.beg; j0 < g.end; j0 += kAhead) {
      int e[kAhead];
      Pc qp[kAhead], dp[kAhead];
      float s[kAhead], p[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        e[u] = j0 + u < g.end ? a.list[j0 + u] : -1;
        if (static_cast<unsigned>(e[u]) >= static_cast<unsigned>(entries)) e[u] = -1;
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {          // (the loads of kAhead entries in flight together)
        qp[u] = Pc{}, dp[u] = Pc{}, s[u] = 0.f, p[u] = 0.f;
        if (e[u] < 0) continue;
        const long long i = static_cast<long long>(e[u]) * a.H + h;
        const long long at = static_cast<long long>(static_cast<unsigned>(e[u]) / static_cast<unsigned>(a.S)) * C + col;
        dp[u] = *reinterpret_cast<const Pc *>(dout + at);
        if constexpr (AGG) {
          p[u] = load_weight<DT>(a.P, a.w_f32, i);
        } else {
          qp[u] = *reinterpret_cast<const Pc *>(q + at);
          s[u] = a.ds[i];
          p[u] = static_cast<const float *>(a.P)[i];
        }
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {          // (the additions in list order)
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if constexpr (!AGG) add_term<kComp>(ak[j], lk[j], s[u], E::up(qp[u].e[j]));
          add_term<kComp>(av[j], lv[j], p[u], E::up(dp[u].e[j]));
        }
      }
    }
    Pc ok, ov;
#pragma unroll
    for (int j = 0; j < V; ++j) ok.e[j] = E::down(ak[j] * a.scale), ov.e[j] = E::down(av[j]);
    const long long at = static_cast<long long>(r) * C + col;
    if constexpr (!AGG) *reinterpret_cast<Pc *>(static_cast<T *>(a.dk) + at) = ok;
    *reinterpret_cast<Pc *>(static_cast<T *>(a.dv) + at) = ov;
  }
}

// ------------------------------------------------------------------------------------------------ host side

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

// f(dt, lgs): the instance of (dtype, head size); lgs = log2 of the lanes of a unit
template <typename F> void dispatch_unit(int dtype, int D, F &&f) {
  dispatch_value<SPX_F32, SPX_F16, SPX_BF16>(dtype, [&](auto dt) {
    constexpr int V = 16 / static_cast<int>(sizeof(typename Elem<decltype(dt)::value>::S));
    dispatch_value<8, 16, 32, 64, 128>(D, [&](auto d) {
      f(dt, std::integral_constant<int, ilog2(decltype(d)::value / V)>{});
    });
  });
}

// 0 = ok: the checks of every call that need no pointer
int check_shape(int M, int S, int n, int H, int D, int dtype, int mode, int w_dt) {
  SPX_CHECK(dtype == SPX_F32 || dtype == SPX_F16 || dtype == SPX_BF16, "dtype must be f32, f16 or bf16, got %d", dtype);
  SPX_CHECK(mode == kModeAttention || mode == kModeAggregate, "mode is 0 (attention) or 1 (aggregate), got %d", mode);
  SPX_CHECK(mode == kModeAttention || w_dt == SPX_F32 || w_dt == dtype, "w must be f32 or of the rows' dtype, got %d", w_dt);
  SPX_CHECK(D == 8 || D == 16 || D == 32 || D == 64 || D == 128, "the head size must be 8, 16, 32, 64 or 128, got %d", D);
  SPX_CHECK(H >= 1 && static_cast<long long>(H) * D <= kMaxChannels, "H * D must be in 1 .. %d, got %d x %d", kMaxChannels,
            H, D);
  SPX_CHECK(M >= 0 && n >= 0, "bad query / row counts %d / %d", M, n);
  SPX_CHECK(S >= 1 && S <= kMaxSample, "nsample must be in 1 .. %d, got %d", kMaxSample, S);
  SPX_CHECK(static_cast<long long>(M) * S < 0x80000000LL, "M * nsample must stay below 2^31, got %d x %d", M, S);
  return 0;
}

int check_rows_of(const char *name, const void *p, long long ld, int C, int eb) {
  SPX_CHECK(aligned_to(p, 16), "%s is not aligned to 16 bytes", name);
  SPX_CHECK(ld >= C && (ld * eb) % 16 == 0 && ld <= 0x7fffffffLL, "the row stride of %s must be >= C and a multiple of 16 "
            "bytes, got %lld elements", name, ld);
  return 0;
}

// grid and chunk of the two kernels whose units are (query, head)
void query_launch(int M, int S, int H, int lgs, unsigned *grid, int *sc) {
  const int upb = kBlock >> lgs;
  const long long total = static_cast<long long>(M) * H;
  *grid = static_cast<unsigned>((total + upb - 1) / upb);
  const int nq_max = (upb - 1) / H + 2;           // queries the units of one workgroup can touch
  const int fit = kStage / nq_max;                // >= 15
  *sc = S < fit ? S : fit;
}

}  // namespace
}  // namespace spx

extern "C" {

size_t spx_neighbor_attn_ws_bytes(int M, int S, int H) {
  if (M < 0 || S < 1 || S > spx::kMaxSample || H < 1 || H > spx::kMaxChannels / 8) return 0;
  if (static_cast<long long>(M) * S >= 0x80000000LL) return 0;
  return spx::align_up(static_cast<size_t>(M) * S * H * sizeof(float), 256);
}

int spx_neighbor_attn_fwd(const void *q, const void *k, const void *v, long long ldk, long long ldv, const int32_t *rows,
                          const float *bias, const void *w, int w_dt, int M, int S, int n, const int32_t *n_live, int H,
                          int D, int dtype, int mode, float scale, void *out, float *P, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_shape(M, S, n, H, D, dtype, mode, w_dt)) return rc;
  if (M == 0) return 0;
  const bool agg = mode == kModeAggregate;
  const int eb = elem_bytes(dtype), C = H * D;
  SPX_CHECK(rows && out && (agg ? w != nullptr : q != nullptr) && (n == 0 || (v && (agg || k))),
            "q / k / v / w / rows / out is NULL");
  SPX_CHECK(aligned_to(q, 16) && aligned_to(out, 16) && aligned_to(rows, 4) && aligned_to(bias, 4) && aligned_to(P, 4) &&
            aligned_to(w, w_dt == SPX_F32 ? 4 : 2), "q / out must be aligned to 16 bytes, tables to their elements");
  if (int rc = check_rows_of("v", v, ldv, C, eb)) return rc;
  if (!agg)
    if (int rc = check_rows_of("k", k, ldk, C, eb)) return rc;
  QueryArgs a = {};
  a.q = q, a.k = k, a.v = v, a.ldk = ldk, a.ldv = ldv, a.rows = rows, a.bias = agg ? nullptr : bias, a.w = w;
  a.w_f32 = w_dt == SPX_F32, a.M = M, a.S = S, a.n = n, a.n_live = n_live, a.H = H, a.scale = scale, a.out = out;
  a.P = agg ? nullptr : P;
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_unit(dtype, D, [&](auto dt, auto lgs) {
    unsigned grid;
    query_launch(M, S, H, lgs, &grid, &a.sc);
    if (agg) hipLaunchKernelGGL((nattn_fwd_kernel<dt, lgs, true>), dim3(grid), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((nattn_fwd_kernel<dt, lgs, false>), dim3(grid), dim3(kBlock), 0, s, a);
  });
  SPX_LAUNCH_CHECK();
  return 0;
}

int spx_neighbor_attn_bwd(const void *q, const void *k, const void *v, long long ldk, long long ldv, const int32_t *rows,
                          const void *pw, int w_dt, const void *d_out, const int32_t *offsets, const int32_t *list, int M,
                          int S, int n, const int32_t *n_live, int H, int D, int dtype, int mode, float scale, void *dq,
                          void *dk, void *dv, void *ds, spx_stream_t stream) {
  using namespace spx;
  if (int rc = check_shape(M, S, n, H, D, dtype, mode, w_dt)) return rc;
  const bool agg = mode == kModeAggregate;
  const int eb = elem_bytes(dtype), C = H * D;
  const bool key_side = dv != nullptr && n > 0, query_side = M > 0 && (agg ? ds != nullptr : true);
  SPX_CHECK(agg || (dk != nullptr) == (dv != nullptr), "dk and dv come together");
  SPX_CHECK(aligned_to(q, 16) && aligned_to(d_out, 16) && aligned_to(dq, 16) && aligned_to(dk, 16) && aligned_to(dv, 16) &&
            aligned_to(pw, agg && w_dt != SPX_F32 ? 2 : 4) && aligned_to(ds, agg && w_dt != SPX_F32 ? 2 : 4) &&
            aligned_to(rows, 4) && aligned_to(offsets, 4) && aligned_to(list, 4),
            "rows must be aligned to 16 bytes, tables to their elements");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (query_side) {
    SPX_CHECK(rows && d_out && pw && ds && (agg || (q && dq)) && (n == 0 || (v && (agg || k))),
              "q / k / v / rows / P / d_out / dq / ds is NULL");
    if (int rc = check_rows_of("v", v, ldv, C, eb)) return rc;
    if (!agg)
      if (int rc = check_rows_of("k", k, ldk, C, eb)) return rc;
    QueryArgs a = {};
    a.q = q, a.k = k, a.v = v, a.dout = d_out, a.ldk = ldk, a.ldv = ldv, a.rows = rows, a.w = pw, a.w_f32 = w_dt == SPX_F32;
    a.M = M, a.S = S, a.n = n, a.n_live = n_live, a.H = H, a.scale = scale, a.out = dq, a.ds = ds;
    a.P = agg ? nullptr : const_cast<float *>(static_cast<const float *>(pw));
    dispatch_unit(dtype, D, [&](auto dt, auto lgs) {
      unsigned grid;
      query_launch(M, S, H, lgs, &grid, &a.sc);
      if (agg) hipLaunchKernelGGL((nattn_bwd_query_kernel<dt, lgs, true>), dim3(grid), dim3(kBlock), 0, s, a);
      else hipLaunchKernelGGL((nattn_bwd_query_kernel<dt, lgs, false>), dim3(grid), dim3(kBlock), 0, s, a);
    });
    SPX_LAUNCH_CHECK();
  }
  if (key_side) {
    SPX_CHECK(offsets && (M == 0 || (list && d_out && pw && (agg || (q && ds)))),
              "offsets / list / q / P / ds / d_out is NULL");
    KeyArgs a = {q, d_out, agg ? nullptr : static_cast<const float *>(ds), pw, w_dt == SPX_F32, offsets, list, M, S, n,
                 n_live, H, scale, dk, dv};
    dispatch_unit(dtype, D, [&](auto dt, auto lgs) {
      const dim3 grid(stream_blocks((static_cast<long long>(n) * H) << lgs, kBlock));
      if (agg) hipLaunchKernelGGL((nattn_bwd_key_kernel<dt, lgs, true>), grid, dim3(kBlock), 0, s, a);
      else hipLaunchKernelGGL((nattn_bwd_key_kernel<dt, lgs, false>), grid, dim3(kBlock), 0, s, a);
    });
    SPX_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
