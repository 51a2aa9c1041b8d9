// Misaligned add: the union of up to eight coordinate sets and the merge of their feature rows
// (spx_union_count / _fill / _static, spx_union_add_fwd / _bwd).
//
// Replaces the torch composite behind functional.sparse_add_hash_based / sparse_add / AddTableMisaligned (reference
// spconv/pytorch/functional.py:439-545): T hash inserts + an arange whose count is read with .item(), T queries, T
// index_add_ (float atomics), T indexed index writes and a zero fill.
//
// The union is numbered through the level's RANK MAP (rankmap.h), as the sorted-order strided builds do -- no hash
// table, and no atomic on the path that numbers the rows:
//   mark    one launch over the rows of ALL operands: a plain byte store per live row into the byte-per-cell map
//           (idempotent: every writer stores 1).  A row is dead when it lies at or beyond *n_live of its operand, when
//           its batch index is outside [0, batch) or a coordinate outside its extent.
//   prefix  bytes -> {bits, prefix} words (conv4_prefix_kernel), then one block scans the blocks' totals and leaves
//           {union size, -, live = min(size, cap)} in the counters.
//   claim   one launch over all rows: rank of the row's key (one 8-byte load) and atomicMax(owner[t][rank], row).  The
//           owner tables ARE the src tables ([T][cap], -1 filled); of rows of one operand with one coordinate the highest
//           row owns the cell (as spx_dense_map), and whoever finds the entry taken raises the duplicate flag.  The
//           atomics decide ownership between duplicates only; every rank is fixed before this pass starts.  The same
//           pass counts the live rows per operand (a ballot per operand and wave).  The static form knows its row
//           count up front, so this pass also writes rows_t and out_indices there: five launches, nothing read back.
//   fill    (two-call form, after the host has read the count) rows_t, out_indices and the src tables in the numbering
//           the caller chose: ascending key (base = -1: row = rank), or operand b's own rows (base = b: the output row
//           of a key is the row of b that holds it).
// The merge is a gather-stream over the src tables: out[r] = sum over the operands present at r, in operand order, in
// fp32 (fp64 for SPX_F64), rounded once; every output element is written exactly once (no zero fill, no atomics); a row
// held by a single operand is copied bit for bit.  One launch for all operands: their pointers travel by value in the
// kernel's argument block.  The backward is a byte-moving gather, din_t[i] = dout[rows_t[i]], one launch as well.
#include "common.h"
#include "fill.h"
#include "piece.h"
#include "rankmap.h"
#include "scan.h"

namespace spx {
namespace {

constexpr int kBlock = 256;
static_assert(kBlock == kScanThreads, "scan.h's primitives are written for this unit's workgroup size");
constexpr int kMaxOps = SPX_UNION_MAX_OPERANDS;
constexpr int kCounters = 4 + kMaxOps;       // {union size, duplicate flag, live output rows, -, live rows of operand t}

// The operands of a build: index rows, device-side live counts (or null), and where each operand's rows start in the
// flat row space the kernels are launched over.
struct UnionOps {
  const int32_t *idx[kMaxOps];
  const int32_t *n_live[kMaxOps];
  int32_t *rows[kMaxOps];
  int off[kMaxOps + 1];
  int T;
};

// operand of flat row g (g < ops.off[ops.T])
__device__ __forceinline__ int operand_of(const int (&off)[kMaxOps + 1], int T, int g) {
  int t = 0;
#pragma unroll
  for (int j = 1; j < kMaxOps; ++j) t += (j < T && g >= off[j]) ? 1 : 0;
  return t;
}

// linear key of row i of operand t (level_key of rankmap.h over all axes), -1 for a dead row
__device__ __forceinline__ long long key_of(const UnionOps &ops, const LevelGeom &g, int t, int i) {
  const int32_t *nl = ops.n_live[t];
  if (nl && i >= *nl) return -1;
  return level_key(ops.idx[t] + static_cast<size_t>(i) * (g.ndim + 1), g, kAllAxes);
}

__global__ void __launch_bounds__(kBlock)
union_mark_kernel(UnionOps ops, LevelGeom g, uint8_t *__restrict__ occupied) {
  const int row = blockIdx.x * kBlock + threadIdx.x;
  if (row >= ops.off[ops.T]) return;
  const int t = operand_of(ops.off, ops.T, row);
  const long long key = key_of(ops, g, t, row - ops.off[t]);
  if (key >= 0) occupied[key] = 1;
}

// owner[t * stride + rank] = the highest row of operand t with that key; ranks >= cap are dropped.  DIRECT (static
// form: row = rank): rows_t and out_indices are written here as well.
template <bool DIRECT>
__global__ void __launch_bounds__(kBlock)
union_claim_kernel(UnionOps ops, LevelGeom g, const uint2 *__restrict__ cells, const int32_t *__restrict__ blockoff,
                   int32_t *__restrict__ owner, int stride, int cap, int32_t *__restrict__ counters,
                   int32_t *__restrict__ live_count, int32_t *__restrict__ out_indices) {
  const int row = blockIdx.x * kBlock + threadIdx.x;
  const bool in = row < ops.off[ops.T];
  int t = -1, i = 0;
  long long key = -1;
  if (in) {
    t = operand_of(ops.off, ops.T, row);
    i = row - ops.off[t];
    key = key_of(ops, g, t, i);
  }
  int r = -1;
  if (key >= 0) {
    r = rank_of(cells, blockoff, static_cast<unsigned long long>(key));
    if (r >= cap) r = -1;                 // an output beyond the caller's bound
  }
  if (r >= 0) {
    const int old = atomicMax(owner + static_cast<size_t>(t) * stride + r, i);
    if (old >= 0) counters[1] = 1;        // the entry was taken: a coordinate twice in one operand (idempotent store)
    if (DIRECT) {
      int32_t *o = out_indices + static_cast<size_t>(r) * (g.ndim + 1);      // (every holder of the key stores the same values)
      const int32_t *src = ops.idx[t] + static_cast<size_t>(i) * (g.ndim + 1);
      for (int d = 0; d <= g.ndim; ++d) o[d] = src[d];
    }
  }
  if (DIRECT && in) ops.rows[t][i] = r;
  // live rows per operand: one add per operand and wave
  for (int u = 0; u < ops.T; ++u) {
    const unsigned long long bal = __ballot(key >= 0 && t == u);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(live_count + u, __popcll(bal));
  }
}

// Two-call form, second phase.  Items [0, rows of all operands): rows_t (and out_indices in key order); items behind
// them: src[t][j] for every operand t and output row j.  base < 0: output row j holds rank j; base = b: output row j is
// row j of operand b (which covers the union and holds no coordinate twice: the host has seen both).
__global__ void __launch_bounds__(kBlock)
union_fill_kernel(UnionOps ops, LevelGeom g, const uint2 *__restrict__ cells, const int32_t *__restrict__ blockoff,
                  const int32_t *__restrict__ owner, int stride, int n_out, int base,
                  int32_t *__restrict__ out_indices, int32_t *__restrict__ src) {
  const long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const int n_rows = ops.off[ops.T];
  if (item < n_rows) {
    const int row = static_cast<int>(item);
    const int t = operand_of(ops.off, ops.T, row), i = row - ops.off[t];
    const long long key = key_of(ops, g, t, i);
    int r = key >= 0 ? rank_of(cells, blockoff, static_cast<unsigned long long>(key)) : -1;
    if (r >= stride) r = -1;
    int o = r;
    if (base >= 0 && r >= 0) o = owner[static_cast<size_t>(base) * stride + r];
    if (o >= n_out) o = -1;
    ops.rows[t][i] = o;
    if (base < 0 && o >= 0) {
      int32_t *dst = out_indices + static_cast<size_t>(o) * (g.ndim + 1);
      const int32_t *from = ops.idx[t] + static_cast<size_t>(i) * (g.ndim + 1);
      for (int d = 0; d <= g.ndim; ++d) dst[d] = from[d];
    }
    return;
  }
  const long long e = item - n_rows;
  if (e >= static_cast<long long>(ops.T) * n_out) return;
  const int t = static_cast<int>(e / n_out), j = static_cast<int>(e - static_cast<long long>(t) * n_out);
  int r = j;
  if (base >= 0) {
    const long long key = key_of(ops, g, base, j);
    r = key >= 0 ? rank_of(cells, blockoff, static_cast<unsigned long long>(key)) : -1;
  }
  src[e] = r >= 0 && r < stride ? owner[static_cast<size_t>(t) * stride + r] : -1;
}

// -------------------------------------------------------------------------------------------- row merge

struct AddOps {
  const void *feat[kMaxOps];
  int n[kMaxOps];
  int T;
};

template <int DT, int V>
__global__ void __launch_bounds__(kBlock)
union_add_fwd_kernel(AddOps ops, const int32_t *__restrict__ src, int n_out, int pieces, void *__restrict__ out_,
                     const int32_t *__restrict__ n_live) {
  using E = Elem<DT>;
  using S = typename E::S;
  using A = typename E::A;
  using P = Piece<S, V>;
  P *out = static_cast<P *>(out_);
  const long long total = static_cast<long long>(n_out) * pieces;
  const int live = n_live ? *n_live : n_out;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < total;
       i += static_cast<long long>(gridDim.x) * kBlock) {
    const int r = static_cast<int>(i / pieces);
    const int p = static_cast<int>(i - static_cast<long long>(r) * pieces);
    int s[kMaxOps];
#pragma unroll
    for (int t = 0; t < kMaxOps; ++t) {
      s[t] = (t < ops.T && r < live) ? src[static_cast<size_t>(t) * n_out + r] : -1;
      if (t < ops.T && static_cast<unsigned>(s[t]) >= static_cast<unsigned>(ops.n[t])) s[t] = -1;     // (checked, not trusted)
    }
    P v[kMaxOps];
#pragma unroll
    for (int t = 0; t < kMaxOps; ++t)       // (every present operand's load in flight together)
      if (s[t] >= 0) v[t] = static_cast<const P *>(ops.feat[t])[static_cast<long long>(s[t]) * pieces + p];
    int present = 0;
    P first;
    A acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      first.e[j] = S(0);
      acc[j] = A(0);
    }
#pragma unroll
    for (int t = 0; t < kMaxOps; ++t) {
      if (s[t] < 0) continue;
      if (present == 0) {
        first = v[t];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = E::up(v[t].e[j]);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += E::up(v[t].e[j]);
      }
      ++present;
    }
    if (present > 1) {                      // (a single operand: its bits as they are; none: zeros)
#pragma unroll
      for (int j = 0; j < V; ++j) first.e[j] = E::down(acc[j]);
    }
    out[i] = first;
  }
}

struct BwdOps {
  void *din[kMaxOps];
  const int32_t *rows[kMaxOps];
  int off[kMaxOps + 1];
  int T;
};

// din_t[i] = dout[rows_t[i]] or zeros, in pieces of sizeof(P) bytes
template <typename P>
__global__ void __launch_bounds__(kBlock)
union_add_bwd_kernel(BwdOps ops, const P *__restrict__ dout, int n_out, int pieces) {
  const long long total = static_cast<long long>(ops.off[ops.T]) * pieces;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < total;
       i += static_cast<long long>(gridDim.x) * kBlock) {
    const int row = static_cast<int>(i / pieces);
    const int p = static_cast<int>(i - static_cast<long long>(row) * pieces);
    const int t = operand_of(ops.off, ops.T, row), local = row - ops.off[t];
    const int r = ops.rows[t][local];
    P v = zero_piece<P>();
    if (static_cast<unsigned>(r) < static_cast<unsigned>(n_out)) v = dout[static_cast<long long>(r) * pieces + p];
    static_cast<P *>(ops.din[t])[static_cast<long long>(local) * pieces + p] = v;
  }
}

// -------------------------------------------------------------------------------------------- host side

// scratch of a build: the numbering's head (byte map, block totals), the counters, the owner tables [T][n_total]
struct UnionWs : RankScratch {
  int32_t *counters, *owner;
  size_t bytes;
  UnionWs(void *ws, size_t W, int T, long long n_total) {
    Carver c(ws);
    carve(c, W);
    counters = c.take<int32_t>(kCounters);
    owner = c.take<int32_t>(static_cast<size_t>(T) * static_cast<size_t>(n_total > 0 ? n_total : 1));
    bytes = c.off;
  }
};

struct Build {
  UnionOps ops;
  LevelGeom g;
  size_t W;
  int n_total;
};

// 0 = ok: checks the arguments every build call shares and fills b
int make_build(const int32_t *const *indices_h, const int *n_h, const int32_t *const *n_live_h, int T, int ndim,
               int batch, const int *spatial_h, const void *rankmap, size_t rankmap_bytes, Build &b) {
  SPX_CHECK(T >= 1 && T <= kMaxOps, "union of %d coordinate sets: 1 to %d operands", T, kMaxOps);
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  SPX_CHECK(indices_h && n_h && spatial_h, "indices / row counts / spatial shape is NULL");
  b.W = rank_words(ndim, batch, spatial_h);
  SPX_CHECK(b.W > 0 && rankmap && rankmap_bytes >= rank_bytes(b.W), "rank map missing or too small (%zu words)", b.W);
  b.g = LevelGeom(ndim, batch, spatial_h);
  long long total = 0;
  b.ops.T = T;
  for (int t = 0; t < kMaxOps; ++t) {
    b.ops.idx[t] = nullptr;
    b.ops.n_live[t] = nullptr;
    b.ops.rows[t] = nullptr;
  }
  for (int t = 0; t < T; ++t) {
    SPX_CHECK(n_h[t] >= 0 && (n_h[t] == 0 || indices_h[t]), "operand %d: bad row count %d or NULL indices", t, n_h[t]);
    b.ops.idx[t] = indices_h[t];
    b.ops.n_live[t] = n_live_h ? n_live_h[t] : nullptr;
    b.ops.off[t] = static_cast<int>(total);
    total += n_h[t];
    SPX_CHECK(total <= 0x7fffffffLL, "more than 2^31 - 1 rows in all");
  }
  for (int t = T; t <= kMaxOps; ++t) b.ops.off[t] = static_cast<int>(total);
  b.n_total = static_cast<int>(total);
  return 0;
}

// fill + mark + number_level: the rank map of the union and its size in counters[0] / [2]
int number_union(const Build &b, void *rankmap, const UnionWs &w, int32_t *counters, int cap, const FillList *more,
                 hipStream_t s) {
  {
    FillList fills;
    fills.add(w.occupied, b.W * 32, 0u);
    fills.add(w.counters, kCounters * sizeof(int32_t), 0u);
    if (counters != w.counters) fills.add(counters, 3 * sizeof(int32_t), 0u);
    if (more) fills.add(*more);
    SPX_HIP(fills.launch(s));
  }
  if (b.n_total > 0) {
    hipLaunchKernelGGL(union_mark_kernel, dim3(div_up(b.n_total, kBlock)), dim3(kBlock), 0, s, b.ops, b.g, w.occupied);
    SPX_LAUNCH_CHECK();
    count(kUnionMark);
  }
  SPX_HIP(number_level(w, b.W, rankmap, cap, counters, s));
  count(kUnionPrefix);
  return 0;
}

template <typename P>
void launch_add_bwd(const BwdOps &ops, const void *dout, int n_out, int pieces, hipStream_t s) {
  hipLaunchKernelGGL(union_add_bwd_kernel<P>, dim3(stream_blocks(static_cast<long long>(ops.off[ops.T]) * pieces, kBlock)),
                     dim3(kBlock), 0, s, ops, static_cast<const P *>(dout), n_out, pieces);
}

}  // namespace
}  // namespace spx

extern "C" {

size_t spx_union_ws_bytes(int ndim, int batch, const int *spatial_h, int T, long long n_total) {
  if (T < 1 || T > spx::kMaxOps || n_total < 0 || n_total > 0x7fffffffLL || !spatial_h) return 0;
  const size_t W = spx::rank_words(ndim, batch, spatial_h);
  return W ? spx::UnionWs(nullptr, W, T, n_total).bytes : 0;
}

int spx_union_count(const int32_t *const *indices_h, const int *n_h, const int32_t *const *n_live_h, int T, int ndim,
                    int batch, const int *spatial_h, void *rankmap, size_t rankmap_bytes, void *ws, size_t ws_bytes,
                    int *result_h, spx_stream_t stream) {
  using namespace spx;
  Build b;
  if (int rc = make_build(indices_h, n_h, n_live_h, T, ndim, batch, spatial_h, rankmap, rankmap_bytes, b)) return rc;
  SPX_CHECK(result_h, "result_h is required");
  UnionWs w(ws, b.W, T, b.n_total);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  FillList pre;
  pre.add(w.owner, sizeof(int32_t) * static_cast<size_t>(T) * (b.n_total > 0 ? b.n_total : 1), 0xFFFFFFFFu);
  if (int rc = number_union(b, rankmap, w, w.counters, -1, &pre, s)) return rc;
  if (b.n_total > 0) {
    hipLaunchKernelGGL(union_claim_kernel<false>, dim3(div_up(b.n_total, kBlock)), dim3(kBlock), 0, s, b.ops, b.g,
                       static_cast<const uint2 *>(rankmap), static_cast<const int32_t *>(rank_blockoff(rankmap, b.W)),
                       w.owner, b.n_total, b.n_total, w.counters, w.counters + 4, static_cast<int32_t *>(nullptr));
    SPX_LAUNCH_CHECK();
    count(kUnionClaim);
  }
  int32_t host[kCounters];
  SPX_HIP(hipMemcpyAsync(host, w.counters, sizeof(host), hipMemcpyDeviceToHost, s));
  SPX_HIP(hipStreamSynchronize(s));
  result_h[0] = host[0];
  result_h[1] = host[1];
  for (int t = 0; t < T; ++t) result_h[2 + t] = host[4 + t];
  return 0;
}

int spx_union_fill(const int32_t *const *indices_h, const int *n_h, const int32_t *const *n_live_h, int T, int ndim,
                   int batch, const int *spatial_h, int n_out, int base, int32_t *out_indices, int32_t *const *rows_h,
                   int32_t *src, const void *rankmap, size_t rankmap_bytes, const void *ws, size_t ws_bytes,
                   spx_stream_t stream) {
  using namespace spx;
  Build b;
  if (int rc = make_build(indices_h, n_h, n_live_h, T, ndim, batch, spatial_h, rankmap, rankmap_bytes, b)) return rc;
  SPX_CHECK(n_out >= 0 && n_out <= b.n_total, "n_out = %d outside [0, rows of all operands = %d]", n_out, b.n_total);
  SPX_CHECK(base >= -1 && base < T, "base = %d: -1 (key order) or an operand", base);
  SPX_CHECK(base < 0 || n_out == n_h[base], "base = %d: n_out must be that operand's row count %d, got %d", base,
            base < 0 ? 0 : n_h[base], n_out);
  SPX_CHECK(rows_h, "rows_h is required");
  for (int t = 0; t < T; ++t) {
    SPX_CHECK(n_h[t] == 0 || rows_h[t], "operand %d: rows is NULL", t);
    b.ops.rows[t] = rows_h[t];
  }
  SPX_CHECK(n_out == 0 || (src && (base >= 0 || out_indices)), "src / out_indices is NULL");
  UnionWs w(const_cast<void *>(ws), b.W, T, b.n_total);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  if (b.n_total == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  void *rm = const_cast<void *>(rankmap);
  const long long items = static_cast<long long>(b.n_total) + static_cast<long long>(T) * n_out;
  SPX_CHECK((items + kBlock - 1) / kBlock <= 0x7fffffffLL, "too many rows");
  hipLaunchKernelGGL(union_fill_kernel, dim3(static_cast<unsigned>((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     b.ops, b.g, static_cast<const uint2 *>(rm), static_cast<const int32_t *>(rank_blockoff(rm, b.W)),
                     static_cast<const int32_t *>(w.owner), b.n_total, n_out, base, out_indices, src);
  SPX_LAUNCH_CHECK();
  count(kUnionFill);
  return 0;
}

int spx_union_static(const int32_t *const *indices_h, const int *n_h, const int32_t *const *n_live_h, int T, int ndim,
                     int batch, const int *spatial_h, int n_out_cap, int32_t *out_indices, int32_t *const *rows_h,
                     int32_t *src, int32_t *n_out_dev, void *rankmap, size_t rankmap_bytes, void *ws, size_t ws_bytes,
                     spx_stream_t stream) {
  using namespace spx;
  Build b;
  if (int rc = make_build(indices_h, n_h, n_live_h, T, ndim, batch, spatial_h, rankmap, rankmap_bytes, b)) return rc;
  SPX_CHECK(n_out_cap > 0 && n_out_dev && out_indices && src && rows_h,
            "n_out_cap > 0, n_out_dev, out_indices, src and rows_h are required");
  for (int t = 0; t < T; ++t) {
    SPX_CHECK(n_h[t] == 0 || rows_h[t], "operand %d: rows is NULL", t);
    b.ops.rows[t] = rows_h[t];
  }
  UnionWs w(ws, b.W, T, b.n_total);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // every launch is stream-ordered and nothing is read back: the call can sit in a hipGraph.  Both sizes are known up
  // front, so the -1 fills of the outputs ride in the first fill launch (as spx_conv_rulebook_static)
  FillList pre;
  pre.add(out_indices, sizeof(int32_t) * static_cast<size_t>(n_out_cap) * (ndim + 1), 0xFFFFFFFFu);
  pre.add(src, sizeof(int32_t) * static_cast<size_t>(T) * n_out_cap, 0xFFFFFFFFu);
  if (int rc = number_union(b, rankmap, w, n_out_dev, n_out_cap, &pre, s)) return rc;
  if (b.n_total > 0) {
    hipLaunchKernelGGL(union_claim_kernel<true>, dim3(div_up(b.n_total, kBlock)), dim3(kBlock), 0, s, b.ops, b.g,
                       static_cast<const uint2 *>(rankmap), static_cast<const int32_t *>(rank_blockoff(rankmap, b.W)), src,
                       n_out_cap, n_out_cap, n_out_dev, w.counters + 4, out_indices);
    SPX_LAUNCH_CHECK();
    count(kUnionClaim);
  }
  return 0;
}

int spx_union_add_fwd(const void *const *feat_h, const int *n_h, int T, const int32_t *src, int n_out, int C, int dtype,
                      void *out, const int32_t *n_live, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(T >= 1 && T <= kMaxOps, "sum of %d operands: 1 to %d", T, kMaxOps);
  const int eb = float_row_elem(dtype, C);
  if (eb < 0) return eb;
  SPX_CHECK(n_out >= 0 && feat_h && n_h, "bad row count %d / NULL operand list", n_out);
  if (n_out == 0) return 0;
  SPX_CHECK(src && out, "src / out is NULL");
  AddOps ops;
  ops.T = T;
  bool vec = (static_cast<long long>(C) * eb) % 16 == 0 && aligned_to(out, 16);
  for (int t = 0; t < kMaxOps; ++t) {
    ops.feat[t] = nullptr;
    ops.n[t] = 0;
  }
  for (int t = 0; t < T; ++t) {
    SPX_CHECK(n_h[t] >= 0 && (n_h[t] == 0 || feat_h[t]), "operand %d: bad row count or NULL rows", t);
    SPX_CHECK(aligned_to(feat_h[t], eb), "operand %d: pointer not aligned to its elements", t);
    ops.feat[t] = feat_h[t];
    ops.n[t] = n_h[t];
    vec = vec && aligned_to(feat_h[t], 16);
  }
  SPX_CHECK(aligned_to(out, eb), "pointer not aligned to its elements");
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_row(dtype, vec, [&](auto dt, auto v) {
    const int pieces = C / v;
    hipLaunchKernelGGL((union_add_fwd_kernel<dt, v>), dim3(stream_blocks(static_cast<long long>(n_out) * pieces, kBlock)),
                       dim3(kBlock), 0, s, ops, src, n_out, pieces, out, n_live);
  });
  SPX_LAUNCH_CHECK();
  count(kUnionAddFwd);
  return 0;
}

int spx_union_add_bwd(const void *dout, int n_out, void *const *din_h, const int32_t *const *rows_h, const int *n_h,
                      int T, int C, int elem_bytes, spx_stream_t stream) {
  using namespace spx;
  SPX_CHECK(T >= 1 && T <= kMaxOps, "gradient of %d operands: 1 to %d", T, kMaxOps);
  SPX_CHECK(elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, "element size must be 2, 4 or 8 bytes, got %d",
            elem_bytes);
  SPX_CHECK(n_out >= 0 && C >= 1 && din_h && rows_h && n_h, "bad row count %d / channel count %d / NULL operand list",
            n_out, C);
  SPX_CHECK(n_out == 0 || dout, "dout is NULL");
  const long long row_bytes = static_cast<long long>(C) * elem_bytes;
  SPX_CHECK(row_bytes <= 0x7fffffffLL, "row too long");
  BwdOps ops;
  ops.T = T;
  long long total = 0;
  int v = piece_bytes(elem_bytes, row_bytes, {dout});
  for (int t = 0; t < kMaxOps; ++t) {
    ops.din[t] = nullptr;
    ops.rows[t] = nullptr;
  }
  for (int t = 0; t < T; ++t) {
    SPX_CHECK(n_h[t] >= 0 && (n_h[t] == 0 || (din_h[t] && rows_h[t])), "operand %d: bad row count or NULL din / rows", t);
    SPX_CHECK(aligned_to(din_h[t], elem_bytes), "operand %d: pointer not aligned to its elements", t);
    ops.din[t] = din_h[t];
    ops.rows[t] = rows_h[t];
    ops.off[t] = static_cast<int>(total);
    total += n_h[t];
    SPX_CHECK(total <= 0x7fffffffLL, "more than 2^31 - 1 rows in all");
    const int vt = piece_bytes(elem_bytes, row_bytes, {din_h[t]});
    v = vt < v ? vt : v;
  }
  for (int t = T; t <= kMaxOps; ++t) ops.off[t] = static_cast<int>(total);
  if (total == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int pieces = static_cast<int>(row_bytes / v);
  switch (v) {
    case 16: launch_add_bwd<uint4>(ops, dout, n_out, pieces, s); break;
    case 8: launch_add_bwd<unsigned long long>(ops, dout, n_out, pieces, s); break;
    case 4: launch_add_bwd<uint32_t>(ops, dout, n_out, pieces, s); break;
    default: launch_add_bwd<uint16_t>(ops, dout, n_out, pieces, s); break;
  }
  SPX_LAUNCH_CHECK();
  count(kUnionAddBwd);
  return 0;
}

}  // extern "C"
