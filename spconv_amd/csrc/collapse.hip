// Axis collapse: drop spatial axes of a sparse tensor, merge the rows that land on one projected cell
// (spx_collapse_count / _fill / _static, spx_collapse_fwd / _bwd).  Height compression of the fully sparse detectors:
// (batch, z, y, x) rows -> (batch, y, x) rows, reduced by sum, mean or max, the 2-D level behind in key order.
//
// The projected cells are numbered through the RANK MAP of the projected grid (rankmap.h: level_key over the kept axes,
// number_level), as the union numbers its coordinates -- no hash table, and no atomic on the path that numbers the rows:
//   mark    a plain byte store per live row into the byte-per-cell map of the PROJECTED grid (every writer stores 1),
//           and the live rows counted (a ballot per wave).  A row is dead when it lies at or beyond *n_live, when its
//           batch index is outside [0, batch) or any coordinate -- a removed one included -- outside its extent.
//   prefix  bytes -> {bits, prefix} words (conv4_prefix_kernel), then one block scans the blocks' totals and leaves
//           {cells found, -, live = min(found, cap)} in the counters.
//   rank    rows[i] = rank of the row's projected key (one 8-byte load), -1 for a dead row or a rank beyond the cap;
//           out_indices[rank] (every holder of a cell stores the same values); the row's SORT KEY = its rank, or
//           `capkey` = min(cap, n) for a dead row, so that dead rows trail; the kept rows counted.
//   list    a STABLE argsort of the rows by that key (the LSD radix of rowsort.hip on ceil(log2(capkey + 1)) bits) IS
//           the list: groups in rank order, ascending input row inside a group -- the order contract comes from the
//           sort's stability, no cursor is handed out.  One launch behind it finds the group boundaries in the sorted
//           order (offsets[r] = first position of rank r: every rank below `live` holds a row, so consecutive sorted
//           keys differ by at most one) and sets the entries from `live` on to the kept rows' count.
// The reduction gives an output row to a group of G lanes (G = a power of two covering the row's pieces, at most a
// wave: a full wave covers 64 x 16 bytes, narrow rows put 64 / G output rows in a wave; a wider row takes several
// passes).  A lane walks list[offsets[r] .. offsets[r + 1]) for its piece (the segment walk of piece.h: four entries'
// loads in flight, a group never split), the additions in list order in fp32 (fp64 for SPX_F64): the accumulator starts
// from the first row's value, one rounding at the end, a group of one row is copied bit for bit, every output element
// is written exactly once.
#include "common.h"
#include "fill.h"
#include "piece.h"
#include "rankmap.h"
#include "scan.h"

namespace spx {
namespace {

constexpr int kBlock = 256;
static_assert(kBlock == kScanThreads, "scan.h's primitives are written for this unit's workgroup size");
constexpr int kCounters = 4;          // {cells found, live input rows, live output rows, kept input rows}

struct CollapseGeom {
  LevelGeom level;                    // the INPUT level
  int kdim;                           // kept axes
  unsigned keep;                      // bit d: axis d stays
};

// linear key of row i on the PROJECTED grid (level_key of rankmap.h over the kept axes; a removed axis is still
// range-checked), -1 for a dead row
__device__ __forceinline__ long long key_of(const int32_t *__restrict__ idx, const int32_t *__restrict__ n_live,
                                            const CollapseGeom &g, int i) {
  if (n_live && i >= *n_live) return -1;
  return level_key(idx + static_cast<size_t>(i) * (g.level.ndim + 1), g.level, g.keep);
}

__global__ void __launch_bounds__(kBlock)
collapse_mark_kernel(const int32_t *__restrict__ idx, int n, const int32_t *__restrict__ n_live, CollapseGeom g,
                     uint8_t *__restrict__ occupied, int32_t *__restrict__ live_rows) {
  const int row = blockIdx.x * kBlock + threadIdx.x;
  const long long key = row < n ? key_of(idx, n_live, g, row) : -1;
  if (key >= 0) occupied[key] = 1;
  const unsigned long long bal = __ballot(key >= 0);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(live_rows, __popcll(bal));      // (an integer count: order-free)
}

__global__ void __launch_bounds__(kBlock)
collapse_rank_kernel(const int32_t *__restrict__ idx, int n, const int32_t *__restrict__ n_live, CollapseGeom g,
                     const uint2 *__restrict__ cells, const int32_t *__restrict__ blockoff, int cap, uint32_t capkey,
                     int32_t *__restrict__ rows, uint32_t *__restrict__ sortkey, int32_t *__restrict__ out_indices,
                     int32_t *__restrict__ kept_rows) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool in = i < n;
  const long long key = in ? key_of(idx, n_live, g, i) : -1;
  int r = -1;
  if (key >= 0) {
    r = rank_of(cells, blockoff, static_cast<unsigned long long>(key));
    if (r >= cap || static_cast<uint32_t>(r) >= capkey) r = -1;       // a cell beyond the caller's bound
  }
  if (in) {
    rows[i] = r;
    sortkey[i] = r >= 0 ? static_cast<uint32_t>(r) : capkey;
  }
  if (r >= 0) {
    int32_t *o = out_indices + static_cast<size_t>(r) * (g.kdim + 1);
    const int32_t *src = idx + static_cast<size_t>(i) * (g.level.ndim + 1);
    int c = 0;
    o[c++] = src[0];
    for (int d = 0; d < g.level.ndim; ++d)
      if ((g.keep >> d) & 1u) o[c++] = src[1 + d];
  }
  const unsigned long long bal = __ballot(r >= 0);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(kept_rows, __popcll(bal));
}

// Group boundaries of the sorted order: position t opens rank k when its key differs from the one before it; the
// offsets from the live count on (the end of the last group, and the static form's flat tail) = the kept rows.
__global__ void __launch_bounds__(kBlock)
collapse_list_kernel(const uint32_t *__restrict__ sortkey, const int32_t *__restrict__ list, int n, int cap,
                     uint32_t capkey, const int32_t *__restrict__ found, const int32_t *__restrict__ kept_rows,
                     int32_t *__restrict__ offsets) {
  const long long t = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (t < n) {
    const uint32_t k = sortkey[list[t]];
    const uint32_t prev = t > 0 ? sortkey[list[t - 1]] : 0xffffffffu;
    if (k < capkey && k != prev) offsets[k] = static_cast<int32_t>(t);
  }
  if (t <= cap) {
    const int f = *found;
    const int live = f < cap ? f : cap;
    if (t >= live) offsets[t] = *kept_rows;
  }
}

// -------------------------------------------------------------------------------------------- reduction

enum { kOpSum = SPX_COLLAPSE_SUM, kOpMean = SPX_COLLAPSE_MEAN, kOpMax = SPX_COLLAPSE_MAX };

// Items = (output row, lane of its group): G lanes per output row, lane `sub` owns the pieces sub, sub + G, ...
template <int DT, int V, int OP>
__global__ void __launch_bounds__(kBlock)
collapse_fwd_kernel(const void *__restrict__ feat_, int n, const int32_t *__restrict__ offsets,
                    const int32_t *__restrict__ list, int n_out, int pieces, int gshift, void *__restrict__ out_,
                    const int32_t *__restrict__ n_live) {
  using E = Elem<DT>;
  using S = typename E::S;
  using A = typename E::A;
  using P = Piece<S, V>;
  const P *feat = static_cast<const P *>(feat_);
  P *out = static_cast<P *>(out_);
  const long long total = static_cast<long long>(n_out) << gshift;
  const int live = n_live ? min(*n_live, n_out) : n_out;
  const int G = 1 << gshift;
  for (long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * kBlock) {
    const Segment g = segment_of(item, gshift, live, offsets, n);
    const int r = g.r, beg = g.beg, end = g.end;
    for (int p = g.sub; p < pieces; p += G) {
      P first;
      A acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        first.e[j] = S(0);
        acc[j] = A(0);
      }
      int present = 0;
      for (int j0 = beg; j0 < end; j0 += kAhead) {
        int s[kAhead];
        P v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          s[u] = j0 + u < end ? list[j0 + u] : -1;
          if (static_cast<unsigned>(s[u]) >= static_cast<unsigned>(n)) s[u] = -1;
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u)        // (the loads of four entries in flight together)
          if (s[u] >= 0) v[u] = feat[static_cast<long long>(s[u]) * pieces + p];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {      // (the additions in list order)
          if (s[u] < 0) continue;
          if (present == 0) {
            first = v[u];
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = E::up(v[u].e[j]);
          } else if (OP == kOpMax) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
              const A x = E::up(v[u].e[j]);
              // (the stored element travels: the output is a copy of an input element.  !(x <= acc) is x > acc or
              // unordered: the first NaN of the group in list order takes the element, and acc == acc keeps it there)
              if (!(x <= acc[j]) && acc[j] == acc[j]) {
                acc[j] = x;
                first.e[j] = v[u].e[j];
              }
            }
          } else {
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] += E::up(v[u].e[j]);
          }
          ++present;
        }
      }
      if (OP == kOpMean) {
        if (present > 0) {
#pragma unroll
          for (int j = 0; j < V; ++j) first.e[j] = E::down(acc[j] / static_cast<A>(present));
        }
      } else if (OP == kOpSum) {
        if (present > 1) {                      // (a single row: its bits as they are; none: zeros)
#pragma unroll
          for (int j = 0; j < V; ++j) first.e[j] = E::down(acc[j]);
        }
      }
      out[static_cast<long long>(r) * pieces + p] = first;
    }
  }
}

// mean: din[i] = dout[r] / count[r]; max: din[i, c] = dout[r, c] where feat[i, c] == out[r, c], or where both are NaN
// (the forward said NaN: the gradient goes to every NaN of the group, not to nobody); r = rows[i], zeros for a dead or
// dropped row.  One item per (input row, piece).
template <int DT, int V, int OP>
__global__ void __launch_bounds__(kBlock)
collapse_bwd_kernel(const void *__restrict__ feat_, const void *__restrict__ out_, const void *__restrict__ dout_,
                    const int32_t *__restrict__ rows, const int32_t *__restrict__ offsets, int n, int n_out, int pieces,
                    void *__restrict__ din_) {
  using E = Elem<DT>;
  using S = typename E::S;
  using A = typename E::A;
  using P = Piece<S, V>;
  const P *feat = static_cast<const P *>(feat_), *out = static_cast<const P *>(out_), *dout = static_cast<const P *>(dout_);
  P *din = static_cast<P *>(din_);
  const long long total = static_cast<long long>(n) * pieces;
  for (long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * kBlock) {
    const int i = static_cast<int>(item / pieces);
    const int p = static_cast<int>(item - static_cast<long long>(i) * pieces);
    const int r = rows[i];
    P v;
#pragma unroll
    for (int j = 0; j < V; ++j) v.e[j] = S(0);
    if (static_cast<unsigned>(r) < static_cast<unsigned>(n_out)) {
      const P g = dout[static_cast<long long>(r) * pieces + p];
      if (OP == kOpMean) {
        const int cnt = offsets[r + 1] - offsets[r];
        const A c = static_cast<A>(cnt > 0 ? cnt : 1);
#pragma unroll
        for (int j = 0; j < V; ++j) v.e[j] = E::down(E::up(g.e[j]) / c);
      } else {
        const P f = feat[item], o = out[static_cast<long long>(r) * pieces + p];
#pragma unroll
        for (int j = 0; j < V; ++j) {         // (ties all receive, as spx_maxpool_bwd; a NaN output: every NaN of the group)
          const A fv = E::up(f.e[j]), ov = E::up(o.e[j]);
          if (fv == ov || (fv != fv && ov != ov)) v.e[j] = g.e[j];
        }
      }
    }
    din[item] = v;
  }
}

// -------------------------------------------------------------------------------------------- host side

// scratch of a build: the numbering's head for the projected grid (byte map, block totals), the counters, the rows'
// sort keys, the radix sort's buffers
struct CollapseWs : RankScratch {
  int32_t *counters;
  uint32_t *sortkey;
  void *sort;
  size_t bytes;
  CollapseWs(void *ws, size_t W, int n) {
    Carver c(ws);
    carve(c, W);
    counters = c.take<int32_t>(kCounters);
    sortkey = c.take<uint32_t>(n > 0 ? n : 1);
    sort = c.take<char>(radix_argsort_ws_bytes(n));
    bytes = c.off;
  }
};

// words of the projected grid's rank map; 0 when the arguments describe no collapse or its key space does not fit
size_t projected_words(int ndim, int batch, const int *spatial_h, int axes_mask, int *kept_h /*[kMaxNdim]*/, int *kdim) {
  if (ndim < 1 || ndim > kMaxNdim || !spatial_h || axes_mask < 0 || (axes_mask >> ndim) != 0) return 0;
  int k = 0;
  for (int d = 0; d < ndim; ++d) {
    if (spatial_h[d] < 1) return 0;
    if (!((axes_mask >> d) & 1)) kept_h[k++] = spatial_h[d];
  }
  if (kdim) *kdim = k;
  return k ? rank_words(k, batch, kept_h) : 0;
}

struct Build {
  CollapseGeom g;
  size_t W;
};

// 0 = ok: the checks every build call shares, none of which looks at a pointer's target
int make_build(int n, int ndim, int batch, const int *spatial_h, int axes_mask, const void *rankmap, size_t rankmap_bytes,
               Build &b) {
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  SPX_CHECK(axes_mask >= 0 && (axes_mask >> ndim) == 0, "axes mask 0x%x names an axis >= ndim = %d", axes_mask, ndim);
  SPX_CHECK(axes_mask != (1 << ndim) - 1, "axes mask 0x%x removes every axis of %d: at least one stays", axes_mask, ndim);
  SPX_CHECK(n >= 0, "bad row count %d", n);
  SPX_CHECK(spatial_h, "spatial shape is NULL");
  int kept[kMaxNdim];
  b.W = projected_words(ndim, batch, spatial_h, axes_mask, kept, &b.g.kdim);
  SPX_CHECK(b.W > 0, "the projected key space does not fit a rank map (or the grid is empty)");
  SPX_CHECK(rankmap && rankmap_bytes >= rank_bytes(b.W), "rank map missing or too small (%zu words)", b.W);
  b.g.level = LevelGeom(ndim, batch, spatial_h);
  b.g.keep = ~static_cast<unsigned>(axes_mask) & ((1u << ndim) - 1u);
  return 0;
}

// fill + mark + number_level: the rank map of the projected level, its size in counters[0] / [2]
int number_cells(const Build &b, const int32_t *indices, int n, const int32_t *n_live, void *rankmap, const CollapseWs &w,
                 int32_t *counters, int cap, const FillList *more, hipStream_t s) {
  {
    FillList fills;
    fills.add(w.occupied, b.W * 32, 0u);
    fills.add(w.counters, kCounters * sizeof(int32_t), 0u);
    if (counters != w.counters) fills.add(counters, 3 * sizeof(int32_t), 0u);
    if (more) fills.add(*more);
    SPX_HIP(fills.launch(s));
  }
  if (n > 0) {
    hipLaunchKernelGGL(collapse_mark_kernel, dim3(div_up(n, kBlock)), dim3(kBlock), 0, s, indices, n, n_live, b.g,
                       w.occupied, w.counters + 1);
    SPX_LAUNCH_CHECK();
    count(kCollapseMark);
  }
  SPX_HIP(number_level(w, b.W, rankmap, cap, counters, s));
  count(kCollapsePrefix);
  return 0;
}

// rank + sort + boundaries: rows, out_indices, list, offsets [cap + 1].  `found`: the device word that holds the cells
// found; w.counters[3] is zero on entry.
int list_rows(const Build &b, const int32_t *indices, int n, const int32_t *n_live, const void *rankmap, const CollapseWs &w,
              int cap, const int32_t *found, int32_t *out_indices, int32_t *rows, int32_t *offsets, int32_t *list,
              hipStream_t s) {
  const uint32_t capkey = static_cast<uint32_t>(cap < n ? cap : n);
  if (n > 0) {
    void *rm = const_cast<void *>(rankmap);
    hipLaunchKernelGGL(collapse_rank_kernel, dim3(div_up(n, kBlock)), dim3(kBlock), 0, s, indices, n, n_live, b.g,
                       static_cast<const uint2 *>(rm), static_cast<const int32_t *>(rank_blockoff(rm, b.W)), cap, capkey, rows,
                       w.sortkey, out_indices, w.counters + 3);
    SPX_LAUNCH_CHECK();
    count(kCollapseRank);
    if (int rc = radix_argsort(w.sortkey, n, key_bits(capkey), list, w.sort, s)) return rc;
  }
  const long long items = n > cap + 1 ? n : static_cast<long long>(cap) + 1;
  hipLaunchKernelGGL(collapse_list_kernel, dim3(static_cast<unsigned>((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     w.sortkey, list, n, cap, capkey, found, w.counters + 3, offsets);
  SPX_LAUNCH_CHECK();
  count(kCollapseList);
  return 0;
}

// the argument checks of the two reduction calls that need no pointer: the bytes of an element, or -1 with the error set
int check_reduce(int n, int n_out, int C, int dtype, int op) {
  const int eb = float_row_elem(dtype, C);
  if (eb < 0) return eb;
  SPX_CHECK(op == kOpSum || op == kOpMean || op == kOpMax, "op must be sum (0), mean (1) or max (2), got %d", op);
  SPX_CHECK(n >= 0 && n_out >= 0, "bad row counts %d / %d", n, n_out);
  return eb;
}

}  // namespace
}  // namespace spx

extern "C" {

size_t spx_collapse_ws_bytes(int ndim, int batch, const int *spatial_h, int axes_mask, long long n) {
  if (n < 0 || n > 0x7fffffffLL) return 0;
  int kept[spx::kMaxNdim];
  const size_t W = spx::projected_words(ndim, batch, spatial_h, axes_mask, kept, nullptr);
  return W ? spx::CollapseWs(nullptr, W, static_cast<int>(n)).bytes : 0;
}

int spx_collapse_count(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, const int *spatial_h,
                       int axes_mask, void *rankmap, size_t rankmap_bytes, void *ws, size_t ws_bytes, int *result_h,
                       spx_stream_t stream) {
  using namespace spx;
  Build b;
  if (int rc = make_build(n, ndim, batch, spatial_h, axes_mask, rankmap, rankmap_bytes, b)) return rc;
  SPX_CHECK(result_h && (n == 0 || indices), "result_h / indices is NULL");
  CollapseWs w(ws, b.W, n);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = number_cells(b, indices, n, n_live, rankmap, w, w.counters, -1, nullptr, s)) return rc;
  int32_t host[kCounters];
  SPX_HIP(hipMemcpyAsync(host, w.counters, sizeof(host), hipMemcpyDeviceToHost, s));
  SPX_HIP(hipStreamSynchronize(s));
  result_h[0] = host[0];
  result_h[1] = host[1];
  return 0;
}

int spx_collapse_fill(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, const int *spatial_h,
                      int axes_mask, int n_out, int32_t *out_indices, int32_t *rows, int32_t *offsets, int32_t *list,
                      const void *rankmap, size_t rankmap_bytes, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  Build b;
  if (int rc = make_build(n, ndim, batch, spatial_h, axes_mask, rankmap, rankmap_bytes, b)) return rc;
  SPX_CHECK(n_out >= 0 && n_out <= n, "n_out = %d outside [0, rows = %d]", n_out, n);
  SPX_CHECK(offsets && (n == 0 || (indices && rows && list)) && (n_out == 0 || out_indices),
            "indices / out_indices / rows / offsets / list is NULL");
  CollapseWs w(ws, b.W, n);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  {
    FillList fills;                   // (the kept rows' count starts at zero on every call)
    fills.add(w.counters + 3, sizeof(int32_t), 0u);
    SPX_HIP(fills.launch(s));
  }
  return list_rows(b, indices, n, n_live, rankmap, w, n_out, w.counters, out_indices, rows, offsets, list, s);
}

int spx_collapse_static(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, const int *spatial_h,
                        int axes_mask, int n_out_cap, int32_t *out_indices, int32_t *rows, int32_t *offsets, int32_t *list,
                        int32_t *n_out_dev, void *rankmap, size_t rankmap_bytes, void *ws, size_t ws_bytes,
                        spx_stream_t stream) {
  using namespace spx;
  Build b;
  if (int rc = make_build(n, ndim, batch, spatial_h, axes_mask, rankmap, rankmap_bytes, b)) return rc;
  SPX_CHECK(n_out_cap > 0 && n_out_dev && out_indices && offsets, "n_out_cap > 0, n_out_dev, out_indices and offsets are required");
  SPX_CHECK(n == 0 || (indices && rows && list), "indices / rows / list is NULL");
  CollapseWs w(ws, b.W, n);
  SPX_CHECK(ws && ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // every launch is stream-ordered and nothing is read back: the call can sit in a hipGraph.  The size is known up
  // front, so the -1 fill of the indices rides in the first fill launch (as spx_union_static)
  FillList pre;
  pre.add(out_indices, sizeof(int32_t) * static_cast<size_t>(n_out_cap) * (b.g.kdim + 1), 0xFFFFFFFFu);
  if (int rc = number_cells(b, indices, n, n_live, rankmap, w, n_out_dev, n_out_cap, &pre, s)) return rc;
  return list_rows(b, indices, n, n_live, rankmap, w, n_out_cap, n_out_dev, out_indices, rows, offsets, list, s);
}

int spx_collapse_fwd(const void *feat, int n, const int32_t *offsets, const int32_t *list, int n_out, int C, int dtype,
                     int op, void *out, const int32_t *n_live_out, spx_stream_t stream) {
  using namespace spx;
  const int eb = check_reduce(n, n_out, C, dtype, op);
  if (eb < 0) return eb;
  if (n_out == 0) return 0;
  SPX_CHECK(offsets && out && (n == 0 || (feat && list)), "feat / offsets / list / out is NULL");
  SPX_CHECK(aligned_to(feat, eb) && aligned_to(out, eb), "pointer not aligned to its elements");
  const bool vec = (static_cast<long long>(C) * eb) % 16 == 0 && aligned_to(out, 16) && aligned_to(feat, 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_row(dtype, vec, [&](auto dt, auto v) {
    const int pieces = C / v, gshift = group_shift(pieces);
    dispatch_value<kOpSum, kOpMean, kOpMax>(op, [&](auto o) {
      hipLaunchKernelGGL((collapse_fwd_kernel<dt, v, o>), dim3(stream_blocks(static_cast<long long>(n_out) << gshift, kBlock)),
                         dim3(kBlock), 0, s, feat, n, offsets, list, n_out, pieces, gshift, out, n_live_out);
    });
  });
  SPX_LAUNCH_CHECK();
  count(kCollapseFwd);
  return 0;
}

int spx_collapse_bwd(const void *feat, const void *out, const void *dout, const int32_t *rows, const int32_t *offsets, int n,
                     int n_out, int C, int dtype, int op, void *din, spx_stream_t stream) {
  using namespace spx;
  const int eb = check_reduce(n, n_out, C, dtype, op);
  if (eb < 0) return eb;
  SPX_CHECK(op != kOpSum, "the gradient of a sum is a gather: spx_union_add_bwd with one operand");
  if (n == 0) return 0;
  SPX_CHECK(rows && din && (n_out == 0 || dout), "rows / dout / din is NULL");
  SPX_CHECK(n_out == 0 || (op == kOpMean ? offsets != nullptr : feat && out), "mean needs offsets, max needs feat and out");
  SPX_CHECK(aligned_to(feat, eb) && aligned_to(out, eb) && aligned_to(dout, eb) && aligned_to(din, eb),
            "pointer not aligned to its elements");
  const bool vec = (static_cast<long long>(C) * eb) % 16 == 0 && aligned_to(feat, 16) && aligned_to(out, 16) &&
                   aligned_to(dout, 16) && aligned_to(din, 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_row(dtype, vec, [&](auto dt, auto v) {
    const int pieces = C / v;
    dispatch_value<kOpMean, kOpMax>(op, [&](auto o) {
      hipLaunchKernelGGL((collapse_bwd_kernel<dt, v, o>), dim3(stream_blocks(static_cast<long long>(n) * pieces, kBlock)),
                         dim3(kBlock), 0, s, feat, out, dout, rows, offsets, n, n_out, pieces, din);
    });
  });
  SPX_LAUNCH_CHECK();
  count(kCollapseBwd);
  return 0;
}

}  // extern "C"
