// Voxel query and neighbour grouping (spx_voxel_query, spx_group_fwd, spx_group_bwd): per query point the first
// `nsample` voxels of a sparse level inside a window of cells (and, optionally, a radius), and their rows gathered --
// the voxel_query / grouping_operation pair the two-stage detectors over sparse backbones are written with (Voxel
// R-CNN's Voxel RoI pooling, the voxel set abstraction of the PV-RCNN family).
//
//   query     the query's own cell is floorf((q - lo) / vsize), the voxeliser's expression.  The candidates are the
//             cells cell + o, |o_d| <= range_d, visited in ascending linear key (axis 0 outermost, the last axis
//             innermost); a candidate is a HIT when it lies inside the grid, a live row holds it and, with a radius,
//             its centre is closer than the radius.  The first nsample hits in visiting order are kept: rows
//             [n_cap, nsample], count [n_cap] = min(hits, nsample), offsets [n_cap, nsample, ndim] = centre - query.
//             A query belongs to a GROUP of W = 2^wshift lanes (1 .. 64, chosen on the host from the window); the
//             lanes of a group test the candidates of one round together and the round's hits take their slots in
//             visiting order, so the result does not depend on W.  The group leaves once nsample slots are taken.
//               hash form    a candidate is a CELL: a probe of the builders' table (table.h), built by lookup.h from
//                            the level's live rows; a ballot and a popcount of the lanes below give the slot.
//               ranked form  a candidate is an X-RUN, the 2 * range + 1 (at most 31) cells of one line of the window:
//                            one or two words of the rank map (rankmap.h) give its occupancy bits, the row of its
//                            first occupied cell is the number of occupied cells before the run, later ones take
//                            consecutive rows (the level is in key order).  A lane may bring several hits, so the
//                            slots come from a prefix sum over the lanes of the group.
//   forward   out[e] = vfeat[rows[e]] (zeros for -1): gather_rows of pointvoxel.hip over the flattened rows, one item per
//             (entry, piece), the bits moved unchanged.
//   backward  dvfeat[v] = sum of dout[e] over the entries e of voxel v's group, the segment walk of piece.h over the
//             transposed list (spx_point_groups over the flattened rows): no atomics, ascending e.
// The radius test and the offsets are fp32 with every operation rounded on its own, so a host loop reproduces every
// element bit for bit.
#include "common.h"
#include "lookup.h"
#include "piece.h"
#include "scenes.h"

// no multiply-add pair of this unit may be contracted into an FMA (see pointvoxel.hip)
#pragma clang fp contract(off)

namespace spx {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxRange = 15;         // a window line of 31 cells spans at most two 32-cell words of the rank map
constexpr int kMaxSample = 128;
static_assert(kRankWords == 1 << 11, "blockoff is indexed by word >> 11");
constexpr int kFlagRadius = 1, kFlagWidthShift = 8;      // (flags >> 8: 0, or 1 + log2 of a forced W; 2: kFlagPadFirst)

struct QueryGeom : PointGeom {
  int range[kPointDims];              // by grid axis (index-column order)
};

struct QueryArgs {
  const float *queries;
  int nfeat;
  const int32_t *batch_ids;
  int n_cap;
  const int32_t *n_queries;
  int wshift, nsample;
  float r2;
  int flags;
  int32_t *rows, *count;
  float *offsets;
};

// A query: its batch, its own cell by grid axis, its coordinates by point column.
template <int NDIM> struct Query {
  bool valid;
  int b;
  int cell[NDIM];
  float q[NDIM];
};

template <int NDIM>
__device__ __forceinline__ Query<NDIM> load_query(const QueryArgs &a, const QueryGeom &g, long long qi) {
  Query<NDIM> r;
  r.valid = point_batch(g, a.batch_ids, a.n_cap, a.n_queries, qi, r.b);
#pragma unroll
  for (int j = 0; j < NDIM; ++j) {
    r.q[j] = 0.f;
    r.cell[NDIM - 1 - j] = 0;
  }
  if (r.valid) {
    const float *pt = a.queries + static_cast<size_t>(qi) * a.nfeat;
#pragma unroll
    for (int j = 0; j < NDIM; ++j) {
      r.q[j] = pt[j];
      float cell;
      point_cell<NDIM>(g, j, r.q[j], cell, r.valid);
      r.cell[NDIM - 1 - j] = r.valid ? static_cast<int>(cell) : 0;
    }
  }
  return r;
}

// centre_j - q_j of the cell with coordinate v along the axis of point column j
__device__ __forceinline__ float centre_offset(const QueryGeom &g, int j, int v, float qj) {
  const float centre = (static_cast<float>(v) + 0.5f) * g.vsize[j] + g.lo[j];
  return centre - qj;
}

// the slots behind the kept hits: -1 / 0, or the first hit again (pad = first)
template <int NDIM>
__device__ __forceinline__ void finish_query(const QueryArgs &a, long long qi, int sub, int W, int cnt, int first_row,
                                             const float (&first_off)[NDIM]) {
  int32_t *ro = a.rows + qi * a.nsample;
  float *oo = a.offsets ? a.offsets + qi * a.nsample * NDIM : nullptr;
  if (cnt > a.nsample) cnt = a.nsample;
  const bool pad = (a.flags & kFlagPadFirst) && cnt > 0;
  for (int s = cnt + sub; s < a.nsample; s += W) {
    ro[s] = pad ? first_row : -1;
    if (oo) {
#pragma unroll
      for (int j = 0; j < NDIM; ++j) oo[s * NDIM + j] = pad ? first_off[j] : 0.f;
    }
  }
  if (sub == 0) a.count[qi] = cnt;
}

// Hash form.  Lane `sub` of the group tests candidate base + sub of the round.
template <int NDIM>
__global__ void __launch_bounds__(kBlock)
query_hash_kernel(QueryArgs a, QueryGeom g, LevelLookup look) {
  const long long qi = (static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x) >> a.wshift;
  if (qi >= a.n_cap) return;                                  // (a whole group: kBlock is a multiple of W)
  const int W = 1 << a.wshift, sub = threadIdx.x & (W - 1);
  const int gbase = (threadIdx.x & 63) & ~(W - 1);
  const unsigned long long gmask = W == 64 ? ~0ull : ((1ull << W) - 1ull);
  const RowFinder<false> row_at(look);
  const Query<NDIM> q = load_query<NDIM>(a, g, qi);
  int ext[NDIM], total = 1;
#pragma unroll
  for (int d = 0; d < NDIM; ++d) {
    ext[d] = 2 * g.range[d] + 1;
    total *= ext[d];
  }
  int32_t *ro = a.rows + qi * a.nsample;
  float *oo = a.offsets ? a.offsets + qi * a.nsample * NDIM : nullptr;
  int cnt = 0, first_row = -1;
  float first_off[NDIM] = {};
  if (q.valid) {
    for (int base = 0; base < total && cnt < a.nsample; base += W) {
      const int c = base + sub;
      int row = -1;
      float dj[NDIM] = {};
      if (c < total) {
        int o[NDIM], rem = c;
#pragma unroll
        for (int d = NDIM - 1; d >= 0; --d) {                 // the last axis fastest
          o[d] = rem % ext[d] - g.range[d];
          rem /= ext[d];
        }
        long long key = q.b;
        bool in = true;
#pragma unroll
        for (int d = 0; d < NDIM; ++d) {
          const int v = q.cell[d] + o[d];
          in = in && static_cast<unsigned>(v) < static_cast<unsigned>(g.level.dims[d]);
          key = key * g.level.dims[d] + v;
          dj[NDIM - 1 - d] = centre_offset(g, NDIM - 1 - d, v, q.q[NDIM - 1 - d]);
        }
        if (in && (!(a.flags & kFlagRadius) || dist2<NDIM>(dj) < a.r2)) row = row_at(key);
      }
      const unsigned long long hits = (__ballot(row >= 0) >> gbase) & gmask;
      if (row >= 0) {
        const int slot = cnt + __popcll(hits & ((1ull << sub) - 1ull));
        if (slot < a.nsample) {
          ro[slot] = row;
          if (oo) {
#pragma unroll
            for (int j = 0; j < NDIM; ++j) oo[slot * NDIM + j] = dj[j];
          }
        }
      }
      if (cnt == 0 && hits != 0ull) {                         // the first hit, for the padding
        const int src = gbase + __ffsll(hits) - 1;
        first_row = __shfl(row, src, 64);
#pragma unroll
        for (int j = 0; j < NDIM; ++j) first_off[j] = __shfl(dj[j], src, 64);
      }
      cnt += __popcll(hits);
    }
  }
  finish_query<NDIM>(a, qi, sub, W, cnt, first_row, first_off);
}

// Ranked form.  Lane `sub` of the group takes x-run base + sub of the round: the window's line at one offset along
// every axis but the last, clipped to the grid.
template <int NDIM>
__global__ void __launch_bounds__(kBlock)
query_ranked_kernel(QueryArgs a, QueryGeom g, LevelLookup look) {
  const long long qi = (static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x) >> a.wshift;
  if (qi >= a.n_cap) return;
  const int W = 1 << a.wshift, sub = threadIdx.x & (W - 1);
  const int gbase = (threadIdx.x & 63) & ~(W - 1);
  const unsigned long long gmask = W == 64 ? ~0ull : ((1ull << W) - 1ull);
  const int live = look.live();
  const uint2 *cells = look.cells;                            // (the words themselves: an x-run reads one or two)
  const int32_t *blockoff = look.blockoff;
  const Query<NDIM> q = load_query<NDIM>(a, g, qi);
  constexpr int X = NDIM - 1;                                 // the axis of a run; point column 0
  int ext[NDIM], runs = 1;
#pragma unroll
  for (int d = 0; d < X; ++d) {
    ext[d] = 2 * g.range[d] + 1;
    runs *= ext[d];
  }
  const int xlo = max(q.cell[X] - g.range[X], 0), xhi = min(q.cell[X] + g.range[X], g.level.dims[X] - 1);
  const int len = xhi - xlo + 1;                              // 1 .. 31 for a valid query
  int32_t *ro = a.rows + qi * a.nsample;
  float *oo = a.offsets ? a.offsets + qi * a.nsample * NDIM : nullptr;
  int cnt = 0, first_row = -1;
  float first_off[NDIM] = {};
  if (q.valid) {
    for (int base = 0; base < runs && cnt < a.nsample; base += W) {
      const int c = base + sub;
      uint32_t occ = 0u, hits = 0u;                           // bit i: cell xlo + i is occupied and live / is a hit
      int row0 = 0;                                           // occupied cells before the run = row of its first one
      float dj[NDIM] = {};
      if (c < runs) {
        int rem = c;
        unsigned long long key = static_cast<unsigned long long>(q.b);
        bool in = true;
        int v[NDIM];
#pragma unroll
        for (int d = X - 1; d >= 0; --d) {
          v[d] = q.cell[d] + rem % ext[d] - g.range[d];
          rem /= ext[d];
        }
#pragma unroll
        for (int d = 0; d < X; ++d) {
          in = in && static_cast<unsigned>(v[d]) < static_cast<unsigned>(g.level.dims[d]);
          key = key * g.level.dims[d] + v[d];
          dj[NDIM - 1 - d] = centre_offset(g, NDIM - 1 - d, v[d], q.q[NDIM - 1 - d]);
        }
        if (in) {
          key = key * g.level.dims[X] + xlo;
          const unsigned sh = static_cast<unsigned>(key & 31ull);
          const unsigned long long word = key >> 5;
          const uint2 w0 = cells[word];
          uint2 w1 = make_uint2(0u, 0u);
          if (sh + len > 32u) w1 = cells[word + 1];           // (the run's last cell lies there)
          const unsigned long long bits = w0.x | (static_cast<unsigned long long>(w1.x) << 32);
          occ = static_cast<uint32_t>(bits >> sh) & ((1u << len) - 1u);
          if (occ) {
            // the prefix of the word that holds the run's first occupied cell: a word without an occupied cell need
            // not carry one (rank_of never reads it, and spx_rankmap_from_sorted leaves such words zero)
            row0 = (w0.x >> sh) != 0u ? blockoff[word >> 11] + static_cast<int>(w0.y) + __popc(w0.x & ((1u << sh) - 1u))
                                      : blockoff[(word + 1) >> 11] + static_cast<int>(w1.y);
            const int room = live - row0;                     // rows ascend along the run: the first `room` are live
            if (room <= 0) occ = 0u;
            while (occ && __popc(occ) > room) occ &= ~(0x80000000u >> __clz(occ));
          }
          hits = occ;
          if (a.flags & kFlagRadius) {
            hits = 0u;
            for (uint32_t m = occ; m; m &= m - 1u) {
              const int bit = __ffs(m) - 1;
              dj[0] = centre_offset(g, 0, xlo + bit, q.q[0]);
              if (dist2<NDIM>(dj) < a.r2) hits |= 1u << bit;
            }
          }
        }
      }
      const int h = __popc(hits);
      int incl = h;                                           // inclusive prefix over the lanes of the group
      for (int d = 1; d < W; d <<= 1) {
        const int u = __shfl_up(incl, d, W);
        if (sub >= d) incl += u;
      }
      const int round = __shfl(incl, W - 1, W);
      int slot = cnt + incl - h;
      for (uint32_t m = hits; m && slot < a.nsample; m &= m - 1u, ++slot) {
        const int bit = __ffs(m) - 1;
        ro[slot] = row0 + __popc(occ & ((1u << bit) - 1u));
        if (oo) {
          dj[0] = centre_offset(g, 0, xlo + bit, q.q[0]);
#pragma unroll
          for (int j = 0; j < NDIM; ++j) oo[slot * NDIM + j] = dj[j];
        }
      }
      if (cnt == 0 && round != 0) {                           // the first hit, for the padding
        const unsigned long long any = (__ballot(h > 0) >> gbase) & gmask;
        const int src = gbase + __ffsll(any) - 1;
        const int bit = h > 0 ? __ffs(hits) - 1 : 0;
        dj[0] = centre_offset(g, 0, xlo + bit, q.q[0]);
        first_row = __shfl(row0 + __popc(occ & ((1u << bit) - 1u)), src, 64);
#pragma unroll
        for (int j = 0; j < NDIM; ++j) first_off[j] = __shfl(dj[j], src, 64);
      }
      cnt += round;
    }
  }
  finish_query<NDIM>(a, qi, sub, W, cnt, first_row, first_off);
}

// -------------------------------------------------------------------------------------------- grouping

// Items = (voxel row, lane of its group), the segment walk of piece.h over the transposed list: entry e brings the
// piece of dout row e.  (interp_bwd_kernel without the weight: its load and multiply would not fold away there.)
template <int DT, int V>
__global__ void __launch_bounds__(kBlock)
group_bwd_kernel(const void *__restrict__ dout_, int entries, const int32_t *__restrict__ offsets,
                 const int32_t *__restrict__ list, int n, int pieces, int gshift, const int32_t *__restrict__ n_live,
                 void *__restrict__ dvfeat_) {
  using E = Elem<DT>;
  using S = typename E::S;
  using A = typename E::A;
  using P = Piece<S, V>;
  const P *dout = static_cast<const P *>(dout_);
  P *dvfeat = static_cast<P *>(dvfeat_);
  const long long total = static_cast<long long>(n) << gshift;
  const int live = n_live ? min(*n_live, n) : n;
  const int G = 1 << gshift;
  for (long long item = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; item < total;
       item += static_cast<long long>(gridDim.x) * kBlock) {
    const Segment g = segment_of(item, gshift, live, offsets, entries);
    const int r = g.r, beg = g.beg, end = g.end;
    for (int p = g.sub; p < pieces; p += G) {
      A acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = A(0);
      for (int j0 = beg; j0 < end; j0 += kAhead) {
        int e[kAhead];
        P v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          e[u] = j0 + u < end ? list[j0 + u] : -1;
          if (static_cast<unsigned>(e[u]) >= static_cast<unsigned>(entries)) e[u] = -1;
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u)        // (the loads of four entries in flight together)
          if (e[u] >= 0) v[u] = dout[static_cast<long long>(e[u]) * pieces + p];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {      // (the additions in list order)
          if (e[u] < 0) continue;
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j] = acc[j] + E::up(v[u].e[j]);
        }
      }
      P o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.e[j] = E::down(acc[j]);
      dvfeat[static_cast<long long>(r) * pieces + p] = o;
    }
  }
}

// -------------------------------------------------------------------------------------------- host side

// 0 = ok: the checks of a query / grouping call over [n_cap, nsample] entries that need no pointer
int check_entries(int n_cap, int nsample, int n) {
  SPX_CHECK(n_cap >= 0 && n >= 0, "bad query / row counts %d / %d", n_cap, n);
  SPX_CHECK(nsample >= 1 && nsample <= kMaxSample, "nsample must be in 1 .. %d, got %d", kMaxSample, nsample);
  SPX_CHECK(static_cast<long long>(n_cap) * nsample < 0x80000000LL, "n_cap * nsample must stay below 2^31, got %d x %d",
            n_cap, nsample);
  return 0;
}

// the checks of the two grouping calls that need no pointer: the bytes of an element, or -1 with the error set
int check_group(int n_cap, int nsample, int n, int C, int dtype) {
  if (int rc = check_entries(n_cap, nsample, n)) return rc;
  return float_row_elem(dtype, C);
}

// log2 of the lanes of a query's group.  The group stops once nsample slots are taken, so lanes beyond the candidates
// that a typical query needs only idle: the width is the power of two covering the candidates, divided by 2^divide,
// at least 4 (or the candidates, if fewer) and at most a wave.  Measured at 110 592 queries over 120 000 voxels
// (profiles/query_probe.json, "width_sweep"): an eighth of the runs in the ranked form, a quarter of the cells in the
// hash form were the best or within 4 % of the best width at ranges 1, 2 and 4.
int width_shift(int candidates, int divide, int flags) {
  const int forced = flags >> kFlagWidthShift;
  if (forced) return forced - 1;
  int s = 0;
  while ((1 << s) < candidates) ++s;
  const int least = s < 2 ? s : 2;
  s -= divide;
  return s < least ? least : (s > 6 ? 6 : s);
}

}  // namespace
}  // namespace spx

extern "C" {

size_t spx_voxel_query_ws_bytes(int n_cap, int nsample, int ndim, int n, int ranked) {
  if ((ndim != 2 && ndim != 3) || n_cap < 0 || n < 0 || n > spx::kMaxRows) return 0;
  if (nsample < 1 || nsample > spx::kMaxSample || static_cast<long long>(n_cap) * nsample >= 0x80000000LL) return 0;
  return ranked ? 0 : spx::LevelTableWs(nullptr, n).bytes;
}

int spx_voxel_query(const float *queries, int nfeat, const int32_t *batch_ids, int n_cap, const int32_t *n_queries_dev,
                    int ndim, const float *vsize, const float *coors_range, const int32_t *indices, int n,
                    const int32_t *n_live, int batch, const int *spatial_h, const void *rankmap, size_t rankmap_bytes,
                    const int *query_range, int nsample, float r2, int flags, int32_t *rows, int32_t *count,
                    float *offsets, void *ws, size_t ws_bytes, spx_stream_t stream) {
  using namespace spx;
  LevelLookup look;
  if (int rc = check_level("queries", ndim, nfeat, n, n_live, batch, spatial_h, vsize, coors_range, rankmap, rankmap_bytes,
                           &look))
    return rc;
  if (int rc = check_entries(n_cap, nsample, n)) return rc;
  SPX_CHECK((flags & ~(kFlagRadius | kFlagPadFirst | (7 << kFlagWidthShift))) == 0,
            "flags must be radius (1) | pad first (2) | a group width (log2 + 1) << 8, got %d", flags);
  SPX_CHECK(!(flags & kFlagRadius) || r2 >= 0.f, "the squared radius must be >= 0 (and no NaN)");
  SPX_CHECK(query_range, "query_range is NULL");
  QueryGeom g{PointGeom(ndim, batch, spatial_h, vsize, coors_range), {}};
  int window = 1, runs = 1;
  for (int d = 0; d < kPointDims; ++d) {
    g.range[d] = d < ndim ? query_range[d] : 0;
    SPX_CHECK(g.range[d] >= 0 && g.range[d] <= kMaxRange, "query_range of axis %d must be in 0 .. %d, got %d", d, kMaxRange,
              g.range[d]);
    window *= 2 * g.range[d] + 1;
    if (d < ndim - 1) runs *= 2 * g.range[d] + 1;
  }
  if (n_cap == 0) return 0;
  SPX_CHECK(queries && rows && count && (n == 0 || indices), "queries / indices / rows / count is NULL");
  SPX_CHECK(aligned_to(queries, 4) && aligned_to(rows, 4) && aligned_to(count, 4) && aligned_to(offsets, 4),
            "pointer not aligned to its elements");
  QueryArgs a = {queries, nfeat, batch_ids, n_cap, n_queries_dev, 0, nsample, r2, flags, rows, count, offsets};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(kBlock);
  auto grid = [&](int wshift) { return dim3(static_cast<unsigned>(((static_cast<long long>(n_cap) << wshift) + kBlock - 1) / kBlock)); };
  if (rankmap) {
    a.wshift = width_shift(runs, 3, flags);
    dispatch_value<2, 3>(ndim, [&](auto nd) {
      hipLaunchKernelGGL((query_ranked_kernel<nd>), grid(a.wshift), block, 0, s, a, g, look);
    });
    SPX_LAUNCH_CHECK();
    spx::count(kQueryRanked);
    return 0;
  }
  if (int rc = build_level_table(ws, ws_bytes, indices, n, n_live, g.level, &look.table, s)) return rc;
  a.wshift = width_shift(window, 2, flags);
  dispatch_value<2, 3>(ndim, [&](auto nd) {
    hipLaunchKernelGGL((query_hash_kernel<nd>), grid(a.wshift), block, 0, s, a, g, look);
  });
  SPX_LAUNCH_CHECK();
  spx::count(kQueryHash);
  return 0;
}

int spx_group_fwd(const void *vfeat, int n, const int32_t *rows, int n_cap, int nsample, int C, int dtype, void *out,
                  spx_stream_t stream) {
  using namespace spx;
  const int eb = check_group(n_cap, nsample, n, C, dtype);
  if (eb < 0) return eb;
  if (n_cap == 0) return 0;
  SPX_CHECK(rows && out && (n == 0 || vfeat), "vfeat / rows / out is NULL");
  SPX_CHECK(aligned_to(vfeat, eb) && aligned_to(out, eb) && aligned_to(rows, 4), "pointer not aligned to its elements");
  const unsigned char zeros[16] = {};             // (the gather of pointvoxel.hip: the bits moved, zeros for a row of -1)
  if (int rc = gather_rows(vfeat, n, rows, static_cast<long long>(n_cap) * nsample, C, eb, zeros, out,
                           static_cast<hipStream_t>(stream)))
    return rc;
  spx::count(kQueryGroupFwd);
  return 0;
}

int spx_group_bwd(const void *dout, int n_cap, int nsample, const int32_t *offsets, const int32_t *list, int n,
                  const int32_t *n_live, int C, int dtype, void *dvfeat, spx_stream_t stream) {
  using namespace spx;
  const int eb = check_group(n_cap, nsample, n, C, dtype);
  if (eb < 0) return eb;
  if (n == 0) return 0;
  SPX_CHECK(offsets && dvfeat && (n_cap == 0 || (dout && list)), "dout / offsets / list / dvfeat is NULL");
  SPX_CHECK(aligned_to(dout, eb) && aligned_to(dvfeat, eb), "pointer not aligned to its elements");
  const bool vec = (static_cast<long long>(C) * eb) % 16 == 0 && aligned_to(dout, 16) && aligned_to(dvfeat, 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_row(dtype, vec, [&](auto dt, auto v) {
    const int pieces = C / v, gshift = group_shift(pieces);
    hipLaunchKernelGGL((group_bwd_kernel<dt, v>), dim3(stream_blocks(static_cast<long long>(n) << gshift, kBlock)),
                       dim3(kBlock), 0, s, dout, n_cap * nsample, offsets, list, n, pieces, gshift, n_live, dvfeat);
  });
  SPX_LAUNCH_CHECK();
  spx::count(kQueryGroupBwd);
  return 0;
}

}  // extern "C"
