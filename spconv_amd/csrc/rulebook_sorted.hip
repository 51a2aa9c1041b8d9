// Sorted-order convolution rulebooks: spx_conv_rulebook_*_sorted and spx_rankmap_from_sorted -- outputs numbered by
// key rank over a level's rank map (rankmap.h).  Shared with the other builders: rulebook.h.
#include "rulebook.h"
#include "rankmap.h"

namespace spx {
namespace {

// ------------------------------------------ regular conv, fourth generation: outputs numbered by KEY RANK
// The passes above number the outputs in the CPU reference's first-seen order (indices.py:1742-1771), which takes a
// hash table, a first-seen bit map and a rank per (offset, input).  The reference's GPU path has no such order: its
// outputs come out of a sort + unique of the linear coordinate keys (all.py:1533-1552) or out of a hash table in slot
// order (indices.py:1380-1425).  This generation produces the SORTED order, without a sort and without a hash table:
//   * the RANK MAP of a level: one {occupancy bits, prefix} pair per 32 consecutive linear keys (batch-major, x
//     fastest), and behind the words the occupied cells before each block of 2048 words.
//     mark: one plain BYTE store per candidate into a byte-per-cell scratch map (idempotent: no atomics);
//     prefix: bytes -> bits, popcount scan of the words inside a block; scan_kernel: the blocks' offsets;
//     row of key = block offset + prefix + popcount(bits below): ONE 8-byte load, no probing, no first-seen resolution;
//   * pairs: per input, the rank of every candidate's key -> both pair tables, the input-side mask, list counts, and
//     the coordinates of the outputs it reaches (every input of an output stores the same values);
//   * the map stays with the level: a SubM layer behind the strided layer looks its neighbours up in it
//     (subm_rank_rows_kernel / subm_rank_probe_kernel below) -- no table fill, no insert, no slot walks -- and its
//     rows, being in key order, put x-neighbours in adjacent rows (what the gather-GEMMs of the level gain:
//     tools/order_probe.py).
// Memory: the map (batch x grid cells) / 4 bytes (47 M cells of a 21 x 800 x 704 x 4 level: 11.8 MB) + one byte per
// cell of scratch during the build; key spaces beyond 2^31 cells keep the hash builder.
// (kRankWords, conv4_prefix_kernel, rank_of and the size helpers of the map: rankmap.h)

template <int MJ>
__global__ void __launch_bounds__(kBlock)
conv4_mark_kernel(const int32_t *__restrict__ indices, int n, Geom g, uint8_t *__restrict__ occupied) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int b, c[4];
  read_row(indices, i, g.ndim, b, c);
  CandIter it;
  it.init(g, c, b >= 0 && b < g.batch);
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    if (!it.live) break;
    int q[4];
    it.offset(g, c, q);
    // one BYTE per cell, plain stores: idempotent (every writer stores 1), nothing to wait for, no atomic -- a bit map
    // costs an agent-scope atomicOr per candidate (20-25 G/s device-wide against ~80 G/s for stores: 58 -> 20 us at
    // 400 k inputs); conv4_prefix_kernel packs the bytes into the words of the rank map
    occupied[static_cast<unsigned long long>(layout_key(b, q, g.out_dims))] = 1;
    it.next();
  }
}

// The rank map of a level whose rows ALREADY are in ascending, unique key order (level 1 of a backbone when the data
// loader sorts its voxels: spconv_amd.pytorch.utils.sort_voxels_by_coordinate): row = rank, so the word of a key holds
// {bits of the level's rows that fall into it, index of the first of them} and every block offset is zero -- no marks,
// no prefix pass, no scan, no atomics.  The first row of a word writes it (it looks ahead over the <= 31 rows that can
// share the word).  Rows that break the contract (a key <= its predecessor's, a live row behind a dead one) raise
// `violation`; dead rows (batch -1: static shapes) must trail.
__global__ void __launch_bounds__(kBlock)
rankmap_from_sorted_kernel(const int32_t *__restrict__ indices, int n, Geom g, uint2 *__restrict__ cells,
                           int32_t *__restrict__ violation) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  auto key_of = [&](int row, bool &ok) __attribute__((always_inline)) {
    int b, c[4];
    read_row(indices, row, g.ndim, b, c);
    ok = b >= 0 && b < g.batch && in_range(c, g.in_dims);
    return ok ? static_cast<unsigned long long>(layout_key(b, c, g.in_dims)) : 0ull;
  };
  bool ok;
  const unsigned long long key = key_of(i, ok);
  if (!ok) return;
  bool first = true;
  if (i > 0) {
    bool pok;
    const unsigned long long prev = key_of(i - 1, pok);
    if (!pok || prev >= key) {
      if (violation) atomicOr(violation, 1);
    }
    first = !pok || (prev >> 5) != (key >> 5);
  }
  if (!first) return;
  uint32_t bits = 1u << (key & 31);
  for (int j = i + 1; j < n && j < i + 32; ++j) {
    bool jok;
    const unsigned long long kj = key_of(j, jok);
    if (!jok || (kj >> 5) != (key >> 5)) break;
    bits |= 1u << (kj & 31);
  }
  cells[key >> 5] = make_uint2(bits, static_cast<uint32_t>(i));
}

// both tables, the input-side mask and the pair counts of the Native lists (as conv3_pairs_kernel; the output row
// of a candidate is its key's rank)
template <int MJ>
__global__ void __launch_bounds__(kBlock)
conv4_pairs_kernel(const int32_t *__restrict__ indices, int n, Geom g, const uint2 *__restrict__ cells,
                   const int32_t *__restrict__ blockoff, int n_out, int32_t *__restrict__ out_indices,
                   int32_t *__restrict__ pair_fwd, int32_t *__restrict__ pair_bwd,
                   uint32_t *__restrict__ mask_bwd, int words, int32_t *__restrict__ groupcount,
                   int32_t *__restrict__ live_out) {
  __shared__ int lds_cnt[kMaxKv3];
  const int i = blockIdx.x * kBlock + threadIdx.x, kv = g.kv;
  // static-shape form: the number of live output rows (outputs found, at most the bound) for the layers behind
  if (live_out && i == 0) live_out[2] = live_out[0] < n_out ? live_out[0] : n_out;
  if (groupcount) {
    if (threadIdx.x < kMaxKv3) lds_cnt[threadIdx.x] = 0;
    __syncthreads();
  }
  int kk[MJ], oid[MJ];
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    kk[j] = -1;
    oid[j] = -1;
  }
  if (i < n) {
    int b, c[4];
    read_row(indices, i, g.ndim, b, c);
    CandIter it;
    it.init(g, c, b >= 0 && b < g.batch);
    unsigned long long key[MJ];
    int qx[MJ][4];
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      key[j] = 0;
      if (it.live) {
        kk[j] = it.offset(g, c, qx[j]);
        key[j] = static_cast<unsigned long long>(layout_key(b, qx[j], g.out_dims));
        it.next();
      }
    }
#pragma unroll
    for (int j = 0; j < MJ; ++j) {                 // (every map load of the row in flight together)
      if (kk[j] >= 0) {
        const int r = rank_of(cells, blockoff, key[j]);
        oid[j] = r < n_out ? r : -1;               // an output beyond the caller's bound
      }
    }
    const int lead = 4 - g.ndim;
#pragma unroll
    for (int j = 0; j < MJ; ++j)
      if (oid[j] >= 0) {
        pair_fwd[static_cast<size_t>(kk[j]) * n_out + oid[j]] = i;
        // the output's coordinates, by every input that reaches it (the same values: idempotent stores instead of a
        // pass over the whole map that decodes the set bits)
        int32_t *dst = out_indices + static_cast<size_t>(oid[j]) * (g.ndim + 1);
        dst[0] = b;
        for (int d = lead; d < 4; ++d) dst[1 + d - lead] = qx[j][d];
      }
  }
  uint32_t mword = 0;
  for (int k = 0; k < kv; ++k) {
    int val = -1;
#pragma unroll
    for (int j = 0; j < MJ; ++j) val = kk[j] == k ? oid[j] : val;
    if (i < n) pair_bwd[static_cast<size_t>(k) * n + i] = val;
    if (val >= 0) mword |= 1u << (k & 31);
    if (mask_bwd && i < n && ((k & 31) == 31 || k == kv - 1)) {
      mask_bwd[static_cast<size_t>(i) * words + (k >> 5)] = mword;
      mword = 0;
    }
    if (groupcount) {
      const unsigned long long bal = __ballot(val >= 0);
      if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&lds_cnt[k], __popcll(bal));
    }
  }
  if (groupcount) {
    __syncthreads();
    if (threadIdx.x < kv) groupcount[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x] = lds_cnt[threadIdx.x];
  }
}

// The rank map is the caller's buffer -- it outlives the call, the SubM layers of the level read it.
struct Conv4Ws {
  Geom g;                              // (conv4_begin: the problem in canonical form, its candidates per input)
  int mj;
  size_t W;                            // words of the level's rank map
  int32_t *blockcount, *d_nout, *groupcount;
  uint8_t *occupied;                   // one byte per cell (32 per word of the rank map), alive between mark and prefix
  int nblk;
  size_t bytes;
};
Conv4Ws carve_conv4_ws(void *ws, int n_in, int kv, size_t W) {
  Conv4Ws w;
  w.W = W;
  w.nblk = static_cast<int>((W + kRankWords - 1) / kRankWords);
  Carver cv(ws);
  w.occupied = cv.take<uint8_t>((W > 0 ? W : 1) * 32);
  w.blockcount = cv.take<int32_t>(w.nblk > 0 ? w.nblk : 1);
  w.d_nout = cv.take<int32_t>(2);
  w.groupcount = cv.take<int32_t>(static_cast<size_t>(kv) * div_up(n_in > 0 ? n_in : 1, kBlock));
  w.bytes = cv.off;
  return w;
}

struct SortedBufs {                    // the caller's two buffers of a sorted-order build
  void *rankmap;
  size_t rankmap_bytes;
  void *ws;
  size_t ws_bytes;
};

// What both passes start with: the problem's checks, its candidate count, the words of its rank map and its workspace.
int conv4_begin(const ConvProblem &p, const SortedBufs &b, Conv4Ws &w) {
  Geom g;
  if (conv_geom(p, g)) return -1;
  const int mj = conv3_cands(p);
  SPX_CHECK(mj > 0, "sorted-order build: this geometry takes the first-seen builder (spx_conv_sorted_ok)");
  const size_t W = rank_words(p.ndim, p.batch_size, p.out_shape);
  SPX_CHECK(W > 0 && b.rankmap && b.rankmap_bytes >= rank_bytes(W), "rank map missing or too small (%zu words)", W);
  w = carve_conv4_ws(b.ws, p.n_in, g.kv, W);
  w.g = g;
  w.mj = mj;
  SPX_CHECK(b.ws && b.ws_bytes >= w.bytes, "workspace too small");
  return 0;
}

// more / nout_dev: as conv_count_impl of the first-seen builder (the static-shape form's fills and counter)
int conv4_count_impl(const ConvProblem &p, const SortedBufs &b, int *n_out_h, hipStream_t s,
                     const FillList *more = nullptr, int32_t *nout_dev = nullptr) {
  Conv4Ws w;
  if (conv4_begin(p, b, w)) return -1;
  const size_t W = w.W;
  if (n_out_h) *n_out_h = 0;
  uint2 *cells = static_cast<uint2 *>(b.rankmap);
  if (nout_dev) w.d_nout = nout_dev;
  {
    FillList fills;
    fills.add(w.occupied, W * 32, 0u);
    fills.add(w.d_nout, 2 * sizeof(int32_t), 0u);
    if (more) fills.add(*more);
    SPX_HIP(fills.launch(s));
  }
  if (p.n_in > 0) {
    SPX_CONV3_LAUNCH(conv4_mark_kernel, w.mj, dim3(div_up(p.n_in, kBlock)), dim3(kBlock), 0, s, p.indices, p.n_in, w.g,
                     w.occupied);
    hipLaunchKernelGGL(conv4_prefix_kernel, dim3(w.nblk), dim3(kBlock), 0, s,
                       reinterpret_cast<const uint4 *>(w.occupied), cells, static_cast<unsigned>(W), w.blockcount);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kBlock), 0, s, w.blockcount, rank_blockoff(b.rankmap, W), w.nblk,
                       w.d_nout);
    SPX_LAUNCH_CHECK();
  }
  return n_out_h ? read_count(w.d_nout, s, n_out_h) : 0;   // (static-shape form: the count stays on the device)
}

int conv4_fill_impl(const ConvProblem &p, const ConvOutputs &o, const SortedBufs &b, hipStream_t s, bool prefilled,
                    int32_t *nout_dev = nullptr) {
  Conv4Ws w;
  if (conv4_begin(p, b, w)) return -1;
  SPX_CHECK(o.pair_fwd && o.pair_bwd && o.out_indices, "out_indices, pair_fwd and pair_bwd are required");
  const int n_in = p.n_in, n_out = o.n_out, kv = w.g.kv, words = div_up(kv, 32);
  const int ngroups = div_up(n_in > 0 ? n_in : 1, kBlock);
  const bool lists = o.pair_native || o.num_per_loc;
  SPX_CHECK(!lists || (ngroups <= 16384 && kv <= 128), "Native lists of a sorted-order build: too many rows / offsets");
  SPX_CHECK(!o.pair_native || o.num_per_loc, "num_per_loc is required with pair_native");
  {
    FillList fills;
    if (n_in > 0 && n_out > 0 && !prefilled)
      fills.add(o.pair_fwd, sizeof(int32_t) * static_cast<size_t>(kv) * n_out, 0xFFFFFFFFu);
    if (n_in == 0 && o.num_per_loc) fills.add(o.num_per_loc, sizeof(int32_t) * kv, 0u);
    SPX_HIP(fills.launch(s));
  }
  if (n_in == 0) return 0;
  SPX_CONV3_LAUNCH(conv4_pairs_kernel, w.mj, dim3(div_up(n_in, kBlock)), dim3(kBlock), 0, s, p.indices, n_in, w.g,
                   static_cast<const uint2 *>(b.rankmap), static_cast<const int32_t *>(rank_blockoff(b.rankmap, w.W)),
                   n_out, o.out_indices, o.pair_fwd, o.pair_bwd, o.mask_bwd, words, lists ? w.groupcount : nullptr,
                   nout_dev);
  if (o.mask_fwd && n_out > 0)
    hipLaunchKernelGGL(mask_from_tables_kernel, dim3(div_up(n_out, kBlock)), dim3(kBlock), 0, s, o.pair_fwd, n_out,
                       o.mask_fwd, o.pair_bwd, 0, o.mask_bwd, kv, words);
  if (lists)
    hipLaunchKernelGGL(subm_lists_kernel, dim3(div_up(n_in, kItems), kv), dim3(kBlock), 0, s, o.pair_bwd, kv, n_in,
                       ngroups, w.groupcount, o.pair_native, o.num_per_loc, 0, 1);
  SPX_LAUNCH_CHECK();
  return 0;
}
}  // namespace
}  // namespace spx

using namespace spx;

extern "C" {

size_t spx_rankmap_bytes(int ndim, int batch_size, const int *shape) {
  return rank_bytes(rank_words(ndim, batch_size, shape));
}

int spx_conv_sorted_ok(int ndim, int batch_size, const int *in_shape, const int *out_shape, const int *ksize,
                       const int *stride, const int *padding, const int *dilation, int transposed) {
  if (ndim < 1 || ndim > kMaxNdim || transposed) return 0;
  return conv3_cands({nullptr, 0, ndim, batch_size, in_shape, out_shape, ksize, stride, padding, dilation, 0}) > 0 &&
         rank_words(ndim, batch_size, out_shape) > 0;
}

size_t spx_conv_rulebook_sorted_ws_bytes(int n_in, int ndim, int batch_size, const int *out_shape, const int *ksize) {
  if (ndim < 1 || ndim > kMaxNdim) return 0;
  int kv = 1;
  for (int i = 0; i < ndim; ++i) kv *= ksize[i];
  return carve_conv4_ws(nullptr, n_in, kv, rank_words(ndim, batch_size, out_shape)).bytes + 256;
}

int spx_conv_rulebook_count_sorted(const int32_t *indices, int n_in, int ndim, int batch_size, const int *in_shape,
                                   const int *out_shape, const int *ksize, const int *stride, const int *padding,
                                   const int *dilation, void *rankmap, size_t rankmap_bytes, void *ws,
                                   size_t ws_bytes, int *n_out_h, spx_stream_t stream) {
  SPX_CHECK(n_out_h, "n_out_h is required");
  const ConvProblem p{indices, n_in, ndim, batch_size, in_shape, out_shape, ksize, stride, padding, dilation, 0};
  return conv4_count_impl(p, {rankmap, rankmap_bytes, ws, ws_bytes}, n_out_h, static_cast<hipStream_t>(stream));
}

int spx_conv_rulebook_fill_sorted(const int32_t *indices, int n_in, int ndim, int batch_size, const int *in_shape,
                                  const int *out_shape, const int *ksize, const int *stride, const int *padding,
                                  const int *dilation, int n_out, int32_t *out_indices, int32_t *pair_fwd,
                                  int32_t *pair_bwd, uint32_t *mask_fwd, uint32_t *mask_bwd, int32_t *pair_native,
                                  int32_t *num_per_loc, void *rankmap, size_t rankmap_bytes, void *ws,
                                  size_t ws_bytes, spx_stream_t stream) {
  const ConvProblem p{indices, n_in, ndim, batch_size, in_shape, out_shape, ksize, stride, padding, dilation, 0};
  const ConvOutputs o{n_out, out_indices, pair_fwd, pair_bwd, mask_fwd, mask_bwd, pair_native, num_per_loc};
  return conv4_fill_impl(p, o, {rankmap, rankmap_bytes, ws, ws_bytes}, static_cast<hipStream_t>(stream), false);
}

int spx_conv_rulebook_static_sorted(const int32_t *indices, int n_in, int ndim, int batch_size, const int *in_shape,
                                    const int *out_shape, const int *ksize, const int *stride, const int *padding,
                                    const int *dilation, int n_out_cap, int32_t *out_indices, int32_t *pair_fwd,
                                    int32_t *pair_bwd, uint32_t *mask_fwd, uint32_t *mask_bwd, int32_t *pair_native,
                                    int32_t *num_per_loc, int32_t *n_out_dev, void *rankmap, size_t rankmap_bytes,
                                    void *ws, size_t ws_bytes, spx_stream_t stream) {
  const ConvProblem p{indices, n_in, ndim, batch_size, in_shape, out_shape, ksize, stride, padding, dilation, 0};
  const ConvOutputs o{n_out_cap, out_indices, pair_fwd, pair_bwd, mask_fwd, mask_bwd, pair_native, num_per_loc};
  const SortedBufs b{rankmap, rankmap_bytes, ws, ws_bytes};
  hipStream_t s = static_cast<hipStream_t>(stream);
  FillList pre;         // (as spx_conv_rulebook_static: the -1 fills of the outputs ride in the first fill launch)
  if (static_prologue(p, o, n_out_dev, pre)) return -1;
  const int rc = conv4_count_impl(p, b, nullptr, s, &pre, n_out_dev);
  return rc ? rc : conv4_fill_impl(p, o, b, s, true, n_out_dev);
}

int spx_rankmap_from_sorted(const int32_t *indices, int n, int ndim, int batch_size, const int *spatial_shape,
                            void *rankmap, size_t rankmap_bytes, int32_t *violation, spx_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  const size_t W = rank_words(ndim, batch_size, spatial_shape);
  SPX_CHECK(W > 0 && rankmap && rankmap_bytes >= rank_bytes(W), "rank map missing or too small (%zu words)", W);
  SPX_CHECK(n >= 0 && (indices || n == 0), "indices required");
  const int one[4] = {1, 1, 1, 1}, zero[4] = {0, 0, 0, 0};
  const Geom g = make_geom(ndim, batch_size, spatial_shape, spatial_shape, one, one, zero, one);
  {
    FillList fills;                    // every word empty, every block offset zero (row = rank: the prefixes are global)
    fills.add(rankmap, rank_bytes(W), 0u);
    if (violation) fills.add(violation, sizeof(int32_t), 0u);
    SPX_HIP(fills.launch(s));
  }
  if (n > 0)
    hipLaunchKernelGGL(rankmap_from_sorted_kernel, dim3(div_up(n, kBlock)), dim3(kBlock), 0, s, indices, n, g,
                       static_cast<uint2 *>(rankmap), violation);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
