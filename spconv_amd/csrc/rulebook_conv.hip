// First-seen convolution rulebooks: spx_conv_rulebook_count / _fill / _static, regular and transposed convolution,
// outputs numbered in the reference's first-seen order.  Thread-per-(offset, input) passes (conv_*), the compact-candidate
// passes of strided convolutions (conv3_*) and the ratio cache that sizes their table.  Shared: rulebook.h.
#include "rulebook.h"

#include <mutex>

namespace spx {
namespace {

// ------------------------------------------------ regular / transposed conv

// Output coordinate for (input row, offset k); false if the pair does not exist.
// Regular: query_npq (indices.py:174-203), transposed: query_nhw_out (:249-269).
__device__ __forceinline__ bool conv_out_coord(const Geom &g, const int (&c)[4],
                                               const int (&r)[4], int transposed,
                                               int (&q)[4]) {
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if (transposed) {
      q[d] = c[d] * g.stride[d] - g.padding[d] + r[d] * g.dilation[d];
    } else {
      const int h = c[d] + g.padding[d] - r[d] * g.dilation[d];
      q[d] = h / g.stride[d];  // C++ truncation, like the reference
      ok = ok && (h % g.stride[d]) == 0;
    }
    ok = ok && q[d] >= 0 && q[d] < g.out_dims[d];
  }
  return ok;
}

// stage 1: hash every candidate output key with value = min first-seen position
// (k * n + i); remember the slot so later passes do not re-probe.
__global__ void __launch_bounds__(kBlock)
conv_stage1_kernel(const int32_t *__restrict__ indices, int n, Geom g, int transposed,
                   Table t, int32_t *__restrict__ slot_of, int32_t *__restrict__ overflow) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const int k = blockIdx.y;
  if (i >= n) return;
  int b, c[4], r[4], q[4];
  read_row(indices, i, g.ndim, b, c);
  decode_offset(k, g.ksize, r);
  const size_t pos = static_cast<size_t>(k) * n + i;
  int slot = -1;
  if (b >= 0 && b < g.batch && conv_out_coord(g, c, r, transposed, q)) {
    slot = table_insert_min<true>(t, layout_key(b, q, g.out_dims), static_cast<int32_t>(pos));
    if (slot < 0) *overflow = 1;          // table full: reported by spx_conv_rulebook_count
  }
  slot_of[pos] = slot;
}

__device__ __forceinline__ bool is_first_seen(const int32_t *slot_of, const Table &t,
                                              size_t pos, bool inb, int &slot) {
  slot = inb ? slot_of[pos] : -1;
  return slot >= 0 && table_val(t, slot) == static_cast<int32_t>(pos);
}

__global__ void __launch_bounds__(kBlock)
conv_count_first_kernel(const int32_t *__restrict__ slot_of, Table t,
                        int n, int nblk, int32_t *__restrict__ blockcount) {
  __shared__ int lds_wave[kBlock / 64];
  const int k = blockIdx.y, blk = blockIdx.x;
  const int begin = blk * kItems;
  int cnt = 0;
#pragma unroll
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    int slot;
    const bool pred = is_first_seen(slot_of, t, static_cast<size_t>(k) * n + e, e < n, slot);
    cnt += __popcll(__ballot(pred));
  }
  if ((threadIdx.x & 63) == 0) lds_wave[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kBlock / 64; ++w) s += lds_wave[w];
    blockcount[static_cast<size_t>(k) * nblk + blk] = s;
  }
}

// Numbers outputs in first-seen order and writes their coordinates.
__global__ void __launch_bounds__(kBlock)
conv_assign_kernel(const int32_t *__restrict__ indices, int n, Geom g, int transposed,
                   const int32_t *__restrict__ slot_of, Table t,
                   int nblk, const int32_t *__restrict__ blockoff,
                   int32_t *__restrict__ slot_out, int32_t *__restrict__ out_indices, int n_cap) {
  __shared__ int lds_wave[kBlock / 64];
  const int k = blockIdx.y, blk = blockIdx.x;
  const int begin = blk * kItems;
  int running = blockoff[static_cast<size_t>(k) * nblk + blk];
  int r[4];
  decode_offset(k, g.ksize, r);
  const int lead = 4 - g.ndim;
  // all of the block's loads first (8 independent slot -> table chains in flight): with the loads
  // inside the ranking loop every iteration paid two dependent memory latencies between barriers
  int slots[kItems / kBlock];
  bool firsts[kItems / kBlock];
#pragma unroll
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    slots[it] = e < n ? slot_of[static_cast<size_t>(k) * n + e] : -1;
  }
#pragma unroll
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    firsts[it] = slots[it] >= 0 &&
                 table_val(t, slots[it]) == static_cast<int32_t>(static_cast<size_t>(k) * n + e);
  }
#pragma unroll
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    const int slot = slots[it];
    const bool first = firsts[it];
    int total;
    const int rank = block_rank(first, total, lds_wave);
    if (first) {
      // outputs beyond the caller's bound (num_out_act_bound, ops.py:263-266) are dropped: no
      // coordinates, no pairs
      const int oid = running + rank;
      slot_out[slot] = oid < n_cap ? oid : -1;
      if (oid < n_cap) {
        int b, c[4], q[4];
        read_row(indices, e, g.ndim, b, c);
        conv_out_coord(g, c, r, transposed, q);
        int32_t *dst = out_indices + static_cast<size_t>(oid) * (g.ndim + 1);
        dst[0] = b;
        for (int d = lead; d < 4; ++d) dst[1 + d - lead] = q[d];
      }
    }
    running += total;
  }
}

__global__ void __launch_bounds__(kBlock)
conv_stage2_kernel(const int32_t *__restrict__ slot_of, const int32_t *__restrict__ slot_out,
                   int n, int n_out, int32_t *__restrict__ pair_fwd,
                   int32_t *__restrict__ pair_bwd, int32_t *__restrict__ groupcount = nullptr) {
  // groupcount[k][block]: pairs of offset k among this block's 256 input rows = the entries of
  // ConvAlgo.Native list k that fall into the group (subm_lists_kernel turns them into offsets)
  __shared__ int lds_wave[kBlock / 64];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const int k = blockIdx.y;
  int oid = -1;
  if (i < n) {
    const size_t pos = static_cast<size_t>(k) * n + i;
    const int slot = slot_of[pos];
    if (slot >= 0) {
      oid = slot_out[slot];                          // -1: an output beyond the caller's bound
      // rows that repeat a coordinate reach the same output through the same offset: the FIRST of them owns the
      // entry (as in the SubM tables and the CPU lists' first entry), whatever order the workgroups run in --
      // the table starts as 0xFFFFFFFF, an unsigned minimum
      if (oid >= 0)
        atomicMin(reinterpret_cast<unsigned int *>(&pair_fwd[static_cast<size_t>(k) * n_out + oid]),
                  static_cast<unsigned int>(i));
    }
    pair_bwd[pos] = oid;
  }
  if (groupcount) {
    const unsigned long long bal = __ballot(oid >= 0);
    if ((threadIdx.x & 63) == 0) lds_wave[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
      int sum = 0;
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) sum += lds_wave[w];
      groupcount[static_cast<size_t>(k) * gridDim.x + blockIdx.x] = sum;
    }
  }
}


// ------------------------------------------ regular conv, third generation: compact candidates
// A strided convolution pairs an input with FEW of the kv offsets: along one axis only the r with
// (c + p - r d) % s == 0 reach an output, at most ceil(k gcd(d, s) / s) of them (conv_max_out), so
// k = 3 / s = 2 in 3-d has <= 8 candidates per input out of 27 (3.4 on average), k = 2 / s = 2 exactly
// one.  The second-generation passes above launch a thread per (offset, input) and stream kv x N
// arrays five times; 85 % of those threads divide, find no pair and write a -1.  Here one thread owns
// an input row: it derives the valid offsets of each axis as a bit set (no integer division: h / s by
// a float multiply, exact below 2^21), walks their product in ascending k -- the candidate index j --
// and every per-candidate array is [MJ, N] with MJ <= 8.  The first-seen numbering (k-major, then
// input-major, indices.py:1742-1771) comes from a BIT MAP of the first-seen candidates, one row per
// offset: the count of an (offset, 2048-input block) is a popcount, the rank of an entry a prefix
// popcount -- in input order by construction, no ballots, no barriers, every pass elementwise.
// (CandIter, kMaxCand, kMaxKv3: rulebook.h)

// pass 1: insert every candidate output key with value = min first-seen position (k * n + i);
// slot_c[j][i] = its slot (entries past an input's candidate count are never read)
template <int MJ>
__global__ void __launch_bounds__(kBlock)
conv3_insert_kernel(const int32_t *__restrict__ indices, int n, Geom g, Table t,
                    int32_t *__restrict__ slot_c, int32_t *__restrict__ overflow) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int b, c[4];
  read_row(indices, i, g.ndim, b, c);
  CandIter it;
  it.init(g, c, b >= 0 && b < g.batch);
  // blockIdx.y: the thread's share of the row's candidates (j = y mod gridDim.y) -- a small scene
  // does not have enough rows to hide eight dependent atomic round trips per thread
  const int share = blockIdx.y, shares = gridDim.y - 1;
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    if (!it.live) break;
    if ((j & shares) == share) {
      int q[4];
      const int k = it.offset(g, c, q);
      const int slot = table_insert_min<true>(t, layout_key(b, q, g.out_dims), k * n + i);
      if (slot < 0) *overflow = 1;             // table full: reported by spx_conv_rulebook_count
      slot_c[static_cast<size_t>(j) * n + i] = slot;
    }
    it.next();
  }
}

// pass 2: bit map of the first-seen candidates, one row of nblk * 64 words per offset (bit i of row k:
// input i is the first to reach its output through k).  A workgroup collects the bits of its 256 rows
// in LDS -- 32 neighbouring inputs share a word, global atomics on it would serialise inside the wave --
// and ORs its non-zero words (8 per offset) into the map; also the per-input byte of first-seen
// candidate indices that lets pass 3 skip everything else
template <int MJ>
__global__ void __launch_bounds__(kBlock)
conv3_first_kernel(const int32_t *__restrict__ indices, int n, Geom g, Table t,
                   const int32_t *__restrict__ slot_c, int nblk, uint32_t *__restrict__ firstbits,
                   uint8_t *__restrict__ firstflags) {
  __shared__ uint32_t bm[kMaxKv3][kBlock / 32];
  const int i = blockIdx.x * kBlock + threadIdx.x, kv = g.kv;
  for (int w = threadIdx.x; w < kv * (kBlock / 32); w += kBlock) (&bm[0][0])[w] = 0;
  __syncthreads();
  const int share = blockIdx.y, shares = gridDim.y - 1;      // (as conv3_insert_kernel)
  if (i < n) {
    int b, c[4];
    read_row(indices, i, g.ndim, b, c);
    CandIter it;
    it.init(g, c, b >= 0 && b < g.batch);
    int kk[MJ], slot[MJ];
#pragma unroll
    for (int j = 0; j < MJ; ++j) {             // every load of the row first
      kk[j] = -1;
      slot[j] = -1;
      if (it.live) {
        if ((j & shares) == share) {
          kk[j] = it.offset(g);
          slot[j] = slot_c[static_cast<size_t>(j) * n + i];
        }
        it.next();
      }
    }
    int val[MJ];
#pragma unroll
    for (int j = 0; j < MJ; ++j) val[j] = slot[j] >= 0 ? table_val(t, slot[j]) : -1;
    uint32_t flags = 0;
#pragma unroll
    for (int j = 0; j < MJ; ++j)
      if (slot[j] >= 0 && val[j] == kk[j] * n + i) {
        atomicOr(&bm[kk[j]][threadIdx.x >> 5], 1u << (threadIdx.x & 31));
        flags |= 1u << j;
      }
    firstflags[static_cast<size_t>(share) * n + i] = static_cast<uint8_t>(flags);   // one plane per share
  }
  __syncthreads();
  const size_t rowwords = static_cast<size_t>(nblk) * (kItems / 32);
  for (int w = threadIdx.x; w < kv * (kBlock / 32); w += kBlock) {
    const uint32_t word = (&bm[0][0])[w];
    if (word) {
      uint32_t *dst = &firstbits[(w / (kBlock / 32)) * rowwords + blockIdx.x * (kBlock / 32) + (w % (kBlock / 32))];
      if (shares) atomicOr(dst, word); else *dst = word;       // one share: this workgroup owns the word
    }
  }
}

// pass 2b: one wave per (offset, 2048-input block): popcount of the block's 64 bit-map words
// (-> blockcount, for the scan) and their exclusive prefix inside the block (-> wordpre)
__global__ void __launch_bounds__(kBlock)
conv3_count_kernel(const uint32_t *__restrict__ firstbits, int rows, int32_t *__restrict__ wordpre,
                   int32_t *__restrict__ blockcount) {
  const int row = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const size_t at = static_cast<size_t>(row) * (kItems / 32) + lane;
  const int cnt = __popc(firstbits[at]);
  int incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(incl, d, 64);
    if (lane >= d) incl += u;
  }
  wordpre[at] = incl - cnt;
  if (lane == 63) blockcount[row] = incl;
}

// pass 3: number the first-seen candidates -- blockoff of (offset, block) + first-seen entries of the
// block before this word + set bits below this input's -- and write their coordinates;
// slot_out[slot] = output row (or -1 beyond the caller's bound)
template <int MJ>
__global__ void __launch_bounds__(kBlock)
conv3_assign_kernel(const int32_t *__restrict__ indices, int n, Geom g,
                    const int32_t *__restrict__ slot_c, int nblk,
                    const uint32_t *__restrict__ firstbits, const uint8_t *__restrict__ firstflags,
                    const int32_t *__restrict__ wordpre, const int32_t *__restrict__ blockoff,
                    int32_t *__restrict__ slot_out, int32_t *__restrict__ out_indices, int n_cap) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t flags = firstflags[static_cast<size_t>(blockIdx.y) * n + i];     // (shares as in pass 2)
  if (!flags) return;                          // (most inputs are first for no offset)
  int b, c[4];
  read_row(indices, i, g.ndim, b, c);
  CandIter it;
  it.init(g, c, b >= 0 && b < g.batch);
  const int lead = 4 - g.ndim;
  const size_t rowwords = static_cast<size_t>(nblk) * (kItems / 32);
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    if (!it.live) break;
    if ((flags >> j) & 1u) {
      int q[4];
      const int k = it.offset(g, c, q);
      const size_t at = k * rowwords + (i >> 5);
      const int oid = blockoff[static_cast<size_t>(k) * nblk + i / kItems] + wordpre[at] +
                      __popc(firstbits[at] & ((1u << (i & 31)) - 1u));
      const int slot = slot_c[static_cast<size_t>(j) * n + i];
      // outputs beyond the caller's bound (num_out_act_bound, ops.py:263-266) are dropped
      slot_out[slot] = oid < n_cap ? oid : -1;
      if (oid < n_cap) {
        int32_t *dst = out_indices + static_cast<size_t>(oid) * (g.ndim + 1);
        dst[0] = b;
        for (int d = lead; d < 4; ++d) dst[1 + d - lead] = q[d];
      }
    }
    it.next();
  }
}

// pass 4: both tables, the input-side mask and the per-(offset, 256 rows) pair counts of the Native
// lists.  pair_bwd and mask_bwd are written whole (no -1 pre-fill, no second pass over pair_bwd).
template <int MJ>
__global__ void __launch_bounds__(kBlock)
conv3_pairs_kernel(const int32_t *__restrict__ indices, int n, Geom g,
                   const int32_t *__restrict__ slot_c, const int32_t *__restrict__ slot_out, int n_out,
                   int32_t *__restrict__ pair_fwd, int32_t *__restrict__ pair_bwd,
                   uint32_t *__restrict__ mask_bwd, int words, int32_t *__restrict__ groupcount) {
  __shared__ int lds_cnt[kMaxKv3];
  const int i = blockIdx.x * kBlock + threadIdx.x, kv = g.kv;
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
    int slot[MJ];
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      slot[j] = -1;
      if (it.live) {
        kk[j] = it.offset(g);
        slot[j] = slot_c[static_cast<size_t>(j) * n + i];
        it.next();
      }
    }
#pragma unroll
    for (int j = 0; j < MJ; ++j)
      if (slot[j] >= 0) oid[j] = slot_out[slot[j]];    // -1: an output beyond the caller's bound
#pragma unroll
    for (int j = 0; j < MJ; ++j)
      if (oid[j] >= 0)      // (smallest row wins among rows that repeat a coordinate, as conv_stage2_kernel)
        atomicMin(reinterpret_cast<unsigned int *>(&pair_fwd[static_cast<size_t>(kk[j]) * n_out + oid[j]]),
                  static_cast<unsigned int>(i));
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

struct ConvWs {
  Table t;
  int32_t *slot_out, *slot_of, *blockcount, *blockoff, *d_nout, *groupcount;
  uint32_t *firstbits;                 // compact passes: [kv, nblk, 64] first-seen bit map ...
  int32_t *wordpre;                    // ... first-seen entries of the block before each of its words
  uint8_t *firstflags;                 // ... and per input the candidate indices that are first-seen
  int nblk;
  size_t bytes;
};

// Launch counter (rulebook/conv3/<mj> | rulebook/conv_generic) of the passes conv3_cands picked.
Counter conv_pass_counter(int mj) {
  return mj == 0 ? kRbConvGeneric : (mj == 1 ? kRbConv3_1 : (mj == 2 ? kRbConv3_2 : (mj == 4 ? kRbConv3_4 : kRbConv3_8)));
}

// Launch counter (rulebook/conv3_shares/<s>) of the grid.y a compact pass is launched with.
Counter conv_shares_counter(int shares) {
  return shares <= 1 ? kRbShares1 : (shares == 2 ? kRbShares2 : (shares == 4 ? kRbShares4 : kRbShares8));
}

// (of the problem: n_in, ndim, ksize, stride, dilation and transposed only -- what the size query knows)
ConvWs carve_conv_ws(void *ws, const ConvProblem &p, bool packed = false) {
  const int rows = p.n_in > 0 ? p.n_in : 1;
  int kv = 1;
  for (int i = 0; i < p.ndim; ++i) kv *= p.ksize[i];
  uint32_t cap = table_capacity(conv_max_out(p.n_in, p.ndim, p.ksize, p.stride, p.dilation, p.transposed));
  // tests only (spx_set_option): a table smaller than the bound, to exercise the overflow report
  const int test_cap = option_int("SPX_TEST_CONV_TABLE_CAP", 0);
  if (test_cap > 0 && static_cast<uint32_t>(test_cap) < cap) cap = table_capacity(static_cast<size_t>(test_cap) / 2);
  ConvWs w;
  w.nblk = div_up(rows, kItems);
  Carver cv(ws);
  {
    hkey_t *keys = cv.take<hkey_t>(cap);
    table_place(w.t, keys, cv.take<int32_t>(cap), cap, packed);
  }
  w.slot_out = cv.take<int32_t>(cap);
  w.slot_of = cv.take<int32_t>(static_cast<size_t>(kv) * rows);
  w.blockcount = cv.take<int32_t>(static_cast<size_t>(kv) * w.nblk);
  w.blockoff = cv.take<int32_t>(static_cast<size_t>(kv) * w.nblk);
  w.d_nout = cv.take<int32_t>(2);      // [0] number of outputs, [1] hash-table overflow flag
  w.groupcount = cv.take<int32_t>(static_cast<size_t>(kv) * div_up(rows, kBlock));
  w.firstbits = cv.take<uint32_t>(static_cast<size_t>(kv <= kMaxKv3 ? kv : 0) * w.nblk * (kItems / 32));
  w.wordpre = cv.take<int32_t>(static_cast<size_t>(kv <= kMaxKv3 ? kv : 0) * w.nblk * (kItems / 32));
  w.firstflags = cv.take<uint8_t>(static_cast<size_t>(kMaxCand) * rows);
  w.bytes = cv.off;
  return w;
}
size_t conv_ws_bytes(const ConvProblem &p) { return carve_conv_ws(nullptr, p).bytes + 256; }

// Table sizing of the compact passes.  The guaranteed bound (conv_max_out: 8 N for k = 3 / s = 2) gives a table that is
// 4 % full on a LiDAR scene -- 67 MB of slots for 313 k outputs at 400 k inputs, every probe its own HBM line, 20 us of
// fill.  The builder therefore sizes the table for the outputs it EXPECTS and keeps the bound as the fallback:
//   * static-shape form: the caller's output bound (more distinct candidates than 2x that: the overflow flag the
//     caller reads back with the count)
//   * two-call form: the outputs-per-input ratio the same geometry produced last time (+25 %), kept in a small
//     direct-mapped cache -- the role of the reference's per-problem tuner cache (convops.py:1150,1283-1297); a table
//     that overflows is seen in the count's read-back and the pass is run again at the guaranteed size.  Results never
//     depend on the size.
struct RatioEntry {
  unsigned long long key;
  int ratio_x64;                     // ceil(64 * n_out / n_in) of the last build, 0 = none yet
};
RatioEntry g_ratio[64];
std::mutex g_ratio_mutex;

unsigned long long geometry_key(const ConvProblem &p) {
  unsigned long long h = 1469598103934665603ull ^ static_cast<unsigned>(p.ndim);
  for (int i = 0; i < p.ndim; ++i)
    for (const int v : {p.in_shape[i], p.ksize[i], p.stride[i], p.padding[i], p.dilation ? p.dilation[i] : 1}) {
      h ^= static_cast<unsigned>(v);
      h *= 1099511628211ull;
    }
  return h | 1ull;
}

size_t expected_outputs(unsigned long long key, int n_in) {
  std::lock_guard<std::mutex> lock(g_ratio_mutex);
  const RatioEntry &e = g_ratio[key % 64];
  if (e.key != key || e.ratio_x64 <= 0) return 0;                       // unknown: the bound
  return static_cast<size_t>(n_in) * e.ratio_x64 / 64 * 5 / 4 + 4096;
}

void remember_outputs(unsigned long long key, int n_in, int n_out) {
  std::lock_guard<std::mutex> lock(g_ratio_mutex);
  RatioEntry &e = g_ratio[key % 64];
  e.key = key;
  e.ratio_x64 = static_cast<int>((static_cast<long long>(n_out) * 64 + n_in - 1) / (n_in > 0 ? n_in : 1)) + 1;
}

// expect_out: distinct outputs to size the hash table for (0 = the guaranteed bound).  *overflow_h (with n_out_h): the
// table filled up -- the caller decides whether a larger table exists.  more: fills of the caller that ride in this
// pass's fill launch; nout_dev: where {count, overflow} go instead of the workspace (static-shape form: no copy after)
int conv_count_impl(const ConvProblem &p, void *ws, size_t ws_bytes, int *n_out_h, int *overflow_h,
                    size_t expect_out, hipStream_t s, const FillList *more = nullptr, int32_t *nout_dev = nullptr) {
  Geom g;
  if (conv_geom(p, g)) return -1;
  SPX_CHECK(ws_bytes >= conv_ws_bytes(p), "workspace too small");
  if (n_out_h) *n_out_h = 0;
  const int n_in = p.n_in;
  if (n_in == 0) return 0;
  ConvWs w = carve_conv_ws(ws, p, keys_fit_u32(g.batch, g.out_dims, 4));
  const int mj = conv3_cands(p);
  if (mj && expect_out > 0) {            // (the later passes of this form never touch the table)
    const uint32_t cap = table_capacity(expect_out);
    if (cap < w.t.mask + 1u) {
      count(kRbConvShrunk);
      table_shrink(w.t, cap);
    }
  }
  {
    FillList fills;                      // table and flags in one launch
    table_fill(fills, w.t);
    if (nout_dev) w.d_nout = nout_dev;
    fills.add(w.d_nout, 2 * sizeof(int32_t), 0u);
    if (more) fills.add(*more);
    if (mj) fills.add(w.firstbits, sizeof(uint32_t) * static_cast<size_t>(g.kv) * w.nblk * (kItems / 32), 0u);
    SPX_HIP(fills.launch(s));
  }
  count(conv_pass_counter(mj));
  if (mj) {
    const int shares = conv3_shares(n_in, mj);
    count(conv_shares_counter(shares));
    SPX_CONV3_LAUNCH(conv3_insert_kernel, mj, dim3(div_up(n_in, kBlock), shares), dim3(kBlock), 0, s, p.indices, n_in, g,
                     w.t, w.slot_of, w.d_nout + 1);
    SPX_CONV3_LAUNCH(conv3_first_kernel, mj, dim3(div_up(n_in, kBlock), shares), dim3(kBlock), 0, s, p.indices, n_in, g,
                     w.t, static_cast<const int32_t *>(w.slot_of), w.nblk, w.firstbits, w.firstflags);
    hipLaunchKernelGGL(conv3_count_kernel, dim3(div_up(g.kv * w.nblk, kBlock / 64)), dim3(kBlock), 0, s,
                       static_cast<const uint32_t *>(w.firstbits), g.kv * w.nblk, w.wordpre, w.blockcount);
  } else {
    hipLaunchKernelGGL(conv_stage1_kernel, dim3(div_up(n_in, kBlock), g.kv), dim3(kBlock), 0, s, p.indices, n_in, g,
                       p.transposed, w.t, w.slot_of, w.d_nout + 1);
    hipLaunchKernelGGL(conv_count_first_kernel, dim3(w.nblk, g.kv), dim3(kBlock), 0, s, w.slot_of, w.t, n_in, w.nblk,
                       w.blockcount);
  }
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kBlock), 0, s, w.blockcount, w.blockoff, g.kv * w.nblk, w.d_nout);
  SPX_LAUNCH_CHECK();
  return n_out_h ? read_count(w.d_nout, s, n_out_h, overflow_h) : 0;   // (static-shape form: the count stays there)
}

// prefilled: pair_fwd already holds -1 (the static-shape form puts that fill into the first launch)
int conv_fill_impl(const ConvProblem &p, const ConvOutputs &o, void *ws, size_t ws_bytes, hipStream_t s,
                   bool prefilled) {
  Geom g;
  if (conv_geom(p, g)) return -1;
  SPX_CHECK(ws_bytes >= conv_ws_bytes(p), "workspace too small");
  SPX_CHECK(o.pair_fwd && o.pair_bwd && o.out_indices, "out_indices, pair_fwd and pair_bwd are required");
  const int n_in = p.n_in, n_out = o.n_out, kv = g.kv, words = div_up(kv, 32);
  const int ngroups = div_up(n_in > 0 ? n_in : 1, kBlock);
  // second form: the Native lists come from subm_lists_kernel (conv mode) over the 256-row pair counts
  // stage 2 leaves behind -- no count / scan launches, no -1 pre-fill of the lists
  const bool v2 = (o.pair_native || o.num_per_loc) && ngroups <= 16384 && kv <= 128;
  FillList fills;                                           // every fill of this call: one launch
  if (o.num_per_loc && (!v2 || n_in == 0)) fills.add(o.num_per_loc, sizeof(int32_t) * kv, 0u);
  if (!v2 && o.pair_native && n_in > 0)
    fills.add(o.pair_native, sizeof(int32_t) * 2 * static_cast<size_t>(kv) * n_in, 0xFFFFFFFFu);
  if (n_in > 0 && n_out > 0 && !prefilled)
    fills.add(o.pair_fwd, sizeof(int32_t) * static_cast<size_t>(kv) * n_out, 0xFFFFFFFFu);
  SPX_HIP(fills.launch(s));
  if (n_in == 0) return 0;
  ConvWs w = carve_conv_ws(ws, p, keys_fit_u32(g.batch, g.out_dims, 4));   // as the count pass
  const int mj = conv3_cands(p);
  count(conv_pass_counter(mj));
  if (mj) {
    const int shares = conv3_shares(n_in, mj);                 // (as the count pass: it wrote one flag plane per share)
    count(conv_shares_counter(shares));
    SPX_CONV3_LAUNCH(conv3_assign_kernel, mj, dim3(div_up(n_in, kBlock), shares), dim3(kBlock), 0, s, p.indices, n_in, g,
                     static_cast<const int32_t *>(w.slot_of), w.nblk, static_cast<const uint32_t *>(w.firstbits),
                     static_cast<const uint8_t *>(w.firstflags), static_cast<const int32_t *>(w.wordpre),
                     static_cast<const int32_t *>(w.blockoff), w.slot_out, o.out_indices, n_out);
    SPX_CONV3_LAUNCH(conv3_pairs_kernel, mj, dim3(div_up(n_in, kBlock)), dim3(kBlock), 0, s, p.indices, n_in, g,
                     static_cast<const int32_t *>(w.slot_of), static_cast<const int32_t *>(w.slot_out), n_out,
                     o.pair_fwd, o.pair_bwd, o.mask_bwd, words, v2 ? w.groupcount : nullptr);
  } else {
    hipLaunchKernelGGL(conv_assign_kernel, dim3(w.nblk, kv), dim3(kBlock), 0, s, p.indices, n_in, g, p.transposed,
                       w.slot_of, w.t, w.nblk, w.blockoff, w.slot_out, o.out_indices, n_out);
    hipLaunchKernelGGL(conv_stage2_kernel, dim3(div_up(n_in, kBlock), kv), dim3(kBlock), 0, s, w.slot_of, w.slot_out,
                       n_in, n_out, o.pair_fwd, o.pair_bwd, v2 ? w.groupcount : nullptr);
  }
  {
    const int na = o.mask_fwd ? n_out : 0, nb = (o.mask_bwd && !mj) ? n_in : 0;
    if (na + nb > 0)
      hipLaunchKernelGGL(mask_from_tables_kernel, dim3(div_up(na + nb, kBlock)), dim3(kBlock), 0, s, o.pair_fwd,
                         na, o.mask_fwd, o.pair_bwd, nb, o.mask_bwd, kv, words);
  }
  SPX_LAUNCH_CHECK();
  if (v2) {
    SPX_CHECK(!o.pair_native || o.num_per_loc, "num_per_loc is required with pair_native");
    hipLaunchKernelGGL(subm_lists_kernel, dim3(w.nblk, kv), dim3(kBlock), 0, s, o.pair_bwd, kv, n_in, ngroups,
                       w.groupcount, o.pair_native, o.num_per_loc, 0, 1);
    SPX_LAUNCH_CHECK();
    return 0;
  }
  if (o.pair_native) {
    SPX_CHECK(o.num_per_loc, "num_per_loc is required with pair_native");
    count(kRbConvListsV1);
  }
  if (o.num_per_loc && launch_native_lists(o.pair_bwd, 1, kv, n_in, kv, w.nblk, w.blockcount, w.blockoff, o.pair_native,
                                           o.num_per_loc, s))
    return -2;
  return 0;
}
}  // namespace
}  // namespace spx

using namespace spx;

extern "C" {

size_t spx_conv_rulebook_ws_bytes(int n_in, int ndim, const int *ksize, const int *stride, const int *dilation,
                                  int transposed) {
  if (ndim < 1 || ndim > kMaxNdim) return 0;
  return conv_ws_bytes({nullptr, n_in, ndim, 0, nullptr, nullptr, ksize, stride, nullptr, dilation, transposed});
}

int spx_conv_rulebook_count(const int32_t *indices, int n_in, int ndim, int batch_size, const int *in_shape,
                            const int *out_shape, const int *ksize, const int *stride, const int *padding,
                            const int *dilation, int transposed, void *ws, size_t ws_bytes, int *n_out_h,
                            spx_stream_t stream) {
  const ConvProblem p{indices, n_in, ndim, batch_size, in_shape, out_shape, ksize, stride, padding, dilation, transposed};
  hipStream_t s = static_cast<hipStream_t>(stream);
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  int overflow = 0;
  if (!n_out_h) return conv_count_impl(p, ws, ws_bytes, nullptr, &overflow, 0, s);   // nothing read back: the bound
  const unsigned long long key = geometry_key(p);
  const size_t expect = expected_outputs(key, n_in);
  int rc = conv_count_impl(p, ws, ws_bytes, n_out_h, &overflow, expect, s);
  if (rc) return rc;
  if (overflow && expect > 0) {          // the expectation was too small: once more, at the bound
    count(kRbConvRetry);
    rc = conv_count_impl(p, ws, ws_bytes, n_out_h, &overflow, 0, s);
    if (rc) return rc;
  }
  SPX_CHECK(overflow == 0, "output hash table overflow: more distinct outputs than the bound %zu",
            conv_max_out(n_in, ndim, ksize, stride, dilation, transposed));
  if (n_in > 0) remember_outputs(key, n_in, *n_out_h);
  return 0;
}

int spx_conv_rulebook_fill(const int32_t *indices, int n_in, int ndim, int batch_size, const int *in_shape,
                           const int *out_shape, const int *ksize, const int *stride, const int *padding,
                           const int *dilation, int transposed, int n_out, int32_t *out_indices, int32_t *pair_fwd,
                           int32_t *pair_bwd, uint32_t *mask_fwd, uint32_t *mask_bwd, int32_t *pair_native,
                           int32_t *num_per_loc, void *ws, size_t ws_bytes, spx_stream_t stream) {
  const ConvProblem p{indices, n_in, ndim, batch_size, in_shape, out_shape, ksize, stride, padding, dilation, transposed};
  const ConvOutputs o{n_out, out_indices, pair_fwd, pair_bwd, mask_fwd, mask_bwd, pair_native, num_per_loc};
  return conv_fill_impl(p, o, ws, ws_bytes, static_cast<hipStream_t>(stream), false);
}

// Every launch is stream-ordered and nothing is read back: the whole call can sit in a hipGraph.  Rows past the number
// of distinct outputs keep out_indices = -1 (a dead row for the next layer: subm_insert_kernel / conv_stage1_kernel skip
// batch < 0), pair_fwd = -1, mask = 0.  {distinct outputs found (may exceed the cap: the first n_out_cap survive),
// hash-table overflow flag} are written straight into n_out_dev: two launches and a copy fewer than the two-call form.
int spx_conv_rulebook_static(const int32_t *indices, int n_in, int ndim, int batch_size, const int *in_shape,
                             const int *out_shape, const int *ksize, const int *stride, const int *padding,
                             const int *dilation, int transposed, int n_out_cap, int32_t *out_indices,
                             int32_t *pair_fwd, int32_t *pair_bwd, uint32_t *mask_fwd, uint32_t *mask_bwd,
                             int32_t *pair_native, int32_t *num_per_loc, int32_t *n_out_dev, void *ws,
                             size_t ws_bytes, spx_stream_t stream) {
  const ConvProblem p{indices, n_in, ndim, batch_size, in_shape, out_shape, ksize, stride, padding, dilation, transposed};
  const ConvOutputs o{n_out_cap, out_indices, pair_fwd, pair_bwd, mask_fwd, mask_bwd, pair_native, num_per_loc};
  hipStream_t s = static_cast<hipStream_t>(stream);
  FillList pre;
  if (static_prologue(p, o, n_out_dev, pre)) return -1;
  const int rc = conv_count_impl(p, ws, ws_bytes, nullptr, nullptr, static_cast<size_t>(n_out_cap), s, &pre, n_out_dev);
  return rc ? rc : conv_fill_impl(p, o, ws, ws_bytes, s, true);
}

}  // extern "C"
