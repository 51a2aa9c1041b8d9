// SubM rulebooks: spx_subm_rulebook over the hash table (table.h), spx_subm_rulebook_ranked over the rank map of a
// sorted-order level (rankmap.h).  Shared with the other builders: rulebook.h.
#include "rulebook.h"
#include "rankmap.h"

namespace spx {
namespace {

// ---------------------------------------------------------------- SubM

__global__ void __launch_bounds__(kBlock)
subm_insert_kernel(const int32_t *__restrict__ indices, int n, Geom g, Table t,
                   int32_t *__restrict__ slot_of, uint32_t *__restrict__ mask_zero = nullptr,
                   int words = 0, int32_t *__restrict__ fill_fwd = nullptr, int32_t *__restrict__ fill_bwd = nullptr,
                   uint32_t *__restrict__ occupied = nullptr) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (mask_zero)      // the probe kernel ORs bits into the masks: clear them here (no fill launch)
    for (int w = 0; w < words; ++w) mask_zero[static_cast<size_t>(i) * words + w] = 0u;
  // the half of the tables that only receives scattered mirror entries starts as -1: written here, by the row's
  // own thread (coalesced along the rows), instead of by the fill launch -- whose job shrinks to the hash table
  if (fill_fwd)
    for (int k = 0; k < g.kv / 2; ++k) fill_fwd[static_cast<size_t>(k) * n + i] = -1;
  if (fill_bwd)
    for (int k = g.kv / 2 + 1; k < g.kv; ++k) fill_bwd[static_cast<size_t>(k) * n + i] = -1;
  int b, c[4];
  read_row(indices, i, g.ndim, b, c);
  // rows with a batch index outside [0, batch) ("deleted" points, docs/USAGE.md:150)
  // never match a neighbour query in the CPU path either; do not hash them.
  int slot = -1;
  if (b >= 0 && b < g.batch && in_range(c, g.in_dims))
    slot = table_insert_min(t, layout_key(b, c, g.in_dims), i);
  if (slot_of) slot_of[i] = slot;
  // one occupancy bit per slot for subm_probe5_kernel (set again by a duplicate coordinate: idempotent)
  if (occupied && slot >= 0) atomicOr(&occupied[slot >> 5], 1u << (slot & 31));
}

// One thread per (voxel, offset k < kv/2): every probe chain is independent and there are only
// kv/2 probes per voxel -- a hit at offset k from row o to row v is also the pair (kv-1-k) from
// v to o (the mirror symmetry the CPU path uses, indices.py:1685-1696), written as a scattered
// 4-byte store.  The tables are pre-filled with -1 and the masks with 0 (only hits write); the
// mask bits are OR-ed in with atomicOr (commutative: the result does not depend on the order).
// Duplicate coordinates: lookups only ever return the FIRST row of a coordinate
// (unordered_map::insert keeps it, indices.py:1672), so a later duplicate never appears as the
// found side; such a row keeps only its k > centre half, which it probes itself here.
__global__ void __launch_bounds__(kBlock)
subm_probe3_kernel(const int32_t *__restrict__ indices, int n, Geom g, Table t,
                   const int32_t *__restrict__ slot_of, int32_t *__restrict__ pair_fwd,
                   int32_t *__restrict__ pair_bwd, uint32_t *__restrict__ mask, int words,
                   int32_t *__restrict__ native) {
  const int o = blockIdx.x * kBlock + threadIdx.x;
  const int kv = g.kv, center = kv / 2;
  int k = blockIdx.y;                         // 0 .. kv/2 (the last one is the identity offset)
  if (o >= n) return;
  auto set = [&](int kk, int row, int val) __attribute__((always_inline)) {
    pair_fwd[static_cast<size_t>(kk) * n + row] = val;
    if (pair_bwd) pair_bwd[static_cast<size_t>(kv - 1 - kk) * n + row] = val;
    atomicOr(&mask[static_cast<size_t>(row) * words + (kk >> 5)], 1u << (kk & 31));
  };
  if (k == center) {
    set(center, o, o);
    if (native) {                            // identity lists of ConvAlgo.Native (indices.py:1678-1682)
      native[static_cast<size_t>(center) * n + o] = o;
      native[static_cast<size_t>(kv + center) * n + o] = o;
    }
    return;
  }
  const int self = slot_of[o];
  if (self < 0) return;
  const bool first = table_val(t, self) == o;
  if (!first) k = kv - 1 - k;                 // a duplicate row only owns its k > centre half
  int b, c[4], r[4], q[4];
  read_row(indices, o, g.ndim, b, c);
  decode_offset(k, g.ksize, r);
#pragma unroll
  for (int d = 0; d < 4; ++d) q[d] = c[d] - g.padding[d] + r[d] * g.dilation[d];
  if (!in_range(q, g.in_dims)) return;
  const int v = table_find(t, layout_key(b, q, g.in_dims));
  if (v < 0) return;
  set(k, o, v);
  if (first) set(kv - 1 - k, v, o);
}

// Third form of the probe pass: as subm_probe3_kernel, but every thread probes an offset ABOVE the
// centre (k' = kv-1-k), i.e. in the CPU loop's own orientation -- row o is the INPUT row i of list
// L = kv-1-k' and the hit is the output row (indices.py:1685-1696).  The direct entry
// pair_fwd[k'][o] then is the thread's own (coalesced, written whether hit or miss: that half of
// the table needs no -1 pre-fill), only the mirror entry pair_fwd[L][found] = o is scattered, and the
// hits of a block ARE the entries of list L that fall into the block's 256-voxel group: the block
// leaves their count for subm_lists_kernel (no count / scan launches).  A row that is not the first
// of its coordinate still owns its k' entries but writes no mirror entry (lookups return the first
// row only), so the first-row test is needed on hits only.
__global__ void __launch_bounds__(kBlock)
subm_probe4_kernel(const int32_t *__restrict__ indices, int n, Geom g, Table t,
                   const int32_t *__restrict__ slot_of, int32_t *__restrict__ pair_fwd,
                   int32_t *__restrict__ pair_bwd, uint32_t *__restrict__ mask, int words,
                   int32_t *__restrict__ groupcount, int ngroups, int mask_pass = 0) {
  // mask_pass: the masks come from a pass over the finished table instead of one atomicOr per entry
  __shared__ int lds_wave[kBlock / 64];
  const int o = blockIdx.x * kBlock + threadIdx.x;
  const int kv = g.kv, center = kv / 2;
  const int list = blockIdx.y;                // 0 .. kv/2 - 1, or kv/2 = the identity offset
  const int k = kv - 1 - list;                // probed offset (> centre), or the centre itself
  auto set = [&](int kk, int row, int val) __attribute__((always_inline)) {
    pair_fwd[static_cast<size_t>(kk) * n + row] = val;
    if (pair_bwd) pair_bwd[static_cast<size_t>(kv - 1 - kk) * n + row] = val;
  };
  if (list == center) {
    if (o < n) {
      set(center, o, o);
      if (!mask_pass) atomicOr(&mask[static_cast<size_t>(o) * words + (center >> 5)], 1u << (center & 31));
    }
    return;
  }
  int v = -1;
  int b = -1, c[4] = {0, 0, 0, 0};
  if (o < n) {
    read_row(indices, o, g.ndim, b, c);
    if (b >= 0 && b < g.batch && in_range(c, g.in_dims)) {
      int r[4], q[4];
      decode_offset(k, g.ksize, r);
#pragma unroll
      for (int d = 0; d < 4; ++d) q[d] = c[d] - g.padding[d] + r[d] * g.dilation[d];
      if (in_range(q, g.in_dims)) v = table_find(t, layout_key(b, q, g.in_dims));
    }
    set(k, o, v);                             // own entry, hit or miss
    if (v >= 0) {
      if (!mask_pass) atomicOr(&mask[static_cast<size_t>(o) * words + (k >> 5)], 1u << (k & 31));
      const int self = slot_of[o];
      if (self >= 0 && table_val(t, self) == o) {       // first row of its coordinate: mirror entry
        set(list, v, o);
        if (!mask_pass) atomicOr(&mask[static_cast<size_t>(v) * words + (list >> 5)], 1u << (list & 31));
      }
    }
  }
  if (groupcount) {
    const unsigned long long bal = __ballot(v >= 0);
    if ((threadIdx.x & 63) == 0) lds_wave[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
      int sum = 0;
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) sum += lds_wave[w];
      groupcount[static_cast<size_t>(list) * ngroups + blockIdx.x] = sum;
    }
  }
}

// Fifth form of the probe pass: an OCCUPANCY BIT per table slot, staged in LDS, answers most probes.
// A SubM probe asks for a neighbour that, on a sparse scene, is almost never there (config 2: 97 % misses), and
// with linear probing and no deletions a key whose HOME slot is empty was never inserted.  The insert kernel sets
// one bit per occupied slot (cap / 8 bytes: 64 KB at 100 k voxels and 4 N slots); a workgroup of 1024 threads copies
// the bits into LDS once, takes 256 voxels x all their upper-half offsets (thread = voxel x one of four offset
// groups), tests every home slot there, and only goes to the table -- random 8-byte reads, the operation the fourth
// form was rate-bound on (84 G/s device-wide, tools/probes/atomic_probe.hip) -- where the bit is set: the table's
// load factor (0.19-0.38) + the real hits.  The first table word of a thread's offsets is requested in one
// straight-line batch (an inactive lane reads slot 0); walks past the home slot are rare and serial.  Offsets are
// decoded once per workgroup (LDS).  Same entries, same masks, same group counts as subm_probe4_kernel.
constexpr int kP5Chunk = 4, kP5Groups = 4, kP5Threads = kBlock * kP5Groups;
__global__ void __launch_bounds__(kP5Threads, 8)   // two workgroups per CU (64 KB of bits each)
subm_probe5_kernel(const int32_t *__restrict__ indices, int n, Geom g, Table t,
                   const uint32_t *__restrict__ occupied, int fwords, const int32_t *__restrict__ slot_of,
                   int32_t *__restrict__ pair_fwd, int32_t *__restrict__ pair_bwd, uint32_t *__restrict__ mask,
                   int words, int32_t *__restrict__ groupcount, int ngroups, int mask_pass) {
  // [fwords] occupancy bits | [half] int4 coordinate steps | [half] key steps | [half][4] hit counts
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_occ[];
  const int tid = threadIdx.x;
  const int kv = g.kv, center = kv / 2, half = kv / 2;
  int4 *lds_delta = reinterpret_cast<int4 *>(lds_occ + fwords);
  hkey_t *lds_dkey = reinterpret_cast<hkey_t *>(lds_delta + half);
  int *lds_cnt = reinterpret_cast<int *>(lds_dkey + half);
  for (int i = tid; i < fwords / 4; i += kP5Threads)
    reinterpret_cast<uint4 *>(lds_occ)[i] = reinterpret_cast<const uint4 *>(occupied)[i];
  for (int l = tid; l < half; l += kP5Threads) {         // neighbour of list l: offset k = kv - 1 - l (> centre)
    int r[4], dq[4];
    decode_offset(kv - 1 - l, g.ksize, r);
    hkey_t dk = 0;                                       // the key is linear in the coordinates: key(c + dq) = key(c) + dk
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      dq[d] = r[d] * g.dilation[d] - g.padding[d];
      dk = dk * g.in_dims[d] + dq[d];
    }
    lds_delta[l] = make_int4(dq[0], dq[1], dq[2], dq[3]);
    lds_dkey[l] = dk;
  }
  const int o = blockIdx.x * kBlock + (tid & (kBlock - 1));
  const int grp = tid / kBlock;                          // lists grp, grp + 4, ... (uniform per wave)
  int b = -1, c[4] = {0, 0, 0, 0};
  bool valid = false;
  if (o < n) {
    read_row(indices, o, g.ndim, b, c);
    valid = b >= 0 && b < g.batch && in_range(c, g.in_dims);
  }
  __syncthreads();
  auto set = [&](int kk, int row, int val) __attribute__((always_inline)) {
    pair_fwd[static_cast<size_t>(kk) * n + row] = val;
    if (pair_bwd) pair_bwd[static_cast<size_t>(kv - 1 - kk) * n + row] = val;
  };
  const unsigned long long *slots = reinterpret_cast<const unsigned long long *>(t.keys);   // packed slots / wide keys
  const hkey_t key0 = layout_key(b, c, g.in_dims);
  int first = -1;                               // row o is the first of its coordinate: looked up at its first hit
  for (int l0 = grp; l0 < half; l0 += kP5Chunk * kP5Groups) {
    hkey_t key[kP5Chunk];
    uint32_t home[kP5Chunk];
    unsigned long long cur[kP5Chunk];
    bool act[kP5Chunk];
#pragma unroll
    for (int j = 0; j < kP5Chunk; ++j) {
      const int lj = l0 + j * kP5Groups;
      const int l = lj < half ? lj : half - 1;
      const int4 dq = lds_delta[l];
      const int q[4] = {c[0] + dq.x, c[1] + dq.y, c[2] + dq.z, c[3] + dq.w};
      key[j] = key0 + lds_dkey[l];
      home[j] = table_home(t, key[j]);
      bool a = valid && lj < half && in_range(q, g.in_dims);
      if (fwords) a = a && ((lds_occ[home[j] >> 5] >> (home[j] & 31)) & 1u);
      act[j] = a;
      cur[j] = slots[a ? home[j] : 0u];
    }
#pragma unroll
    for (int j = 0; j < kP5Chunk; ++j) {
      const int l = l0 + j * kP5Groups;
      const bool live = l < half;                 // (uniform per wave)
      const int k = kv - 1 - l;
      int v = -1;
      if (act[j]) {
        const bool hit = t.packed ? (static_cast<uint32_t>(cur[j] >> 32) == static_cast<uint32_t>(key[j]) &&
                                     cur[j] != kEmptySlot)
                                  : cur[j] == static_cast<unsigned long long>(key[j]);
        if (hit) v = t.packed ? static_cast<int32_t>(static_cast<uint32_t>(cur[j])) : t.vals[home[j]];
        else if (cur[j] != kEmptySlot)
          v = table_find_from(t, key[j], (home[j] + (1u << t.gbits)) & t.mask, 1u);
      }
      if (live && o < n) {
        set(k, o, v);                             // own entry, hit or miss
        if (v >= 0) {
          if (!mask_pass) atomicOr(&mask[static_cast<size_t>(o) * words + (k >> 5)], 1u << (k & 31));
          if (first < 0) {
            const int self = slot_of[o];
            first = (self >= 0 && table_val(t, self) == o) ? 1 : 0;
          }
          if (first) {                            // first row of its coordinate: mirror entry
            set(l, v, o);
            if (!mask_pass) atomicOr(&mask[static_cast<size_t>(v) * words + (l >> 5)], 1u << (l & 31));
          }
        }
      }
      if (groupcount && live) {
        const unsigned long long bal = __ballot(v >= 0);
        if ((tid & 63) == 0) lds_cnt[l * 4 + ((tid >> 6) & 3)] = __popcll(bal);
      }
    }
  }
  if (grp == 0 && o < n) {
    set(center, o, o);
    if (!mask_pass) atomicOr(&mask[static_cast<size_t>(o) * words + (center >> 5)], 1u << (center & 31));
  }
  if (groupcount) {                               // hits per (list, 256-voxel group), as the fourth form leaves them
    __syncthreads();
    for (int l = tid; l < half; l += kP5Threads)
      groupcount[static_cast<size_t>(l) * ngroups + blockIdx.x] =
          lds_cnt[l * 4] + lds_cnt[l * 4 + 1] + lds_cnt[l * 4 + 2] + lds_cnt[l * 4 + 3];
  }
}

// SubM probe pass over the rank map of a level whose rows are in key order (row = rank of its key): as
// subm_probe4_kernel -- same entries, masks and group counts --, the neighbour looked up by rank_of instead of a
// hash walk; every row is the first (and only) row of its coordinate.
__global__ void __launch_bounds__(kBlock)
subm_rank_probe_kernel(const int32_t *__restrict__ indices, int n, Geom g, const uint2 *__restrict__ cells,
                       const int32_t *__restrict__ blockoff, int32_t *__restrict__ pair_fwd, int32_t *__restrict__ pair_bwd,
                       uint32_t *__restrict__ mask, int words, int32_t *__restrict__ groupcount, int ngroups,
                       int mask_pass) {
  __shared__ int lds_wave[kBlock / 64];
  const int o = blockIdx.x * kBlock + threadIdx.x;
  const int kv = g.kv, center = kv / 2;
  const int list = blockIdx.y;                // 0 .. kv/2 - 1, or kv/2 = the identity offset
  const int k = kv - 1 - list;                // probed offset (> centre), or the centre itself
  auto set = [&](int kk, int row, int val) __attribute__((always_inline)) {
    pair_fwd[static_cast<size_t>(kk) * n + row] = val;
    if (pair_bwd) pair_bwd[static_cast<size_t>(kv - 1 - kk) * n + row] = val;
  };
  if (list == center) {
    if (o < n) {
      set(center, o, o);
      if (!mask_pass) atomicOr(&mask[static_cast<size_t>(o) * words + (center >> 5)], 1u << (center & 31));
    }
    return;
  }
  int v = -1;
  if (o < n) {
    int b, c[4];
    read_row(indices, o, g.ndim, b, c);
    if (b >= 0 && b < g.batch && in_range(c, g.in_dims)) {
      int r[4], q[4];
      decode_offset(k, g.ksize, r);
#pragma unroll
      for (int d = 0; d < 4; ++d) q[d] = c[d] - g.padding[d] + r[d] * g.dilation[d];
      if (in_range(q, g.in_dims)) {
        v = rank_of(cells, blockoff, static_cast<unsigned long long>(layout_key(b, q, g.in_dims)));
        if (v >= n) v = -1;                   // (an output the producing layer's bound dropped)
      }
      set(k, o, v);                           // own entry, hit or miss
      if (v >= 0) {
        if (!mask_pass) atomicOr(&mask[static_cast<size_t>(o) * words + (k >> 5)], 1u << (k & 31));
        set(list, v, o);                      // mirror entry
        if (!mask_pass) atomicOr(&mask[static_cast<size_t>(v) * words + (list >> 5)], 1u << (list & 31));
      }
    } else {
      set(k, o, -1);                          // a dead row (static shapes): no neighbours, and nobody's neighbour
    }
  }
  if (groupcount) {
    const unsigned long long bal = __ballot(v >= 0);
    if ((threadIdx.x & 63) == 0) lds_wave[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
      int sum = 0;
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) sum += lds_wave[w];
      groupcount[static_cast<size_t>(list) * ngroups + blockIdx.x] = sum;
    }
  }
}

// SubM build over a rank map, ROW-OWNED: one thread per row looks up ALL its neighbours itself (a lookup is one 8-byte
// load, and in key order the three x-offsets of a (dz, dy) pair share a word) and writes its whole column of the
// table(s) and its mask word -- no mirror scatter, no atomicOr, no -1 pre-fill, one launch.  Same tables, masks and
// list counts as subm_rank_probe_kernel / subm_probe4_kernel (tests/test_gpu_sorted.py: torch.equal to the hash build).
constexpr int kRowsChunk = 9;
__global__ void __launch_bounds__(kBlock)
subm_rank_rows_kernel(const int32_t *__restrict__ indices, int n, Geom g, const uint2 *__restrict__ cells,
                      const int32_t *__restrict__ blockoff, int32_t *__restrict__ pair_fwd,
                      int32_t *__restrict__ pair_bwd, uint32_t *__restrict__ mask, int words,
                      int32_t *__restrict__ groupcount, int ngroups) {
  // [kv] coordinate steps | [kv] key steps | [kv] hits of the block per offset
  extern __shared__ __attribute__((aligned(16))) int4 lds_delta[];
  const int kv = g.kv, center = kv / 2;
  hkey_t *lds_dkey = reinterpret_cast<hkey_t *>(lds_delta + kv);
  int *lds_cnt = reinterpret_cast<int *>(lds_dkey + kv);
  for (int k = threadIdx.x; k < kv; k += kBlock) {
    int r[4], dq[4];
    decode_offset(k, g.ksize, r);
    hkey_t dk = 0;                                         // the key is linear in the coordinates
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      dq[d] = r[d] * g.dilation[d] - g.padding[d];
      dk = dk * g.in_dims[d] + dq[d];
    }
    lds_delta[k] = make_int4(dq[0], dq[1], dq[2], dq[3]);
    lds_dkey[k] = dk;
    lds_cnt[k] = 0;
  }
  const int o = blockIdx.x * kBlock + threadIdx.x;
  int b = -1, c[4] = {0, 0, 0, 0};
  bool valid = false;
  if (o < n) {
    read_row(indices, o, g.ndim, b, c);
    valid = b >= 0 && b < g.batch && in_range(c, g.in_dims);
  }
  __syncthreads();
  const hkey_t key0 = layout_key(b, c, g.in_dims);
  uint32_t mword = 0;
  for (int k0 = 0; k0 < kv; k0 += kRowsChunk) {
    uint2 cell[kRowsChunk];
    hkey_t key[kRowsChunk];
    bool act[kRowsChunk];
#pragma unroll
    for (int j = 0; j < kRowsChunk; ++j) {                 // the chunk's loads in one straight-line batch
      const int k = k0 + j < kv ? k0 + j : kv - 1;
      const int4 dq = lds_delta[k];
      const int q[4] = {c[0] + dq.x, c[1] + dq.y, c[2] + dq.z, c[3] + dq.w};
      key[j] = key0 + lds_dkey[k];
      act[j] = valid && k0 + j < kv && k != center && in_range(q, g.in_dims);
      cell[j] = cells[act[j] ? static_cast<unsigned long long>(key[j]) >> 5 : 0ull];
    }
#pragma unroll
    for (int j = 0; j < kRowsChunk; ++j) {
      const int k = k0 + j;
      const bool live = k < kv;                            // (uniform; no break: the loop must unroll -- cell[] in registers)
      int v = -1;
      if (act[j]) {
        const uint32_t bit = 1u << (static_cast<unsigned long long>(key[j]) & 31);
        if (cell[j].x & bit)
          v = blockoff[static_cast<unsigned long long>(key[j]) >> 16] + static_cast<int>(cell[j].y) +
              __popc(cell[j].x & (bit - 1u));
        if (v >= n) v = -1;                                // (an output the producing layer's bound dropped)
      }
      if (k == center && o < n) v = o;                     // (dead rows of a static level too: as the other forms)
      if (live && o < n) {
        pair_fwd[static_cast<size_t>(k) * n + o] = v;
        if (pair_bwd) pair_bwd[static_cast<size_t>(kv - 1 - k) * n + o] = v;
      }
      if (live && v >= 0) mword |= 1u << (k & 31);
      if (live && o < n && ((k & 31) == 31 || k == kv - 1)) {
        mask[static_cast<size_t>(o) * words + (k >> 5)] = mword;
        mword = 0;
      }
      if (groupcount && live && k > center) {              // list kv - 1 - k: the pairs found through offset k
        const unsigned long long bal = __ballot(v >= 0);
        if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&lds_cnt[k], __popcll(bal));
      }
    }
  }
  if (groupcount) {
    __syncthreads();
    for (int l = threadIdx.x; l < center; l += kBlock)
      groupcount[static_cast<size_t>(l) * ngroups + blockIdx.x] = lds_cnt[kv - 1 - l];
  }
}

struct SubmWs {
  Table t;
  int32_t *blockcount, *blockoff, *scratch_totals, *slot_of, *groupcount;
  uint32_t *occupied;                  // occupancy bit per table slot (subm_probe5_kernel)
  int nblk, nblk256;
  size_t bytes;
};

// 4 N slots instead of 2 N while the table stays within 8 MB (two XCD L2s): at load 0.1-0.19 a lookup resolves in
// ~1.2 probes instead of ~2 -- SubM tables 40.8 -> 36.9 us at 100 k uniform voxels, 67.1 -> 54.6 on the 125 k fixture;
// beyond (400 k voxels: 16 MB) the extra lines cost more than the probes save (151 -> 159 us).  The workspace keeps
// room for 4 N slots at every size (the size query promises callers one formula); the table sits at its head.
SubmWs carve_subm_ws(void *ws, int n, int kv, bool packed = false) {
  const int rows = n > 0 ? n : 1;
  uint32_t cap = table_capacity(rows);
  const uint32_t room = cap << 1;
  if (cap <= (1u << 19)) cap <<= 1;
  SubmWs w;
  w.nblk = div_up(rows, kItems);
  w.nblk256 = div_up(rows, kBlock);
  Carver cv(ws);
  {
    hkey_t *keys = cv.take<hkey_t>(room);
    cv.take<int32_t>(room);
    table_place(w.t, keys, reinterpret_cast<int32_t *>(keys + cap), cap, packed);
  }
  w.blockcount = cv.take<int32_t>(static_cast<size_t>(kv) * w.nblk);
  w.blockoff = cv.take<int32_t>(static_cast<size_t>(kv) * w.nblk);
  w.scratch_totals = cv.take<int32_t>(64);                 // list totals when num_per_loc is NULL
  w.slot_of = cv.take<int32_t>(rows);                      // hash slot of every row
  w.groupcount = cv.take<int32_t>(static_cast<size_t>(kv / 2 + 1) * w.nblk256);   // hits per (list, 256-voxel group)
  w.occupied = cv.take<uint32_t>(room / 32);
  w.bytes = cv.off;
  return w;
}

struct RankedWs {
  int32_t *scratch_totals, *groupcount;
  size_t bytes;
};
RankedWs carve_ranked_ws(void *ws, int n, int kv) {
  RankedWs w;
  Carver cv(ws);
  w.scratch_totals = cv.take<int32_t>(64);
  w.groupcount = cv.take<int32_t>(static_cast<size_t>(kv / 2 + 1) * div_up(n > 0 ? n : 1, kBlock));
  w.bytes = cv.off;
  return w;
}

// What both SubM builds start with: the geometry of a SubM problem (stride 1, "same" padding) after its checks.
// Returns 1 when there are no rows (num_per_loc zeroed: the build is done), 0 to go on, < 0 on error.
int subm_begin(int n, int ndim, int batch_size, const int *spatial_shape, const int *ksize, const int *dilation,
               const int32_t *pair_fwd, const uint32_t *mask, int32_t *num_per_loc, hipStream_t s, Geom &g) {
  int padding[4], stride[4] = {1, 1, 1, 1}, kv = 1;
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  for (int i = 0; i < ndim; ++i) {
    SPX_CHECK(ksize[i] % 2 == 1, "subm only support odd ksize");  // indices.py:1650
    padding[i] = (ksize[i] / 2) * dilation[i];                    // indices.py:1652
    kv *= ksize[i];
  }
  if (check_geom(ndim, n, kv)) return -1;
  if (n == 0) {
    if (num_per_loc) SPX_HIP(hipMemsetAsync(num_per_loc, 0, sizeof(int32_t) * kv, s));
    return 1;
  }
  SPX_CHECK(pair_fwd && mask, "pair_fwd and mask are required");
  g = make_geom(ndim, batch_size, spatial_shape, spatial_shape, ksize, stride, padding, dilation);
  return 0;
}

// ConvAlgo.Native lists (or just their lengths) of a finished SubM table, from the group counts its probe pass left.
int subm_lists(const int32_t *pair_fwd, int kv, int n, const int32_t *groupcount, int32_t *pair_native,
               int32_t *num_per_loc, int32_t *scratch_totals, hipStream_t s) {
  SPX_CHECK(!pair_native || num_per_loc || kv / 2 <= 64, "num_per_loc required for kv > 128");
  hipLaunchKernelGGL(subm_lists_kernel, dim3(div_up(n, kItems), kv / 2 + 1), dim3(kBlock), 0, s, pair_fwd, kv, n,
                     div_up(n, kBlock), groupcount, pair_native, num_per_loc ? num_per_loc : scratch_totals,
                     num_per_loc ? kv : 0);
  return 0;
}

}  // namespace
}  // namespace spx

using namespace spx;

extern "C" {

size_t spx_subm_rulebook_ws_bytes(int n, int kv) { return carve_subm_ws(nullptr, n, kv).bytes; }

int spx_subm_rulebook(const int32_t *indices, int n, int ndim, int batch_size, const int *spatial_shape,
                      const int *ksize, const int *dilation, int32_t *pair_fwd, int32_t *pair_bwd, uint32_t *mask,
                      int32_t *pair_native, int32_t *num_per_loc, void *ws, size_t ws_bytes, spx_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  Geom g;
  if (const int rc = subm_begin(n, ndim, batch_size, spatial_shape, ksize, dilation, pair_fwd, mask, num_per_loc, s, g))
    return rc < 0 ? rc : 0;
  const int kv = g.kv, words = div_up(kv, 32);
  SPX_CHECK(ws_bytes >= spx_subm_rulebook_ws_bytes(n, kv), "workspace too small: %zu < %zu", ws_bytes,
            spx_subm_rulebook_ws_bytes(n, kv));
  const SubmWs w = carve_subm_ws(ws, n, kv, keys_fit_u32(g.batch, g.in_dims, 4));
  const uint32_t cap = w.t.mask + 1u;
  // probe pass, fifth form (subm_probe5_kernel): behind an occupancy bit per slot in LDS for tables up to 2^19 slots
  // (64 KB of bits, two workgroups per CU) -- the north star's "LDS-staged open-address hashing".  Measured
  // (profiles/r04_experiments.md 1f, r05 7): 35.4 vs 36.9 us at 100 k uniform voxels, level at 100-125 k LiDAR-density
  // voxels; without the bits (beyond 2^19 slots 128 KB of bits would leave one workgroup per CU) the fourth form is
  // faster (150 vs 163 us at 400 k) and stays.
  const bool probe5 = option_int("SPX_SUBM_PROBE", 5) >= 5 && cap >= 1024u && cap <= (1u << 19) && kv <= 128;
  const dim3 grid(w.nblk256);
  // second generation: 4 launches (table fill, insert, probe, lists), no table pre-fills; beyond ~4 M voxels the lists
  // kernel's in-block prefix over the group counts would dominate.  third form: fills (table, lower half of pair_fwd
  // [+ pair_bwd's upper half]) -> insert (+ mask clear) -> probe4 (block-local list counts) -> lists: 11 MB of fills, not 34
  if (kv > 1 && kv <= 128 && w.nblk256 <= 16384) {
    FillList fills;                    // the hash table only: the -1 halves of the tables ride in the insert kernel
    table_fill(fills, w.t);            // (pair_fwd rows k < centre; pair_bwd[kv-1-kk] mirrors pair_fwd[kk]: its rows above)
    if (probe5) fills.add(w.occupied, cap / 8, 0u);
    SPX_HIP(fills.launch(s));
    // masks from a pass over the finished table instead of one atomicOr per entry: the extra launch costs 5-10 us at
    // 100 k voxels, the saved atomics (20-25 G/s device-wide) win from ~250 k (400 k: 162 -> 151 us); -1 = by size
    const int mp_opt = option_int("SPX_SUBM_MASK_PASS", -1);
    const int mask_pass = mp_opt < 0 ? (n >= 250000 ? 1 : 0) : mp_opt;
    hipLaunchKernelGGL(subm_insert_kernel, grid, dim3(kBlock), 0, s, indices, n, g, w.t, w.slot_of,
                       mask_pass ? static_cast<uint32_t *>(nullptr) : mask, words, pair_fwd, pair_bwd,
                       probe5 ? w.occupied : static_cast<uint32_t *>(nullptr));
    const bool lists = pair_native || num_per_loc;
    count(probe5 ? kRbSubmProbe5 : kRbSubmProbe4);
    if (probe5) {
      const int fwords = static_cast<int>(cap / 32);
      const size_t lds = static_cast<size_t>(fwords) * 4 + static_cast<size_t>(kv / 2) * (16 + 8 + 16);
      static std::atomic<uint64_t> attr_done{0};      // one bit per device (common.h: ensure_dynamic_lds)
      SPX_HIP(ensure_dynamic_lds(reinterpret_cast<const void *>(&subm_probe5_kernel), 160 * 1024, attr_done));
      hipLaunchKernelGGL(subm_probe5_kernel, grid, dim3(kP5Threads), lds, s, indices, n, g, w.t, w.occupied, fwords,
                         w.slot_of, pair_fwd, pair_bwd, mask, words, lists ? w.groupcount : nullptr, w.nblk256, mask_pass);
    } else {
      hipLaunchKernelGGL(subm_probe4_kernel, dim3(w.nblk256, kv / 2 + 1), dim3(kBlock), 0, s, indices, n,
                         g, w.t, w.slot_of, pair_fwd, pair_bwd, mask, words, lists ? w.groupcount : nullptr, w.nblk256,
                         mask_pass);
    }
    if (mask_pass) {
      count(kRbSubmMaskPass);
      hipLaunchKernelGGL(mask_from_table_kernel, grid, dim3(kBlock), 0, s, pair_fwd, kv, n, words, mask);
    }
    if (lists) {
      count(kRbSubmLists);
      if (subm_lists(pair_fwd, kv, n, w.groupcount, pair_native, num_per_loc, w.scratch_totals, s)) return -1;
    }
    SPX_LAUNCH_CHECK();
    return 0;
  }
  // every fill of this build in one launch: hash table, masks, counts, -1 tables (callers that carve the tables out of
  // one buffer get one contiguous range)
  FillList fills;
  table_fill(fills, w.t);
  fills.add(mask, sizeof(uint32_t) * static_cast<size_t>(n) * words, 0u);
  if (num_per_loc) fills.add(num_per_loc, sizeof(int32_t) * kv, 0u);
  {
    const size_t tb = sizeof(int32_t) * static_cast<size_t>(kv) * n;
    fills.add(pair_fwd, tb, 0xFFFFFFFFu);
    if (pair_bwd) fills.add(pair_bwd, tb, 0xFFFFFFFFu);
    if (pair_native) fills.add(pair_native, 2 * tb, 0xFFFFFFFFu);
  }
  SPX_HIP(fills.launch(s));
  hipLaunchKernelGGL(subm_insert_kernel, grid, dim3(kBlock), 0, s, indices, n, g, w.t, w.slot_of);
  count(kRbSubmProbe3);
  hipLaunchKernelGGL(subm_probe3_kernel, dim3(w.nblk256, kv / 2 + 1), dim3(kBlock), 0, s, indices, n, g, w.t,
                     w.slot_of, pair_fwd, pair_bwd, mask, words, pair_native);
  SPX_LAUNCH_CHECK();
  if (pair_native) {
    SPX_CHECK(num_per_loc || kv / 2 <= 64, "num_per_loc required for kv > 128");
    if (kv / 2 > 0) count(kRbNativeListsV1);
  }
  // num_per_loc: counts only for k < kv/2 (indices.py:1685,1692)
  if ((pair_native || num_per_loc) &&
      launch_native_lists(pair_fwd, 0, kv, n, kv / 2, w.nblk, w.blockcount, w.blockoff, pair_native,
                          num_per_loc ? num_per_loc : w.scratch_totals, s))
    return -2;
  return 0;
}

size_t spx_subm_rulebook_ranked_ws_bytes(int n, int kv) { return carve_ranked_ws(nullptr, n, kv).bytes + 256; }

int spx_subm_rulebook_ranked(const int32_t *indices, int n, int ndim, int batch_size, const int *spatial_shape,
                             const int *ksize, const int *dilation, int32_t *pair_fwd, int32_t *pair_bwd,
                             uint32_t *mask, int32_t *pair_native, int32_t *num_per_loc, const void *rankmap,
                             size_t rankmap_bytes, void *ws, size_t ws_bytes, spx_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  Geom g;
  if (const int rc = subm_begin(n, ndim, batch_size, spatial_shape, ksize, dilation, pair_fwd, mask, num_per_loc, s, g))
    return rc < 0 ? rc : 0;
  const int kv = g.kv, words = div_up(kv, 32), nblk256 = div_up(n, kBlock);
  SPX_CHECK(kv > 1 && kv <= 128 && nblk256 <= 16384, "ranked SubM build: 1 < kernel volume <= 128, <= 4 M rows");
  const size_t W = rank_words(ndim, batch_size, spatial_shape);
  SPX_CHECK(W > 0 && rankmap && rankmap_bytes >= rank_bytes(W), "rank map missing or too small (%zu words)", W);
  SPX_CHECK(ws && ws_bytes >= spx_subm_rulebook_ranked_ws_bytes(n, kv), "workspace too small");
  const RankedWs w = carve_ranked_ws(ws, n, kv);
  const uint2 *cells = static_cast<const uint2 *>(rankmap);
  const int32_t *blockoff = rank_blockoff(const_cast<void *>(rankmap), W);
  const bool lists = pair_native || num_per_loc;
  // row-owned form from ~200 k rows (28 vs 35-37 us at 313-326 k rows); below, one thread per row is too few threads to
  // hide its lookups (19 vs 14 us at 77 k) and the probe form stays.  SPX_SUBM_RANK_ROWS = 1 / 0 forces / forbids.
  const int rows_opt = option_int("SPX_SUBM_RANK_ROWS", -1);
  if (rows_opt > 0 || (rows_opt < 0 && n >= 196608)) {
    // every entry of the tables and the masks is written by its row's thread -- no fill launch
    const size_t lds = static_cast<size_t>(kv) * (sizeof(int4) + sizeof(hkey_t) + sizeof(int));
    hipLaunchKernelGGL(subm_rank_rows_kernel, dim3(nblk256), dim3(kBlock), lds, s, indices, n, g, cells, blockoff,
                       pair_fwd, pair_bwd, mask, words, lists ? w.groupcount : nullptr, nblk256);
  } else {
    // probe form (SPX_SUBM_RANK_ROWS = 0, for A/B runs): thread per (row, upper offset), mirror entries scattered.
    // masks by atomicOr, at every size: rows in key order keep a wave's mask words in a few lines (measured 34.5 vs
    // 45.0 us with the table pass at 313 k rows, 36.9 vs 48.0 at 326 k; the hash build of shuffled rows switches at 250 k)
    const int mp_opt = option_int("SPX_SUBM_MASK_PASS", -1);
    const int mask_pass = mp_opt < 0 ? 0 : mp_opt;
    // what subm_insert_kernel writes on the hash path: the halves of the tables that only receive scattered mirror
    // entries start as -1, the masks (atomicOr targets without the mask pass) as 0
    FillList fills;
    fills.add(pair_fwd, sizeof(int32_t) * static_cast<size_t>(kv / 2) * n, 0xFFFFFFFFu);
    if (pair_bwd)
      fills.add(pair_bwd + static_cast<size_t>(kv / 2 + 1) * n, sizeof(int32_t) * static_cast<size_t>(kv - kv / 2 - 1) * n,
                0xFFFFFFFFu);
    if (!mask_pass) fills.add(mask, sizeof(uint32_t) * static_cast<size_t>(n) * words, 0u);
    SPX_HIP(fills.launch(s));
    hipLaunchKernelGGL(subm_rank_probe_kernel, dim3(nblk256, kv / 2 + 1), dim3(kBlock), 0, s, indices, n, g, cells,
                       blockoff, pair_fwd, pair_bwd, mask, words, lists ? w.groupcount : nullptr, nblk256, mask_pass);
    if (mask_pass)
      hipLaunchKernelGGL(mask_from_table_kernel, dim3(nblk256), dim3(kBlock), 0, s, pair_fwd, kv, n, words, mask);
  }
  if (lists && subm_lists(pair_fwd, kv, n, w.groupcount, pair_native, num_per_loc, w.scratch_totals, s)) return -1;
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
