// The build-time hash table of the index builders (rulebook_*.hip, voxelize.hip; hash.hip borrows its hash function) and
// the coordinate helpers that make its keys.  Every definition has internal linkage.
//
// One open-addressing table in global memory.  Whenever the key space (batch x grid volume) fits 32 bits -- every
// configuration in BASELINE.json does -- a slot is ONE 64-bit word {key32 : value32}: an insert is a single atomicCAS
// (plus an atomicMin only when a duplicate key has to lower the value) and a probe is a single 8-byte load.  Larger
// key spaces use separate int64 key / int32 value arrays.  At 2x load headroom the packed table is 2 MB per 100k
// voxels and stays in the 4 MiB XCD-local L2.  Duplicate keys are resolved with atomicMin (smallest index wins == the
// CPU path's unordered_map::insert), so nothing depends on the order in which threads arrive.
#pragma once
#include "common.h"
#include "fill.h"

namespace spx {
namespace {
typedef long long hkey_t;      // EMPTY == -1

struct Table {
  hkey_t *keys;    // wide: keys[cap].  packed: slots[cap], slot = (key32 << 32) | value32
  int32_t *vals;   // wide: vals[cap].  packed: the low halves of the slots (stride 2)
  uint32_t mask;   // capacity - 1 (capacity is a power of two)
  int packed;      // 1 when every key fits 32 bits
  int gbits;       // low key bits that pick the slot inside a group of 2^gbits slots (see hash_key)
  uint32_t max_probe;  // longest probe walk (slots - 1).  A table sized for the guaranteed bound is never more than
                       // half full and walks a handful of slots; a table sized for the outputs EXPECTED
                       // (table_shrink: static bound / last ratio) can fill up, and without a cap every insert and
                       // lookup of a key that no longer fits would walk all of it -- O(capacity) per candidate.
                       // Inserts and lookups share the cap, so a key that went in is found; one that did not fit
                       // raises the overflow flag of its pass (the count's read-back / the static form's counter).
};
constexpr uint32_t kMaxProbeShrunk = 2047;

constexpr unsigned long long kEmptySlot = ~0ull;

// Home slot of a key: the murmur3 finaliser of key >> gbits picks a group of 2^gbits slots, the low key
// bits the slot inside it (gbits = 3: 8 consecutive cells along the last spatial dimension share one
// 64-byte line of the table).  Measured and left at gbits = 0 everywhere: on the half-full SubM tables
// groups that are either empty or full turn every collision into a walk across a full group (fixture
// rulebook 78 -> 139 us); on the 4-8 % full regular-conv tables the lookups get 5-12 % faster
// (conv_count_first 8.5 -> 7.5, conv_assign 19.6 -> 18.0 us) but the inserts of neighbouring threads
// now contend for the same lines (conv_stage1 22.6 -> 30.6 us).  Results never depend on the slot.
__device__ __forceinline__ uint32_t hash_key(hkey_t k, int gbits) {
  // murmur3 fmix64
  unsigned long long x = static_cast<unsigned long long>(k) >> gbits;
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return (static_cast<uint32_t>(x) << gbits) | (static_cast<uint32_t>(k) & ((1u << gbits) - 1u));
}

__device__ __forceinline__ uint32_t hash_key32(uint32_t k, int gbits) {
  // murmur3 fmix32
  uint32_t x = k >> gbits;
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return (x << gbits) | (k & ((1u << gbits) - 1u));
}

// Value stored in a slot returned by table_insert_min.
__device__ __forceinline__ int32_t table_val(const Table &t, int slot) {
  return t.vals[static_cast<size_t>(slot) << t.packed];
}

// Inserts key (if absent) and lowers its value to min(value, val). Returns the slot.
template <bool LOOK = false>
__device__ __forceinline__ int table_insert_min(const Table &t, hkey_t key, int32_t val) {
  if (t.packed) {
    unsigned long long *slots = reinterpret_cast<unsigned long long *>(t.keys);
    const uint32_t k32 = static_cast<uint32_t>(key);
    const unsigned long long want =
        (static_cast<unsigned long long>(k32) << 32) | static_cast<uint32_t>(val);
    uint32_t slot = hash_key32(k32, t.gbits) & t.mask;
    for (uint32_t probe = 0; probe <= t.max_probe; ++probe) {  // bounded: the table is never full (or capped)
      // look before the atomic: a slot only ever goes empty -> key, and its value only decreases, so a
      // (possibly stale) plain read that shows our key with a value <= ours, or another key, is final --
      // several inputs reach the same output on dense scenes, and all but the winner leave here
      // (LOOK: regular-conv builders; SubM keys are distinct, there the read would only add latency)
      unsigned long long cur = LOOK ? slots[slot] : kEmptySlot;
      if (cur == kEmptySlot) {
        cur = atomicCAS(&slots[slot], kEmptySlot, want);
        if (cur == kEmptySlot) return static_cast<int>(slot);
      }
      if (static_cast<uint32_t>(cur >> 32) == k32) {
        if (static_cast<uint32_t>(cur) > static_cast<uint32_t>(val)) atomicMin(&slots[slot], want);
        return static_cast<int>(slot);
      }
      slot = (slot + (1u << t.gbits)) & t.mask;      // (stays in its in-line position, see hash_key)
    }
    return -1;
  }
  uint32_t slot = hash_key(key, t.gbits) & t.mask;
  for (uint32_t probe = 0; probe <= t.max_probe; ++probe) {
    unsigned long long prev = LOOK ? static_cast<unsigned long long>(t.keys[slot])     // (as above)
                                   : static_cast<unsigned long long>(-1LL);
    if (prev == static_cast<unsigned long long>(-1LL))
      prev = atomicCAS(reinterpret_cast<unsigned long long *>(&t.keys[slot]),
                       static_cast<unsigned long long>(-1LL), static_cast<unsigned long long>(key));
    if (prev == static_cast<unsigned long long>(-1LL) ||
        prev == static_cast<unsigned long long>(key)) {
      // values start as 0xFFFFFFFF (one memset with the keys): unsigned min
      if (!LOOK || static_cast<unsigned int>(t.vals[slot]) > static_cast<unsigned int>(val))
        atomicMin(reinterpret_cast<unsigned int *>(&t.vals[slot]), static_cast<unsigned int>(val));
      return static_cast<int>(slot);
    }
    slot = (slot + (1u << t.gbits)) & t.mask;
  }
  return -1;
}

// Home slot of a key.
__device__ __forceinline__ uint32_t table_home(const Table &t, hkey_t key) {
  return (t.packed ? hash_key32(static_cast<uint32_t>(key), t.gbits) : hash_key(key, t.gbits)) & t.mask;
}

// Value of key, or -1 when absent (values are row indices / positions, never negative): the walk from `slot`,
// `probe` slots into it.
__device__ __forceinline__ int32_t table_find_from(const Table &t, hkey_t key, uint32_t slot, uint32_t probe) {
  if (t.packed) {
    const unsigned long long *slots = reinterpret_cast<const unsigned long long *>(t.keys);
    const uint32_t k32 = static_cast<uint32_t>(key);
    for (; probe <= t.max_probe; ++probe) {
      const unsigned long long v = slots[slot];
      if (static_cast<uint32_t>(v >> 32) == k32 && v != kEmptySlot) return static_cast<int32_t>(v);
      if (v == kEmptySlot) return -1;
      slot = (slot + (1u << t.gbits)) & t.mask;
    }
    return -1;
  }
  for (; probe <= t.max_probe; ++probe) {
    const hkey_t k = t.keys[slot];
    if (k == key) return t.vals[slot];
    if (k == -1LL) return -1;
    slot = (slot + (1u << t.gbits)) & t.mask;
  }
  return -1;
}

__device__ __forceinline__ int32_t table_find(const Table &t, hkey_t key) {
  return table_find_from(t, key, table_home(t, key), 0u);
}

// Reads one index row (batch, coords...) into canonical 4-d form.
__device__ __forceinline__ void read_row(const int32_t *indices, int i, int ndim, int &b,
                                         int (&c)[4]) {
  if (ndim == 3) {
    const int4 v = reinterpret_cast<const int4 *>(indices)[i];
    b = v.x;
    c[0] = 0;
    c[1] = v.y;
    c[2] = v.z;
    c[3] = v.w;
  } else {
    const int32_t *row = indices + static_cast<size_t>(i) * (ndim + 1);
    b = row[0];
    const int lead = 4 - ndim;
#pragma unroll
    for (int d = 0; d < 4; ++d) c[d] = (d < lead) ? 0 : row[1 + d - lead];
  }
}

__device__ __forceinline__ hkey_t layout_key(int b, const int (&c)[4], const int (&dims)[4]) {
  hkey_t v = b;
#pragma unroll
  for (int d = 0; d < 4; ++d) v = v * dims[d] + c[d];
  return v;
}

__device__ __forceinline__ void decode_offset(int k, const int (&ksize)[4], int (&r)[4]) {
#pragma unroll
  for (int d = 3; d >= 0; --d) {
    r[d] = k % ksize[d];
    k /= ksize[d];
  }
}

__device__ __forceinline__ bool in_range(const int (&c)[4], const int (&dims)[4]) {
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 4; ++d) ok = ok && c[d] >= 0 && c[d] < dims[d];
  return ok;
}

uint32_t table_capacity(size_t entries) {
  size_t cap = 256;
  while (cap < 2 * entries) cap <<= 1;
  return static_cast<uint32_t>(cap);
}

// True when every key of a (batch, dims[0..3]) layout is below 0xFFFFFFFF: the table then keeps
// key and value in one 64-bit slot.
bool keys_fit_u32(long long batch, const int *dims, int ndims) {
  unsigned long long v = batch > 0 ? static_cast<unsigned long long>(batch) : 1ull;
  for (int d = 0; d < ndims; ++d) {
    const unsigned long long e = dims[d] > 0 ? static_cast<unsigned long long>(dims[d]) : 1ull;
    if (v > 0xFFFFFFFFull / e) return false;
    v *= e;
  }
  return v <= 0xFFFFFFFFull;   // largest key is v - 1 <= 0xFFFFFFFE
}

// Places a table of `cap` slots at `mem` (room for the wide form: 12 bytes per slot).
void table_place(Table &t, hkey_t *keys, int32_t *vals, uint32_t cap, bool packed, int gbits = 0) {
  t.keys = keys;
  t.vals = packed ? reinterpret_cast<int32_t *>(keys) : vals;
  t.mask = cap - 1;
  t.packed = packed ? 1 : 0;
  t.gbits = gbits;
  t.max_probe = t.mask;
}

// The same storage as a smaller table (capacity a power of two below the placed one).
void table_shrink(Table &t, uint32_t cap) {
  if (!t.packed) t.vals = reinterpret_cast<int32_t *>(t.keys + cap);
  t.mask = cap - 1;
  t.max_probe = t.mask < kMaxProbeShrunk ? t.mask : kMaxProbeShrunk;
}

// The table's bytes as a 0xFF range of a FillList (see table_clear).
void table_fill(FillList &f, const Table &t) {
  const size_t cap = static_cast<size_t>(t.mask) + 1;
  const size_t bytes = t.packed ? cap * sizeof(unsigned long long)
                                : static_cast<size_t>(reinterpret_cast<char *>(t.vals + cap) -
                                                      reinterpret_cast<char *>(t.keys));
  f.add(t.keys, bytes, 0xFFFFFFFFu);
}

// Empties the table: every byte 0xFF (keys -1, values 0xFFFFFFFF, packed slots ~0).
hipError_t table_clear(const Table &t, hipStream_t s) {
  const size_t cap = static_cast<size_t>(t.mask) + 1;
  const size_t bytes = t.packed ? cap * sizeof(unsigned long long)
                                : static_cast<size_t>(reinterpret_cast<char *>(t.vals + cap) -
                                                      reinterpret_cast<char *>(t.keys));
  return hipMemsetAsync(t.keys, 0xFF, bytes, s);
}
}  // namespace
}  // namespace spx
