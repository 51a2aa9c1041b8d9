// Feature rows as PIECES: the storage / accumulator types of the four floating dtypes, the 16-byte (or one-element)
// piece a lane moves, the index arithmetic of the group reductions' segment walk and of an item = (row, piece) launch
// (row_of), and the host side of a row launch: the checks of a
// floating feature row, the way from (dtype, vec) to a kernel instance, the lanes of a group, the bits of a sort key,
// the grid of a streaming launch.  Shared by the translation units that merge, reduce, score, interpolate or decorate
// rows (union.hip, collapse.hip, select.hip, interp.hip, query.hip, pointvoxel.hip, serialize.hip); every definition has
// internal linkage.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.h"

namespace spx {
namespace {

template <int DT> struct Elem;
template <> struct Elem<SPX_F32> {
  using S = float;
  using A = float;
  static __device__ __forceinline__ A up(S v) { return v; }
  static __device__ __forceinline__ S down(A v) { return v; }
};
template <> struct Elem<SPX_F64> {
  using S = double;
  using A = double;
  static __device__ __forceinline__ A up(S v) { return v; }
  static __device__ __forceinline__ S down(A v) { return v; }
};
template <> struct Elem<SPX_F16> {
  using S = uint16_t;
  using A = float;
  static __device__ __forceinline__ A up(S v) { return static_cast<float>(__builtin_bit_cast(_Float16, v)); }
  static __device__ __forceinline__ S down(A v) { return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v)); }
};
template <> struct Elem<SPX_BF16> {
  using S = uint16_t;
  using A = float;
  static __device__ __forceinline__ A up(S v) { return __builtin_bit_cast(float, static_cast<unsigned>(v) << 16); }
  static __device__ __forceinline__ S down(A x) {            // round to nearest even; NaN stays NaN
    unsigned u = __builtin_bit_cast(unsigned, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return static_cast<uint16_t>(u >> 16);
  }
};

// A piece of a row: V elements, 16 bytes (V = 16 / sizeof(S)) or one element (V = 1: the scalar tail form for rows
// whose byte size is no multiple of 16).
template <typename S, int V> struct alignas(V * sizeof(S)) Piece {
  S e[V];
};

template <typename P> __device__ __forceinline__ P zero_piece() { return P(0); }
template <> __device__ __forceinline__ uint4 zero_piece<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }

// The SEGMENT WALK of a group reduction (collapse_fwd_kernel, interp_bwd_kernel).  Items = (row, lane of its group):
// G = 1 << gshift lanes per row, lane `sub` owns the pieces sub, sub + G, ... and walks the whole segment
// list[offsets[r] .. offsets[r + 1]) for each of them, kAhead entries' loads in flight together, combined in list
// order; a group is never split: that would change the order of the sum.  Shared here: the constant and the index
// arithmetic, item -> (row, lane, clamped segment).  The per-piece loop stays in each kernel: merged into one template
// over load / combine callables it cost registers in some instances of either kernel (profiles/rowlayer_kernels.json).
constexpr int kAhead = 4;             // list entries whose loads are in flight together

struct Segment {
  int r, sub;                         // row, lane of its group
  int beg, end;                       // list[beg .. end), inside [0, limit); empty for a row at or beyond `live`
};

__device__ __forceinline__ Segment segment_of(long long item, int gshift, int live, const int32_t *__restrict__ offsets,
                                              int limit) {
  const int G = 1 << gshift;
  Segment g;
  g.r = static_cast<int>(item >> gshift);
  g.sub = static_cast<int>(item) & (G - 1);
  g.beg = 0;
  g.end = 0;
  if (g.r < live) {
    g.beg = offsets[g.r];
    g.end = offsets[g.r + 1];
    g.beg = g.beg < 0 ? 0 : g.beg;                // (checked, not trusted)
    g.end = g.end > limit ? limit : g.end;
  }
  return g;
}

// row of an item = (row, piece): a 32-bit division wherever the item count allows one
__device__ __forceinline__ long long row_of(long long item, long long total, int pieces) {
  return total <= 0x7fffffffLL ? static_cast<long long>(static_cast<unsigned>(item) / static_cast<unsigned>(pieces))
                               : item / pieces;
}

inline bool aligned_to(const void *p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// workgroups of `block` threads for `total` items (grid-stride loops beyond 2048 workgroups)
inline unsigned stream_blocks(long long total, int block) {
  const long long b = (total + block - 1) / block;
  return static_cast<unsigned>(b < 2048 ? (b < 1 ? 1 : b) : 2048);
}

// widest piece (16 bytes down to one element) that divides the row's byte count and the alignment of every pointer
inline int piece_bytes(int elem_bytes, long long row_bytes, std::initializer_list<const void *> ptrs) {
  int v = 16;
  for (; v > elem_bytes; v >>= 1) {
    bool ok = row_bytes % v == 0;
    for (const void *p : ptrs) ok = ok && (p == nullptr || aligned_to(p, v));
    if (ok) break;
  }
  return v;
}

// The checks of a floating feature row [*, C] that need no pointer; returns the bytes of an element, or -1 with the
// error set.  Whether the row moves in 16-byte pieces (`vec`) stays with the caller, who knows its pointers:
// (C * bytes) % 16 == 0 && aligned_to(each of them, 16).
inline int float_row_elem(int dtype, int C) {
  SPX_CHECK(dtype == SPX_F32 || dtype == SPX_F16 || dtype == SPX_BF16 || dtype == SPX_F64,
            "dtype must be f32, f16, bf16 or f64, got %d", dtype);
  SPX_CHECK(C >= 1, "channel count must be >= 1, got %d", C);
  SPX_CHECK(static_cast<long long>(C) * elem_bytes(dtype) <= 0x7fffffffLL, "row too long");
  return elem_bytes(dtype);
}

// From a runtime value to a compile-time one: f(std::integral_constant<int, v>) for the one of VS that equals v.  Only
// the listed values are instantiated.
template <int... VS, typename F> void dispatch_value(int v, F &&f) {
  ((v == VS ? f(std::integral_constant<int, VS>{}) : void()), ...);
}

// From (dtype, vec) to a kernel instance: f(dt, v) with dt one of DTS and v = the elements of a 16-byte piece of that
// dtype (vec) or 1.  A call site names its kernel once: kernel<dt, v>.
template <int... DTS, typename F> void dispatch_row_of(int dtype, bool vec, F &&f) {
  dispatch_value<DTS...>(dtype, [&](auto dt) {
    constexpr int V = 16 / static_cast<int>(sizeof(typename Elem<dt>::S));
    if (vec) f(dt, std::integral_constant<int, V>{});
    else f(dt, std::integral_constant<int, 1>{});
  });
}
template <typename F> void dispatch_row(int dtype, bool vec, F &&f) {
  dispatch_row_of<SPX_F32, SPX_F16, SPX_BF16, SPX_F64>(dtype, vec, f);
}

// log2 of the lanes that share a row: the power of two covering its pieces, at most a wave
inline int group_shift(int pieces) {
  int gshift = 0;
  while (gshift < 6 && (1 << gshift) < pieces) ++gshift;
  return gshift;
}

// bits of the radix sort's keys 0 .. max_key
inline int key_bits(uint32_t max_key) {
  int nbits = 1;
  while (nbits < 32 && (max_key >> nbits) != 0) ++nbits;
  return nbits;
}

}  // namespace
}  // namespace spx
