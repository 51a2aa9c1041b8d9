// Feature rows as PIECES: the storage / accumulator types of the four floating dtypes, the 16-byte (or one-element)
// piece a lane moves, and the host helpers that pick a piece width and a grid for a streaming launch.  Shared by the
// translation units that merge, reduce or score rows (union.hip, collapse.hip, select.hip); every definition has internal
// linkage.
#pragma once
#include <initializer_list>

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

}  // namespace
}  // namespace spx
