// The RANK MAP of a level (rulebook_sorted.hip, "outputs numbered by KEY RANK"; rulebook_subm.hip; union.hip;
// collapse.hip): its layout in the caller's buffer,
// the prefix pass that builds it from a byte-per-cell occupancy map, and the lookup.  Shared by the translation units
// that build or read one; every definition has internal linkage.
#pragma once
#include "common.h"

namespace spx {
namespace {
constexpr int kRankThreads = 256;     // threads of a prefix-pass workgroup
constexpr int kRankWords = 2048;      // words (65536 cells) per prefix block
constexpr int kRankPer = kRankWords / kRankThreads;

// the byte map packed into the words of the rank map (cells[w].x), block-local exclusive prefix of their popcounts
// (cells[w].y), block total -> blockcount.  32 bytes (two 16-byte loads) per word; a byte is 0 or 1, so four of them
// become a nibble with one multiply: ((v * 0x01020408) >> 24) & 15.
__device__ __forceinline__ uint32_t pack_flags16(const uint4 &v) {
  auto nib = [](uint32_t d) __attribute__((always_inline)) { return ((d * 0x01020408u) >> 24) & 15u; };
  return nib(v.x) | (nib(v.y) << 4) | (nib(v.z) << 8) | (nib(v.w) << 12);
}

__global__ void __launch_bounds__(kRankThreads)
conv4_prefix_kernel(const uint4 *__restrict__ occupied, uint2 *__restrict__ cells, unsigned W,
                    int32_t *__restrict__ blockcount) {
  __shared__ int lds_wave[kRankThreads / 64];
  __shared__ __attribute__((aligned(16))) uint16_t lds_half[2 * kRankWords];
  const unsigned base = blockIdx.x * kRankWords + threadIdx.x * kRankPer;
  // The block's 64 KB of flag bytes in 16-byte pieces, lane-consecutive (a thread reading ITS eight words' 256 bytes put
  // every load instruction on 64 different lines: 27 us for the 59 MB of a 47 M-cell level); a piece becomes 16 bits,
  // the halves of a word meet in LDS
  {
    const size_t piece0 = static_cast<size_t>(blockIdx.x) * (2 * kRankWords);
    const size_t pieces = 2 * static_cast<size_t>(W);
    uint4 v[2 * kRankPer];
#pragma unroll
    for (int j = 0; j < 2 * kRankPer; ++j) {
      const size_t pc = piece0 + static_cast<size_t>(j) * kRankThreads + threadIdx.x;
      v[j] = pc < pieces ? occupied[pc] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int j = 0; j < 2 * kRankPer; ++j) lds_half[j * kRankThreads + threadIdx.x] = static_cast<uint16_t>(pack_flags16(v[j]));
  }
  __syncthreads();
  uint32_t bits[kRankPer];
  int cnt[kRankPer], sum = 0;
  {
    const uint4 *w4 = reinterpret_cast<const uint4 *>(lds_half) + threadIdx.x * (kRankPer / 4);
    static_assert(kRankPer == 8, "two 16-byte reads per thread");
    const uint4 a = w4[0], b = w4[1];
    const uint32_t w[kRankPer] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int e = 0; e < kRankPer; ++e) {
      bits[e] = base + e < W ? w[e] : 0u;
      cnt[e] = __popc(bits[e]);
      sum += cnt[e];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(incl, d, 64);
    if (lane >= d) incl += u;
  }
  if (lane == 63) lds_wave[wave] = incl;
  __syncthreads();
  int prefix = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kRankThreads / 64; ++w) {
    const int x = lds_wave[w];
    if (w < wave) prefix += x;
    total += x;
  }
  int run = prefix + incl - sum;
#pragma unroll
  for (int e = 0; e < kRankPer; ++e) {
    if (base + e < W) cells[base + e] = make_uint2(bits[e], static_cast<uint32_t>(run));
    run += cnt[e];
  }
  if (threadIdx.x == 0) blockcount[blockIdx.x] = total;
}

// row of a key: occupied cells before its 65536-cell block + before its word inside the block + below it in the word
__device__ __forceinline__ int rank_of(const uint2 *__restrict__ cells, const int32_t *__restrict__ blockoff,
                                       unsigned long long key) {
  const uint2 cell = cells[key >> 5];
  const uint32_t bit = 1u << (key & 31);
  return (cell.x & bit) ? blockoff[key >> 16] + static_cast<int>(cell.y) + __popc(cell.x & (bit - 1u)) : -1;
}

// words of a level's rank map (0: the key space does not fit)
size_t rank_words(int ndim, int batch_size, const int *shape) {
  if (ndim < 1 || ndim > kMaxNdim || batch_size < 1) return 0;
  unsigned long long cells = static_cast<unsigned long long>(batch_size);
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] < 1) return 0;
    cells *= static_cast<unsigned long long>(shape[i]);
    if (cells > 0x7fffffe0ull) return 0;
  }
  return static_cast<size_t>((cells + 31) / 32);
}

// the caller's rank-map buffer: W {bits, prefix} words, then the occupied cells before each 2048-word block
size_t rank_cells_bytes(size_t W) { return align_up(W * sizeof(uint2), 256); }
size_t rank_blocks(size_t W) { return (W + kRankWords - 1) / kRankWords; }
size_t rank_bytes(size_t W) { return W ? rank_cells_bytes(W) + align_up(rank_blocks(W) * sizeof(int32_t), 256) : 0; }
int32_t *rank_blockoff(void *rankmap, size_t W) {
  return reinterpret_cast<int32_t *>(static_cast<char *>(rankmap) + rank_cells_bytes(W));
}
}  // namespace
}  // namespace spx
