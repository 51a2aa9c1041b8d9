// A LEVEL and its RANK MAP ("outputs numbered by KEY RANK"): the level's geometry and the linear key of an index row;
// the map's layout in the caller's buffer, the lookup, and the numbering that builds it from a byte-per-cell occupancy
// map (prefix pass + totals scan, with the head of the scratch it needs).  Shared by the translation units that build
// or read one (rulebook_sorted.hip, rulebook_subm.hip, voxelize.hip, union.hip, collapse.hip, select.hip, and through
// lookup.h interp.hip and query.hip); every definition has internal linkage.
#pragma once
#include "common.h"
#include "scan.h"

namespace spx {
namespace {
// A level: batch x grid, the extents in index-column order (unused axes are 1).
struct LevelGeom {
  int ndim, batch;
  int dims[kMaxNdim];
  LevelGeom() = default;
  LevelGeom(int ndim_, int batch_, const int *spatial_h) : ndim(ndim_), batch(batch_) {
    for (int d = 0; d < kMaxNdim; ++d) dims[d] = d < ndim ? spatial_h[d] : 1;
  }
};

// The index row r = {batch index, coordinates} against the level: -1 when the batch index or ANY coordinate -- one
// that does not enter the key included -- is outside its extent; otherwise, KEYED, the linear key over the axes whose
// bit is set in `axes` (batch-major, the last of them fastest), and 0 when only the range checks are asked for.
// Whether the row is live at all (n_live) is the caller's to test.
template <bool KEYED>
__device__ __forceinline__ long long level_row(const int32_t *__restrict__ r, const LevelGeom &g, unsigned axes) {
  const int b = r[0];
  if (static_cast<unsigned>(b) >= static_cast<unsigned>(g.batch)) return -1;
  long long key = KEYED ? b : 0;
  for (int d = 0; d < g.ndim; ++d) {
    const int v = r[1 + d];
    if (static_cast<unsigned>(v) >= static_cast<unsigned>(g.dims[d])) return -1;
    if (KEYED && ((axes >> d) & 1u)) key = key * g.dims[d] + v;
  }
  return key;
}
constexpr unsigned kAllAxes = (1u << kMaxNdim) - 1u;

// the linear key of a row, -1 for one outside the level
__device__ __forceinline__ long long level_key(const int32_t *__restrict__ r, const LevelGeom &g, unsigned axes) {
  return level_row<true>(r, g, axes);
}

// the range checks alone, for a grid that need not fit a key
__device__ __forceinline__ bool level_holds(const int32_t *__restrict__ r, const LevelGeom &g) {
  return level_row<false>(r, g, 0u) == 0;
}

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

// ------------------------------------------------------------ numbering a level from its byte map
// head of the scratch of a numbering: the byte-per-cell map (32 bytes per word) and the prefix pass's block totals
struct RankScratch {
  uint8_t *occupied;
  int32_t *blockcount;
  int nblk;
  void carve(Carver &c, size_t W) {
    nblk = static_cast<int>(rank_blocks(W));
    occupied = c.take<uint8_t>(W * 32);
    blockcount = c.take<int32_t>(nblk > 0 ? nblk : 1);
  }
};

// Exclusive scan of the prefix pass's block totals by one block (block_scan_loop of scan.h); counters[0] = the cells
// found, counters[2] = the live output rows = min(found, cap) (cap < 0: no bound).
__global__ void __launch_bounds__(kScanThreads)
rank_totals_kernel(const int32_t *__restrict__ cnt, int32_t *__restrict__ off, int len, int cap,
                   int32_t *__restrict__ counters) {
  __shared__ int lds_wave[kScanThreads / 64];
  const int carry = block_scan_loop(cnt, off, len, lds_wave);
  if (threadIdx.x == 0) {
    counters[0] = carry;
    counters[2] = cap >= 0 && carry > cap ? cap : carry;
  }
}

// prefix pass + totals scan over a marked byte map: the rank map of the level, its size in counters[0] / [2]
hipError_t number_level(const RankScratch &w, size_t W, void *rankmap, int cap, int32_t *counters, hipStream_t s) {
  hipLaunchKernelGGL(conv4_prefix_kernel, dim3(w.nblk), dim3(kRankThreads), 0, s,
                     reinterpret_cast<const uint4 *>(w.occupied), static_cast<uint2 *>(rankmap),
                     static_cast<unsigned>(W), w.blockcount);
  hipLaunchKernelGGL(rank_totals_kernel, dim3(1), dim3(kScanThreads), 0, s, w.blockcount, rank_blockoff(rankmap, W), w.nblk,
                     cap, counters);
  return hipGetLastError();
}
}  // namespace
}  // namespace spx
