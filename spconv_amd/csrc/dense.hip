// Sparse <-> dense conversion (spx_dense_map, spx_to_dense, spx_dense_gather, spx_from_dense_*).
//
// Replaces the torch composites behind SparseConvTensor.dense() / from_dense (reference spconv/pytorch/core.py
// scatter_nd, dense, from_dense): an index_put over a zero-filled tensor + permute().contiguous(), and to_sparse.
//
// Everything goes through the CELL MAP: map[cell] = the row that owns the cell (or -1), cell = batch * S + linear
// spatial index, S = prod(spatial).  The kernels move bytes: they are instantiated per element size (1, 2, 4, 8), not
// per dtype; every offset into the dense tensor is 64-bit.
//
//   map      fill with -1, one pass over the index rows: atomicMax(map + cell, row).  Dead rows (batch < 0, >= B),
//            rows with a coordinate outside the grid and rows >= *n_live are skipped; of several rows with one
//            coordinate the HIGHEST row number owns the cell (deterministic).
//   scatter  driven by the OUTPUT: every element of the dense tensor is written exactly once, a feature value or
//            the fill value; no zero-fill pass, no atomics.
//            channels-last   one row copy (or fill row) per cell, in the widest pieces the row allows
//            channels-first  a workgroup owns kTS = 256 consecutive cells of one batch item x 64 bytes of channels.
//                            Thread t owns cell t: it loads its row's 64 bytes as 16-byte pieces and writes the
//                            elements into the LDS tile lds[channel][shift(channel) + t] -- the 64 lanes of a wave write
//                            consecutive addresses of one LDS row (no bank conflict).  shift(channel) is the
//                            misalignment (in elements) of that channel's run in the OUTPUT against 16 bytes, so the
//                            store side reads whole 16-byte LDS slots (rows are (256 + 16 / E) elements long, a
//                            multiple of 16 bytes; consecutive lanes read consecutive slots: conflict-free
//                            ds_read_b128) and stores them to 16-byte aligned addresses along the cell axis; the
//                            pieces at the two ends of a run fall back to element stores.  Nothing assumes that
//                            c * S is aligned: an odd innermost extent only moves the shift.
//                            A tile without a live cell writes its fill value from registers and never touches LDS.
//   gather   the same tile walk backwards (dense -> rows): tiles without a live cell are skipped after a ballot on the
//            map and read nothing; the rows are cleared first, so rows that own no cell come out as zeros.
//   compact  from_dense: pass 1 flags the cells with a non-zero channel (to_sparse semantics: -0.0 is zero, NaN is
//            not) and counts them per 256-cell block (block_rank of scan.h), one block scans the
//            counts (scan_kernel of scan.h); the total is read back once; pass 2 writes the coordinates in ascending cell order, the rows,
//            and the cell map of the result.
#include "common.h"
#include "scan.h"

namespace spx {
namespace {

constexpr int kBlock = 256;
static_assert(kBlock == kScanThreads, "scan.h's primitives are written for this unit's workgroup size");
constexpr int kTS = 256;          // cells of a channels-first tile
constexpr int kChunkBytes = 64;   // bytes of channels of a channels-first tile

struct DenseGeom {
  int ndim, batch;
  int dims[kMaxNdim];
  long long S;       // cells of one batch item
  long long cells;   // batch * S
};

// 0 = ok; fills g.  cells must fit int32 (the map holds row numbers per cell and is indexed with int32 elsewhere).
int make_dense_geom(int ndim, int batch, const int *spatial_h, DenseGeom &g) {
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  SPX_CHECK(spatial_h != nullptr, "spatial shape is NULL");
  SPX_CHECK(batch >= 0, "negative batch size");
  g.ndim = ndim;
  g.batch = batch;
  g.S = 1;
  for (int i = 0; i < kMaxNdim; ++i) g.dims[i] = 1;
  for (int i = 0; i < ndim; ++i) {
    SPX_CHECK(spatial_h[i] >= 0, "negative spatial extent");
    g.dims[i] = spatial_h[i];
    g.S *= spatial_h[i];
    SPX_CHECK(g.S <= 0x7fffffffLL, "dense grid of more than 2^31 - 1 cells");
  }
  g.cells = g.S * batch;
  SPX_CHECK(g.cells <= 0x7fffffffLL, "dense grid of more than 2^31 - 1 cells (batch %d x %lld)", batch, g.S);
  return 0;
}

template <int E> struct UInt;
template <> struct UInt<1> { using type = uint8_t; };
template <> struct UInt<2> { using type = uint16_t; };
template <> struct UInt<4> { using type = uint32_t; };
template <> struct UInt<8> { using type = unsigned long long; };
template <> struct UInt<16> { using type = uint4; };

// the fill value as a V-byte piece: fill8 holds the element's bit pattern repeated over 8 bytes
template <typename T> __device__ __forceinline__ T fill_piece(unsigned long long fill8) { return static_cast<T>(fill8); }
template <> __device__ __forceinline__ uint4 fill_piece<uint4>(unsigned long long fill8) {
  const uint32_t lo = static_cast<uint32_t>(fill8), hi = static_cast<uint32_t>(fill8 >> 32);
  return make_uint4(lo, hi, lo, hi);
}

// -------------------------------------------------------------------------------------------- cell map

// p[0 .. words) = v: the -1 fill of the map and the clear of the gather's rows.  A kernel of this file rather than
// a runtime memset, so that a captured pass consists of kernel nodes only.
__global__ void __launch_bounds__(kBlock)
fill_words_kernel(uint32_t *__restrict__ p, long long words, uint32_t v) {
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < words;
       i += static_cast<long long>(gridDim.x) * kBlock)
    p[i] = v;
}

// the same for a byte range that is not a whole number of aligned words
__global__ void __launch_bounds__(kBlock)
fill_bytes_kernel(uint8_t *__restrict__ p, long long bytes, uint8_t v) {
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < bytes;
       i += static_cast<long long>(gridDim.x) * kBlock)
    p[i] = v;
}

__global__ void __launch_bounds__(kBlock)
dense_map_kernel(const int32_t *__restrict__ indices, int n, const int32_t *__restrict__ n_live, DenseGeom g,
                 int32_t *__restrict__ map) {
  const int row = blockIdx.x * kBlock + threadIdx.x;
  if (row >= n) return;
  if (n_live && row >= *n_live) return;
  const int32_t *r = indices + static_cast<size_t>(row) * (g.ndim + 1);
  const int b = r[0];
  if (static_cast<unsigned>(b) >= static_cast<unsigned>(g.batch)) return;
  long long cell = b;
  for (int d = 0; d < g.ndim; ++d) {
    const int v = r[1 + d];
    if (static_cast<unsigned>(v) >= static_cast<unsigned>(g.dims[d])) return;
    cell = cell * g.dims[d] + v;
  }
  atomicMax(map + cell, row);
}

// -------------------------------------------------------------------------------------------- channels-last

// out[cell] = rows[map[cell]] or the fill row, in pieces of sizeof(T) bytes; ld = row stride of `rows` in pieces
template <typename T>
__global__ void __launch_bounds__(kBlock)
scatter_cl_kernel(const T *__restrict__ rows, long long ld, const int32_t *__restrict__ map, T *__restrict__ out,
                  int pieces, long long total, unsigned long long fill8, int n) {
  const T fill = fill_piece<T>(fill8);
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < total;
       i += static_cast<long long>(gridDim.x) * kBlock) {
    const long long cell = i / pieces;
    const int p = static_cast<int>(i - cell * pieces);
    const int r = map[cell];
    T v = fill;
    if (static_cast<unsigned>(r) < static_cast<unsigned>(n)) v = rows[r * ld + p];     // (a map entry is checked, not trusted)
    out[i] = v;
  }
}

// rows[map[cell]] = dense[cell] for the cells that have an owner (rows cleared beforehand)
template <typename T>
__global__ void __launch_bounds__(kBlock)
gather_cl_kernel(const T *__restrict__ dense, const int32_t *__restrict__ map, T *__restrict__ rows, int pieces,
                 long long total, int n) {
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < total;
       i += static_cast<long long>(gridDim.x) * kBlock) {
    const long long cell = i / pieces;
    const int p = static_cast<int>(i - cell * pieces);
    const int r = map[cell];
    if (static_cast<unsigned>(r) < static_cast<unsigned>(n)) rows[static_cast<long long>(r) * pieces + p] = dense[i];
  }
}

// -------------------------------------------------------------------------------------------- channels-first

template <int E> struct Tile {
  using T = typename UInt<E>::type;
  static constexpr int PV = 16 / E;                 // elements of a 16-byte piece
  static constexpr int TC = kChunkBytes / E;        // channels of a tile
  static constexpr int PIECES = kChunkBytes / 16;   // 16-byte pieces of a cell's chunk
  static constexpr int LD = kTS + PV;               // elements of an LDS row: one slot of room for the shift
  static constexpr int NP = kTS / PV + 1;           // 16-byte slots of an LDS row
  union Piece {
    uint4 v;
    T e[PV];
  };
};

// Where a tile lies: batch item b, cells [s0, s0 + valid) of it, channels [c0, c0 + nc)
struct TilePos {
  long long b, s0;
  int valid, c0, nc;
};

__device__ __forceinline__ TilePos tile_pos(long long S, int C, int TC) {
  const long long tiles = (S + kTS - 1) / kTS;
  TilePos p;
  p.b = blockIdx.x / tiles;
  p.s0 = (blockIdx.x - p.b * tiles) * kTS;
  p.valid = static_cast<int>(S - p.s0 < kTS ? S - p.s0 : kTS);
  p.c0 = blockIdx.y * TC;
  p.nc = C - p.c0 < TC ? C - p.c0 : TC;
  return p;
}

template <int E>
__global__ void __launch_bounds__(kBlock)
scatter_cf_kernel(const typename UInt<E>::type *__restrict__ rows, long long ld, int rows_vec,
                  const int32_t *__restrict__ map, typename UInt<E>::type *__restrict__ out, int C, long long S,
                  unsigned long long fill8, int n) {
  using TL = Tile<E>;
  using T = typename TL::T;
  __shared__ __attribute__((aligned(16))) T lds[TL::TC][TL::LD];
  __shared__ int shift[TL::TC];
  const TilePos tp = tile_pos(S, C, TL::TC);
  const int t = threadIdx.x;
  // element index of channel c's run in the output, and its misalignment against 16 bytes (in elements)
  auto run_of = [&](int c) { return (tp.b * C + tp.c0 + c) * S + tp.s0; };
  if (t < tp.nc)
    shift[t] = static_cast<int>((reinterpret_cast<uintptr_t>(out + run_of(t)) & 15) / E);
  int r = t < tp.valid ? map[tp.b * S + tp.s0 + t] : -1;
  if (static_cast<unsigned>(r) >= static_cast<unsigned>(n)) r = -1;      // (a map entry is checked, not trusted)
  const bool live = __syncthreads_or(r >= 0) != 0;      // (also publishes shift[])
  const T fill = static_cast<T>(fill8);
  if (live) {
    // load side: thread t owns cell t
    if (t < tp.valid) {
      const T *src = r >= 0 ? rows + r * ld + tp.c0 : nullptr;
#pragma unroll
      for (int q = 0; q < TL::PIECES; ++q) {
        const int cq = q * TL::PV;
        if (cq >= tp.nc) break;
        typename TL::Piece pc;
        if (!src) {
#pragma unroll
          for (int j = 0; j < TL::PV; ++j) pc.e[j] = fill;
        } else if (rows_vec && cq + TL::PV <= tp.nc) {
          pc.v = *reinterpret_cast<const uint4 *>(src + cq);
        } else {
#pragma unroll
          for (int j = 0; j < TL::PV; ++j) pc.e[j] = cq + j < tp.nc ? src[cq + j] : fill;
        }
#pragma unroll
        for (int j = 0; j < TL::PV; ++j)
          if (cq + j < tp.nc) lds[cq + j][shift[cq + j] + t] = pc.e[j];
      }
    }
    __syncthreads();
  }
  // store side: 16-byte aligned slots along the cell axis
  for (int id = t; id < tp.nc * TL::NP; id += kBlock) {
    const int c = id / TL::NP, p = id - c * TL::NP;
    const int e_lo = p * TL::PV - shift[c];           // first element of the slot, relative to the run
    if (e_lo >= tp.valid || e_lo + TL::PV <= 0) continue;
    T *dst = out + run_of(c) + e_lo;
    typename TL::Piece pc;
    if (live) {
      pc.v = *reinterpret_cast<const uint4 *>(&lds[c][p * TL::PV]);
    } else {
#pragma unroll
      for (int j = 0; j < TL::PV; ++j) pc.e[j] = fill;
    }
    if (e_lo >= 0 && e_lo + TL::PV <= tp.valid) {
      *reinterpret_cast<uint4 *>(dst) = pc.v;
    } else {
#pragma unroll
      for (int j = 0; j < TL::PV; ++j)
        if (e_lo + j >= 0 && e_lo + j < tp.valid) dst[j] = pc.e[j];
    }
  }
}

template <int E>
__global__ void __launch_bounds__(kBlock)
gather_cf_kernel(const typename UInt<E>::type *__restrict__ dense, const int32_t *__restrict__ map,
                 typename UInt<E>::type *__restrict__ rows, int rows_vec, int C, long long S, int n) {
  using TL = Tile<E>;
  using T = typename TL::T;
  __shared__ __attribute__((aligned(16))) T lds[TL::TC][TL::LD];
  __shared__ int shift[TL::TC];
  const TilePos tp = tile_pos(S, C, TL::TC);
  const int t = threadIdx.x;
  auto run_of = [&](int c) { return (tp.b * C + tp.c0 + c) * S + tp.s0; };
  if (t < tp.nc)
    shift[t] = static_cast<int>((reinterpret_cast<uintptr_t>(dense + run_of(t)) & 15) / E);
  int r = t < tp.valid ? map[tp.b * S + tp.s0 + t] : -1;
  if (static_cast<unsigned>(r) >= static_cast<unsigned>(n)) r = -1;
  if (!__syncthreads_or(r >= 0)) return;                // no live cell: nothing is read
  for (int id = t; id < tp.nc * TL::NP; id += kBlock) {
    const int c = id / TL::NP, p = id - c * TL::NP;
    const int e_lo = p * TL::PV - shift[c];
    if (e_lo >= tp.valid || e_lo + TL::PV <= 0) continue;
    const T *src = dense + run_of(c) + e_lo;
    if (e_lo >= 0 && e_lo + TL::PV <= tp.valid) {
      *reinterpret_cast<uint4 *>(&lds[c][p * TL::PV]) = *reinterpret_cast<const uint4 *>(src);
    } else {
#pragma unroll
      for (int j = 0; j < TL::PV; ++j)
        if (e_lo + j >= 0 && e_lo + j < tp.valid) lds[c][p * TL::PV + j] = src[j];
    }
  }
  __syncthreads();
  if (r < 0) return;
  T *dst = rows + static_cast<long long>(r) * C + tp.c0;
#pragma unroll
  for (int q = 0; q < TL::PIECES; ++q) {
    const int cq = q * TL::PV;
    if (cq >= tp.nc) break;
    typename TL::Piece pc;
#pragma unroll
    for (int j = 0; j < TL::PV; ++j)
      if (cq + j < tp.nc) pc.e[j] = lds[cq + j][shift[cq + j] + t];
    if (rows_vec && cq + TL::PV <= tp.nc) {
      *reinterpret_cast<uint4 *>(dst + cq) = pc.v;
    } else {
#pragma unroll
      for (int j = 0; j < TL::PV; ++j)
        if (cq + j < tp.nc) dst[cq + j] = pc.e[j];
    }
  }
}

// -------------------------------------------------------------------------------------------- compaction

template <typename T> __device__ __forceinline__ bool piece_nonzero(T v, unsigned long long mask8) {
  return (v & static_cast<T>(mask8)) != 0;
}
template <> __device__ __forceinline__ bool piece_nonzero<uint4>(uint4 v, unsigned long long mask8) {
  const uint32_t lo = static_cast<uint32_t>(mask8), hi = static_cast<uint32_t>(mask8 >> 32);
  return ((v.x & lo) | (v.y & hi) | (v.z & lo) | (v.w & hi)) != 0;
}

// Pass 1.  A block owns kBlock consecutive cells = one contiguous stretch of the channels-last tensor, read in pieces
// of sizeof(T) bytes.  mask8: the bits of an element that make it non-zero (floats: everything but the sign),
// repeated over 8 bytes.  flags[cell] = 1 / 0, blockcount[block] = active cells of the block.
template <typename T>
__global__ void __launch_bounds__(kBlock)
compact_flag_kernel(const T *__restrict__ dense, int pieces, long long cells, unsigned long long mask8,
                    int32_t *__restrict__ flags, int32_t *__restrict__ blockcount) {
  __shared__ int active[kBlock];
  __shared__ int lds_wave[kBlock / 64];
  const long long cell0 = static_cast<long long>(blockIdx.x) * kBlock;
  const int ncell = static_cast<int>(cells - cell0 < kBlock ? cells - cell0 : kBlock);
  active[threadIdx.x] = 0;
  __syncthreads();
  const T *src = dense + cell0 * pieces;
  const long long total = static_cast<long long>(ncell) * pieces;
  for (long long i = threadIdx.x; i < total; i += kBlock)
    if (piece_nonzero<T>(src[i], mask8)) active[i / pieces] = 1;     // (racing writers store the same value)
  __syncthreads();
  const bool on = threadIdx.x < ncell && active[threadIdx.x] != 0;
  if (threadIdx.x < ncell) flags[cell0 + threadIdx.x] = on ? 1 : 0;
  int count;
  block_rank(on, count, lds_wave);
  if (threadIdx.x == 0) blockcount[blockIdx.x] = count;
}

// Pass 2: coordinates (ascending cell order), rows, and the cell map of the result.
template <typename T>
__global__ void __launch_bounds__(kBlock)
compact_fill_kernel(const T *__restrict__ dense, int pieces, DenseGeom g, const int32_t *__restrict__ flags,
                    const int32_t *__restrict__ blockoff, int32_t *__restrict__ indices, T *__restrict__ rows,
                    int32_t *__restrict__ map) {
  __shared__ int rank_of[kBlock];
  __shared__ int lds_wave[kBlock / 64];
  const long long cell0 = static_cast<long long>(blockIdx.x) * kBlock;
  const int ncell = static_cast<int>(g.cells - cell0 < kBlock ? g.cells - cell0 : kBlock);
  const long long cell = cell0 + threadIdx.x;
  const bool on = threadIdx.x < ncell && flags[cell] != 0;
  int count;
  const int rank = blockoff[blockIdx.x] + block_rank(on, count, lds_wave);
  rank_of[threadIdx.x] = on ? rank : -1;
  if (threadIdx.x < ncell && map) map[cell] = on ? rank : -1;
  if (on) {
    int32_t *o = indices + static_cast<long long>(rank) * (g.ndim + 1);
    long long rest = cell;
    for (int d = g.ndim - 1; d >= 0; --d) {
      o[1 + d] = static_cast<int32_t>(rest % g.dims[d]);
      rest /= g.dims[d];
    }
    o[0] = static_cast<int32_t>(rest);
  }
  __syncthreads();
  if (count == 0) return;
  const T *src = dense + cell0 * pieces;
  const long long total = static_cast<long long>(ncell) * pieces;
  for (long long i = threadIdx.x; i < total; i += kBlock) {
    const int cl = static_cast<int>(i / pieces);
    const int r = rank_of[cl];
    if (r >= 0) rows[static_cast<long long>(r) * pieces + (i - static_cast<long long>(cl) * pieces)] = src[i];
  }
}

// -------------------------------------------------------------------------------------------- host side

inline bool aligned_to(const void *p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// widest piece (16 bytes down to one element) that divides every byte count of `strides` and the alignment of every pointer
int piece_bytes(int elem_bytes, std::initializer_list<long long> strides, std::initializer_list<const void *> ptrs) {
  int v = 16;
  for (; v > elem_bytes; v >>= 1) {
    bool ok = true;
    for (long long s : strides) ok = ok && s % v == 0;
    for (const void *p : ptrs) ok = ok && (p == nullptr || aligned_to(p, v));
    if (ok) break;
  }
  return v;
}

unsigned long long repeat8(unsigned long long bits, int elem_bytes) {
  if (elem_bytes >= 8) return bits;
  bits &= (1ull << (8 * elem_bytes)) - 1;
  unsigned long long r = 0;
  for (int i = 0; i < 8; i += elem_bytes) r |= bits << (8 * i);
  return r;
}

inline bool elem_ok(int e) { return e == 1 || e == 2 || e == 4 || e == 8; }

inline unsigned stream_blocks(long long total) {
  const long long b = (total + kBlock - 1) / kBlock;
  return static_cast<unsigned>(b < (1 << 20) ? b : (1 << 20));     // (grid-stride loops beyond 2^28 pieces)
}

// p[0 .. bytes) = byte v, as words where the range allows
void launch_fill(void *p, long long bytes, uint8_t v, hipStream_t s) {
  if (bytes <= 0) return;
  if (aligned_to(p, 4) && bytes % 4 == 0)
    hipLaunchKernelGGL(fill_words_kernel, dim3(stream_blocks(bytes / 4)), dim3(kBlock), 0, s, static_cast<uint32_t *>(p),
                       bytes / 4, 0x01010101u * v);
  else
    hipLaunchKernelGGL(fill_bytes_kernel, dim3(stream_blocks(bytes)), dim3(kBlock), 0, s, static_cast<uint8_t *>(p), bytes, v);
}

template <typename T>
void launch_scatter_cl(const void *rows, long long ld_bytes, const int32_t *map, void *out, int row_bytes,
                       long long cells, unsigned long long fill8, int n, hipStream_t s) {
  const int pieces = row_bytes / static_cast<int>(sizeof(T));
  const long long total = cells * pieces;
  hipLaunchKernelGGL(scatter_cl_kernel<T>, dim3(stream_blocks(total)), dim3(kBlock), 0, s, static_cast<const T *>(rows),
                     ld_bytes / static_cast<long long>(sizeof(T)), map, static_cast<T *>(out), pieces, total, fill8, n);
}

template <typename T>
void launch_gather_cl(const void *dense, const int32_t *map, void *rows, int row_bytes, long long cells, int n,
                      hipStream_t s) {
  const int pieces = row_bytes / static_cast<int>(sizeof(T));
  const long long total = cells * pieces;
  hipLaunchKernelGGL(gather_cl_kernel<T>, dim3(stream_blocks(total)), dim3(kBlock), 0, s, static_cast<const T *>(dense), map,
                     static_cast<T *>(rows), pieces, total, n);
}

template <int E>
void launch_scatter_cf(const void *rows, long long ld, int rows_vec, const int32_t *map, void *out, int C,
                       const DenseGeom &g, unsigned long long fill8, int n, hipStream_t s) {
  using T = typename UInt<E>::type;
  const long long tiles = (g.S + kTS - 1) / kTS * g.batch;
  hipLaunchKernelGGL(scatter_cf_kernel<E>, dim3(static_cast<unsigned>(tiles), div_up(C, Tile<E>::TC)), dim3(kBlock), 0, s,
                     static_cast<const T *>(rows), ld, rows_vec, map, static_cast<T *>(out), C, g.S, fill8, n);
}

template <int E>
void launch_gather_cf(const void *dense, const int32_t *map, void *rows, int rows_vec, int C, const DenseGeom &g,
                      int n, hipStream_t s) {
  using T = typename UInt<E>::type;
  const long long tiles = (g.S + kTS - 1) / kTS * g.batch;
  hipLaunchKernelGGL(gather_cf_kernel<E>, dim3(static_cast<unsigned>(tiles), div_up(C, Tile<E>::TC)), dim3(kBlock), 0, s,
                     static_cast<const T *>(dense), map, static_cast<T *>(rows), rows_vec, C, g.S, n);
}

// scratch of the compaction: flags [cells], blockcount / blockoff [nblk], total [1]
struct CompactWs {
  int32_t *flags, *blockcount, *blockoff, *total;
  int nblk;
  size_t bytes;
  CompactWs(void *ws, long long cells) {
    Carver c(ws);
    nblk = static_cast<int>((cells + kBlock - 1) / kBlock);
    flags = c.take<int32_t>(static_cast<size_t>(cells));
    blockcount = c.take<int32_t>(nblk);
    blockoff = c.take<int32_t>(nblk);
    total = c.take<int32_t>(1);
    bytes = c.off;
  }
};

}  // namespace
}  // namespace spx

#define SPX_BY_PIECE(v, call_)                                 \
  switch (v) {                                                 \
    case 16: { using P = uint4; call_; break; }                \
    case 8: { using P = unsigned long long; call_; break; }    \
    case 4: { using P = uint32_t; call_; break; }              \
    case 2: { using P = uint16_t; call_; break; }              \
    default: { using P = uint8_t; call_; break; }              \
  }

extern "C" {

size_t spx_dense_ws_bytes(int ndim, int batch, const int *spatial_h) {
  spx::DenseGeom g;
  if (spx::make_dense_geom(ndim, batch, spatial_h, g) != 0) return 0;
  return spx::align_up(static_cast<size_t>(g.cells) * sizeof(int32_t), 256);
}

int spx_dense_map(const int32_t *indices, int n, const int32_t *n_live, int ndim, int batch, const int *spatial_h,
                  int32_t *map, spx_stream_t stream) {
  spx::DenseGeom g;
  if (int rc = spx::make_dense_geom(ndim, batch, spatial_h, g)) return rc;
  SPX_CHECK(n >= 0, "negative row count");
  if (g.cells == 0) return 0;
  SPX_CHECK(map != nullptr, "map is NULL");
  SPX_CHECK(n == 0 || indices != nullptr, "indices is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  spx::launch_fill(map, g.cells * 4, 0xff, s);     // every cell: -1
  SPX_LAUNCH_CHECK();
  if (n > 0) {
    hipLaunchKernelGGL(spx::dense_map_kernel, dim3(spx::div_up(n, spx::kBlock)), dim3(spx::kBlock), 0, s, indices, n,
                       n_live, g, map);
    SPX_LAUNCH_CHECK();
  }
  spx::count(spx::kDenseMap);
  return 0;
}

int spx_to_dense(const void *rows, int n, long long row_stride, const int32_t *map, void *out, int C, int elem_bytes,
                 int channels_first, long long fill_bits, int ndim, int batch, const int *spatial_h,
                 spx_stream_t stream) {
  spx::DenseGeom g;
  if (int rc = spx::make_dense_geom(ndim, batch, spatial_h, g)) return rc;
  SPX_CHECK(spx::elem_ok(elem_bytes), "element size must be 1, 2, 4 or 8 bytes, got %d", elem_bytes);
  SPX_CHECK(n >= 0 && C >= 0 && row_stride >= C, "bad row count %d / channel count %d / row stride %lld", n, C, row_stride);
  if (g.cells == 0 || C == 0) return 0;
  SPX_CHECK(map != nullptr && out != nullptr && (n == 0 || rows != nullptr), "map / out / rows is NULL");
  SPX_CHECK(spx::aligned_to(out, elem_bytes) && spx::aligned_to(rows, elem_bytes), "pointer not aligned to its elements");
  SPX_CHECK(static_cast<long long>(C) * elem_bytes <= 0x7fffffffLL, "row too long");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned long long fill8 = spx::repeat8(static_cast<unsigned long long>(fill_bits), elem_bytes);
  const int row_bytes = C * elem_bytes;
  const long long ld_bytes = row_stride * elem_bytes;
  if (!channels_first || g.S == 1) {          // (one cell per batch item: the two layouts coincide)
    const int v = spx::piece_bytes(elem_bytes, {row_bytes, ld_bytes}, {rows, out});
    SPX_BY_PIECE(v, spx::launch_scatter_cl<P>(rows, ld_bytes, map, out, row_bytes, g.cells, fill8, n, s));
    SPX_LAUNCH_CHECK();
    spx::count(spx::kDenseScatterCl);
    return 0;
  }
  SPX_CHECK(spx::div_up(C, spx::kChunkBytes / elem_bytes) <= 65535, "too many channels: %d", C);
  const int rows_vec = ld_bytes % 16 == 0 && spx::aligned_to(rows, 16) ? 1 : 0;
  switch (elem_bytes) {
    case 1: spx::launch_scatter_cf<1>(rows, row_stride, rows_vec, map, out, C, g, fill8, n, s); break;
    case 2: spx::launch_scatter_cf<2>(rows, row_stride, rows_vec, map, out, C, g, fill8, n, s); break;
    case 4: spx::launch_scatter_cf<4>(rows, row_stride, rows_vec, map, out, C, g, fill8, n, s); break;
    default: spx::launch_scatter_cf<8>(rows, row_stride, rows_vec, map, out, C, g, fill8, n, s); break;
  }
  SPX_LAUNCH_CHECK();
  spx::count(spx::kDenseScatterCf);
  return 0;
}

int spx_dense_gather(const void *dense, const int32_t *map, void *rows, int n, int C, int elem_bytes,
                     int channels_first, int ndim, int batch, const int *spatial_h, spx_stream_t stream) {
  spx::DenseGeom g;
  if (int rc = spx::make_dense_geom(ndim, batch, spatial_h, g)) return rc;
  SPX_CHECK(spx::elem_ok(elem_bytes), "element size must be 1, 2, 4 or 8 bytes, got %d", elem_bytes);
  SPX_CHECK(n >= 0 && C >= 0, "negative size");
  if (n == 0 || C == 0) return 0;
  SPX_CHECK(rows != nullptr, "rows is NULL");
  SPX_CHECK(static_cast<long long>(C) * elem_bytes <= 0x7fffffffLL, "row too long");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int row_bytes = C * elem_bytes;
  spx::launch_fill(rows, static_cast<long long>(n) * row_bytes, 0, s);       // rows that own no cell: zeros
  SPX_LAUNCH_CHECK();
  if (g.cells == 0) return 0;
  SPX_CHECK(map != nullptr && dense != nullptr, "map / dense is NULL");
  SPX_CHECK(spx::aligned_to(dense, elem_bytes) && spx::aligned_to(rows, elem_bytes), "pointer not aligned to its elements");
  if (!channels_first || g.S == 1) {
    const int v = spx::piece_bytes(elem_bytes, {row_bytes}, {rows, dense});
    SPX_BY_PIECE(v, spx::launch_gather_cl<P>(dense, map, rows, row_bytes, g.cells, n, s));
    SPX_LAUNCH_CHECK();
    spx::count(spx::kDenseGatherCl);
    return 0;
  }
  SPX_CHECK(spx::div_up(C, spx::kChunkBytes / elem_bytes) <= 65535, "too many channels: %d", C);
  const int rows_vec = row_bytes % 16 == 0 && spx::aligned_to(rows, 16) ? 1 : 0;
  switch (elem_bytes) {
    case 1: spx::launch_gather_cf<1>(dense, map, rows, rows_vec, C, g, n, s); break;
    case 2: spx::launch_gather_cf<2>(dense, map, rows, rows_vec, C, g, n, s); break;
    case 4: spx::launch_gather_cf<4>(dense, map, rows, rows_vec, C, g, n, s); break;
    default: spx::launch_gather_cf<8>(dense, map, rows, rows_vec, C, g, n, s); break;
  }
  SPX_LAUNCH_CHECK();
  spx::count(spx::kDenseGatherCf);
  return 0;
}

size_t spx_from_dense_ws_bytes(int ndim, int batch, const int *spatial_h) {
  spx::DenseGeom g;
  if (spx::make_dense_geom(ndim, batch, spatial_h, g) != 0) return 0;
  return spx::CompactWs(nullptr, g.cells).bytes;
}

int spx_from_dense_count(const void *dense, int C, int elem_bytes, int is_float, int ndim, int batch,
                         const int *spatial_h, void *ws, size_t ws_bytes, int *n_active_h, spx_stream_t stream) {
  spx::DenseGeom g;
  if (int rc = spx::make_dense_geom(ndim, batch, spatial_h, g)) return rc;
  SPX_CHECK(spx::elem_ok(elem_bytes), "element size must be 1, 2, 4 or 8 bytes, got %d", elem_bytes);
  SPX_CHECK(n_active_h != nullptr, "n_active_h is NULL");
  SPX_CHECK(C >= 0 && static_cast<long long>(C) * elem_bytes <= 0x7fffffffLL, "bad channel count %d", C);
  *n_active_h = 0;
  if (g.cells == 0 || C == 0) return 0;
  SPX_CHECK(dense != nullptr && ws != nullptr, "dense / ws is NULL");
  SPX_CHECK(spx::aligned_to(dense, elem_bytes), "pointer not aligned to its elements");
  spx::CompactWs w(ws, g.cells);
  SPX_CHECK(ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int row_bytes = C * elem_bytes;
  const unsigned long long sign = 1ull << (8 * elem_bytes - 1);
  const unsigned long long mask8 = spx::repeat8(is_float ? ~sign : ~0ull, elem_bytes);
  const int v = spx::piece_bytes(elem_bytes, {row_bytes}, {dense});
  SPX_BY_PIECE(v, hipLaunchKernelGGL(spx::compact_flag_kernel<P>, dim3(w.nblk), dim3(spx::kBlock), 0, s,
                                     static_cast<const P *>(dense), row_bytes / static_cast<int>(sizeof(P)), g.cells,
                                     mask8, w.flags, w.blockcount));
  SPX_LAUNCH_CHECK();
  hipLaunchKernelGGL(spx::scan_kernel, dim3(1), dim3(spx::kBlock), 0, s, w.blockcount, w.blockoff, w.nblk,
                     w.total);
  SPX_LAUNCH_CHECK();
  SPX_HIP(hipMemcpyAsync(n_active_h, w.total, sizeof(int), hipMemcpyDeviceToHost, s));
  SPX_HIP(hipStreamSynchronize(s));
  spx::count(spx::kDenseCompact);
  return 0;
}

int spx_from_dense_fill(const void *dense, int C, int elem_bytes, int ndim, int batch, const int *spatial_h,
                        const void *ws, size_t ws_bytes, int32_t *indices, void *rows, int32_t *map,
                        spx_stream_t stream) {
  spx::DenseGeom g;
  if (int rc = spx::make_dense_geom(ndim, batch, spatial_h, g)) return rc;
  SPX_CHECK(spx::elem_ok(elem_bytes), "element size must be 1, 2, 4 or 8 bytes, got %d", elem_bytes);
  SPX_CHECK(C >= 0 && static_cast<long long>(C) * elem_bytes <= 0x7fffffffLL, "bad channel count %d", C);
  if (g.cells == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (C == 0) {                               // no channel, no active cell
    if (map) {
      spx::launch_fill(map, g.cells * 4, 0xff, s);
      SPX_LAUNCH_CHECK();
    }
    return 0;
  }
  SPX_CHECK(dense != nullptr && ws != nullptr, "dense / ws is NULL");
  spx::CompactWs w(const_cast<void *>(ws), g.cells);
  SPX_CHECK(ws_bytes >= w.bytes, "workspace too small: %zu < %zu", ws_bytes, w.bytes);
  const int row_bytes = C * elem_bytes;
  const int v = spx::piece_bytes(elem_bytes, {row_bytes}, {dense, rows});
  SPX_BY_PIECE(v, hipLaunchKernelGGL(spx::compact_fill_kernel<P>, dim3(w.nblk), dim3(spx::kBlock), 0, s,
                                     static_cast<const P *>(dense), row_bytes / static_cast<int>(sizeof(P)), g, w.flags,
                                     w.blockoff, indices, static_cast<P *>(rows), map));
  SPX_LAUNCH_CHECK();
  spx::count(spx::kDenseCompact);
  return 0;
}

}  // extern "C"
