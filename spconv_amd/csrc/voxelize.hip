// Point -> voxel (spx_point2voxel_ws_bytes, spx_point2voxel; spx_point2voxel_static_ws_bytes, spx_point2voxel_static).
//
// Voxeliser.  Deterministic and identical to the reference's CPU loop
// (csrc/sparse/pointops.py Point2VoxelCPU::point_to_voxel, lines 135-172 of the class): voxels
// are numbered in first-seen point order, a voxel keeps its first max_points points in point
// order, voxels past max_voxels are dropped.  Same building blocks as the rulebook: hash with
// atomicMin (first point of a voxel), count -> scan -> assign (numbering), stable radix sort by
// voxel id (slot of a point inside its voxel), no order-dependent atomics.
//
// spx_point2voxel_static is the same pipeline with nothing read back: the number of points is a device word, every
// grid depends on host-known sizes only, rows behind the voxels kept come out dead (static.py's padding contract), and
// the counts {kept, found} stay on the device, so the call can sit inside a stream capture.  key_order = 1 numbers the
// kept voxels by ascending coordinate key instead of by their first point: the first-seen numbering still decides
// WHICH voxels are kept; each of them then sets its cell's bit in the level's rank map (rankmap.h), a prefix pass over
// the map's words turns the bits into ranks and the rank of a voxel's key is its row -- no sort, and the map is what
// the SubM layers of the first level build their rulebooks from.  The mean of a voxel's stored points (the "mean VFE" feature row) is read off the sorted point
// list, so it needs neither the voxel tensor nor its empty-slot fill.
#include "common.h"
#include "rankmap.h"
#include "scan.h"
#include "table.h"

namespace spx {
namespace {

constexpr int kBlock = 256;
constexpr int kItems = 2048;  // entries per block in count/scatter passes (8 x 256)
static_assert(kBlock == kScanThreads, "scan.h's primitives are written for this unit's workgroup size");

struct P2VGeom {
  int ndim;
  int batch;       // scenes: the batch index of a point is the leading digit of its key
  float vsize[4], lo[4];
  int grid[4];
};

__device__ __forceinline__ bool p2v_coor(const float *__restrict__ pt, const P2VGeom &g, int (&c)[4]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < g.ndim) {
      // zyx order: coordinate j comes from point column ndim-1-j (pointops.py:107,138)
      const float v = floorf((pt[g.ndim - 1 - j] - g.lo[j]) / g.vsize[j]);
      const int ci = static_cast<int>(v);
      ok = ok && !(v < 0.f) && v < static_cast<float>(g.grid[j]);
      c[j] = ci;
    } else {
      c[j] = 0;
    }
  }
  return ok;
}

// Cell of point i: coordinates (zyx), batch index (0 without point_batch) and linear key (batch-major, last axis
// fastest).  False: the point is dropped (outside the range, or a batch index outside [0, batch)).
__device__ __forceinline__ bool p2v_cell(const float *__restrict__ pts, const int32_t *__restrict__ point_batch, int i,
                                         int nfeat, const P2VGeom &g, int (&c)[4], int &b, hkey_t &key) {
  b = point_batch ? point_batch[i] : 0;
  const bool ok = p2v_coor(pts + static_cast<size_t>(i) * nfeat, g, c) && b >= 0 && b < g.batch;
  key = b;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < g.ndim) key = key * g.grid[j] + c[j];
  return ok;
}

// n_dev (static form): the number of points is a device word; rows behind it are no points, whatever they hold
__global__ void __launch_bounds__(kBlock)
p2v_insert_kernel(const float *__restrict__ pts, const int32_t *__restrict__ point_batch, int n_cap,
                  const int32_t *__restrict__ n_dev, int nfeat, P2VGeom g, Table t, int32_t *__restrict__ slot_of) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_cap) return;
  const int n = n_dev ? *n_dev : n_cap;
  int c[4], b;
  hkey_t key;
  int slot = -1;
  if (i < n && p2v_cell(pts, point_batch, i, nfeat, g, c, b, key)) slot = table_insert_min(t, key, i);
  slot_of[i] = slot;
}

__global__ void __launch_bounds__(kBlock)
p2v_count_first_kernel(const int32_t *__restrict__ slot_of, Table t, int n,
                       int32_t *__restrict__ blockcount) {
  __shared__ int lds_wave[kBlock / 64];
  const int begin = blockIdx.x * kItems;
  int cnt = 0;
#pragma unroll
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    const int slot = e < n ? slot_of[e] : -1;
    cnt += __popcll(__ballot(slot >= 0 && table_val(t, slot) == e));
  }
  if ((threadIdx.x & 63) == 0) lds_wave[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < kBlock / 64; ++w) sum += lds_wave[w];
    blockcount[blockIdx.x] = sum;
  }
}

// lead = 1: index rows carry the batch index in front of zyx (the static form).  cells (key order): a kept voxel sets
// its cell's bit in the zeroed rank map instead of writing its row -- one atomicOr per VOXEL, whose result does not
// depend on the order of arrival (the level builders mark a byte per cell with plain stores: they mark 27 candidates
// per row, rulebook_sorted.hip conv4_mark_kernel; here the byte map would cost 32 x the fill and a pass over it per call);
// p2v_renumber_kernel numbers the voxel once p2v_rank_prefix_kernel has turned the bits into ranks.
__global__ void __launch_bounds__(kBlock)
p2v_assign_kernel(const float *__restrict__ pts, const int32_t *__restrict__ point_batch, int n, int nfeat, P2VGeom g,
                  const int32_t *__restrict__ slot_of, Table t,
                  const int32_t *__restrict__ blockoff, int max_voxels,
                  int32_t *__restrict__ slot_vid, int32_t *__restrict__ indices, int lead,
                  uint2 *__restrict__ cells) {
  __shared__ int lds_wave[kBlock / 64];
  const int begin = blockIdx.x * kItems;
  int running = blockoff[blockIdx.x];
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    const int slot = e < n ? slot_of[e] : -1;
    const bool first = slot >= 0 && table_val(t, slot) == e;
    int total;
    const int rank = block_rank(first, total, lds_wave);
    if (first) {
      const int vid = running + rank;
      if (vid < max_voxels) {
        slot_vid[slot] = vid;
        int c[4], b;
        hkey_t key;
        p2v_cell(pts, point_batch, e, nfeat, g, c, b, key);
        if (cells) {
          atomicOr(&cells[static_cast<unsigned long long>(key) >> 5].x, 1u << (key & 31));
        } else {
          int32_t *row = indices + static_cast<size_t>(vid) * (g.ndim + lead);
          if (lead) row[0] = b;
          for (int j = 0; j < g.ndim; ++j) row[lead + j] = c[j];
        }
      }
    }
    running += total;
  }
}

// The rank map from occupancy BITS already in place (cells[w].x; .y anything): block-local exclusive prefix of the
// words' popcounts -> cells[w].y, block total -> blockcount -- what conv4_prefix_kernel leaves, without a byte map in
// front.  Words travel lane-consecutive; the thread that scans eight consecutive words meets them in LDS.
__global__ void __launch_bounds__(kRankThreads)
p2v_rank_prefix_kernel(uint2 *__restrict__ cells, unsigned W, int32_t *__restrict__ blockcount) {
  __shared__ int lds_wave[kRankThreads / 64];
  __shared__ __attribute__((aligned(16))) uint32_t lds_bits[kRankWords];
  __shared__ __attribute__((aligned(16))) uint32_t lds_pre[kRankWords];
  const unsigned block0 = blockIdx.x * kRankWords;
#pragma unroll
  for (int j = 0; j < kRankPer; ++j) {
    const unsigned w = block0 + j * kRankThreads + threadIdx.x;
    lds_bits[j * kRankThreads + threadIdx.x] = w < W ? cells[w].x : 0u;
  }
  __syncthreads();
  static_assert(kRankPer == 8, "two 16-byte LDS accesses per thread");
  const uint4 a = reinterpret_cast<const uint4 *>(lds_bits)[threadIdx.x * 2];
  const uint4 b = reinterpret_cast<const uint4 *>(lds_bits)[threadIdx.x * 2 + 1];
  const uint32_t bits[kRankPer] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  int cnt[kRankPer], sum = 0;
#pragma unroll
  for (int e = 0; e < kRankPer; ++e) {
    cnt[e] = __popc(bits[e]);
    sum += cnt[e];
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
  uint32_t pre[kRankPer];
  int run = prefix + incl - sum;
#pragma unroll
  for (int e = 0; e < kRankPer; ++e) {
    pre[e] = static_cast<uint32_t>(run);
    run += cnt[e];
  }
  reinterpret_cast<uint4 *>(lds_pre)[threadIdx.x * 2] = make_uint4(pre[0], pre[1], pre[2], pre[3]);
  reinterpret_cast<uint4 *>(lds_pre)[threadIdx.x * 2 + 1] = make_uint4(pre[4], pre[5], pre[6], pre[7]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRankPer; ++j) {
    const unsigned w = block0 + j * kRankThreads + threadIdx.x;
    if (w < W) cells[w] = make_uint2(lds_bits[j * kRankThreads + threadIdx.x], lds_pre[j * kRankThreads + threadIdx.x]);
  }
  if (threadIdx.x == 0) blockcount[blockIdx.x] = total;
}

// Key order: the row of a kept voxel is the rank of its key in the level's rank map (cells, blockoff: rank_of).  The
// first point of the voxel renumbers its table slot and writes the index row {batch, zyx}; nobody else touches either.
__global__ void __launch_bounds__(kBlock)
p2v_renumber_kernel(const float *__restrict__ pts, const int32_t *__restrict__ point_batch, int n, int nfeat,
                    P2VGeom g, const int32_t *__restrict__ slot_of, Table t, const uint2 *__restrict__ cells,
                    const int32_t *__restrict__ blockoff, int max_voxels, int32_t *__restrict__ slot_vid,
                    int32_t *__restrict__ indices) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  const int slot = slot_of[e];
  if (slot < 0 || table_val(t, slot) != e || slot_vid[slot] < 0) return;
  int c[4], b;
  hkey_t key;
  p2v_cell(pts, point_batch, e, nfeat, g, c, b, key);
  const int vid = rank_of(cells, blockoff, static_cast<unsigned long long>(key));
  if (vid < 0 || vid >= max_voxels) return;          // (cannot happen: the voxel set its bit, ranks are < kept)
  slot_vid[slot] = vid;
  int32_t *row = indices + static_cast<size_t>(vid) * (g.ndim + 1);
  row[0] = b;
  for (int j = 0; j < g.ndim; ++j) row[1 + j] = c[j];
}

// `drop`: the sort key of a point without a voxel, above every voxel id (0xffffffff; the static form uses max_voxels,
// which bounds the digits the sort has to look at)
__global__ void __launch_bounds__(kBlock)
p2v_point_vid_kernel(const int32_t *__restrict__ slot_of, const int32_t *__restrict__ slot_vid, int n, uint32_t drop,
                     long long *__restrict__ pc_voxel_id, uint32_t *__restrict__ key32) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int slot = slot_of[i];
  const int vid = slot >= 0 ? slot_vid[slot] : -1;
  pc_voxel_id[i] = vid;
  key32[i] = vid < 0 ? drop : static_cast<uint32_t>(vid);
}

// sorted (voxel id, point) pairs -> slot of the point inside its voxel
__global__ void __launch_bounds__(kBlock)
p2v_segment_kernel(const uint32_t *__restrict__ keys, int n, uint32_t drop, int32_t *__restrict__ seg_start) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  const uint32_t v = keys[q];
  if (v != drop && (q == 0 || keys[q - 1] != v)) seg_start[v] = q;
}

// voxels == nullptr (the static form when only the mean is wanted): the counts alone
__global__ void __launch_bounds__(kBlock)
p2v_scatter_kernel(const float *__restrict__ pts, int nfeat, const uint32_t *__restrict__ keys,
                   const int32_t *__restrict__ order, int n, uint32_t drop, const int32_t *__restrict__ seg_start,
                   int max_points, float *__restrict__ voxels, int32_t *__restrict__ num_per_voxel) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  const uint32_t v = keys[q];
  if (v == drop) return;
  const int rank = q - seg_start[v];
  if (voxels && rank < max_points) {
    const float *src = pts + static_cast<size_t>(order[q]) * nfeat;
    float *dst = voxels + (static_cast<size_t>(v) * max_points + rank) * nfeat;
    for (int k = 0; k < nfeat; ++k) dst[k] = src[k];
  }
  if (q == n - 1 || keys[q + 1] != v) num_per_voxel[v] = min(rank + 1, max_points);
}

// empty_mean: slots num..max_points-1 of a voxel receive the mean of its points
__global__ void __launch_bounds__(kBlock)
p2v_mean_kernel(float *__restrict__ voxels, const int32_t *__restrict__ num_per_voxel,
                const int32_t *__restrict__ n_voxels, int max_points, int nfeat) {
  const long long gid = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const int v = static_cast<int>(gid / nfeat), k = static_cast<int>(gid % nfeat);
  if (v >= *n_voxels) return;
  const int num = num_per_voxel[v];
  if (num <= 0 || num >= max_points) return;
  float *base = voxels + static_cast<size_t>(v) * max_points * nfeat + k;
  float sum = 0.f;
  for (int j = 0; j < num; ++j) sum += base[static_cast<size_t>(j) * nfeat];
  const float mean = sum / static_cast<float>(num);
  for (int j = num; j < max_points; ++j) base[static_cast<size_t>(j) * nfeat] = mean;
}

// The reference's CPU loop AS IT BEHAVES (pointops.py:663-686): `mean_value.clear()` leaves the accumulator's
// contents in place, so voxel v starts from the mean of voxel v - 1:  m_v = (m_{v-1} + sum_j x_j) / num_v, point by
// point in fp32.  A sequential recurrence over the voxels in their (first-seen) order: one thread per feature
// walks all of them.  Opt-in (empty_mean = 2: SPCONV_AMD_REFERENCE_QUIRKS=1), bit-identical to the reference's code
// executed (tests/golden/p2v_ref.npz); milliseconds, not microseconds.
__global__ void p2v_mean_carry_kernel(float *__restrict__ voxels, const int32_t *__restrict__ num_per_voxel,
                                      const int32_t *__restrict__ n_voxels, int max_points, int nfeat) {
  const int k = threadIdx.x;
  if (k >= nfeat) return;
  const int nv = *n_voxels;
  float carry = 0.f;
  for (int v = 0; v < nv; ++v) {
    const int num = num_per_voxel[v];
    if (num <= 0) continue;
    float *base = voxels + static_cast<size_t>(v) * max_points * nfeat + k;
    for (int j = 0; j < num; ++j) carry += base[static_cast<size_t>(j) * nfeat];
    carry /= static_cast<float>(num);
    for (int j = num; j < max_points; ++j) base[static_cast<size_t>(j) * nfeat] = carry;
  }
}

// Mean feature row of every voxel ("mean VFE"): its stored points j = 0 .. num - 1 added in that order in fp32, divided
// by num in fp32, rounded to nearest-even into T; zeros for a voxel without points (a dead row).  The points come
// through the sorted list (point order inside a voxel: the sort is stable), not from `voxels`.
template <typename T>
__global__ void __launch_bounds__(kBlock)
p2v_voxel_mean_kernel(const float *__restrict__ pts, int nfeat, const int32_t *__restrict__ order,
                      const int32_t *__restrict__ seg_start, const int32_t *__restrict__ num_per_voxel,
                      int max_voxels, T *__restrict__ mean_out) {
  const long long gid = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const int v = static_cast<int>(gid / nfeat), k = static_cast<int>(gid % nfeat);
  if (v >= max_voxels) return;
  const int num = num_per_voxel[v];
  float mean = 0.f;
  if (num > 0) {
    const int32_t *pt = order + seg_start[v];
    float sum = 0.f;
    for (int j = 0; j < num; ++j) sum += pts[static_cast<size_t>(pt[j]) * nfeat + k];
    mean = sum / static_cast<float>(num);
  }
  mean_out[gid] = static_cast<T>(mean);
}

// n_voxels[0] = voxels kept, n_voxels[1] = voxels found (found > kept: the scene hit max_voxels)
__global__ void p2v_clamp_count_kernel(const int32_t *total, int max_voxels, int32_t *n_voxels) {
  n_voxels[0] = *total < max_voxels ? *total : max_voxels;
  n_voxels[1] = *total;
}

// ------------------------------------------------------- points by voxel id
// Stable LSD radix sort of (voxel id, point) with 8-bit digits built from the
// same count -> scan -> scatter primitives.
constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;

__global__ void __launch_bounds__(kBlock)
radix_count_kernel(const uint32_t *__restrict__ keys, int n, int shift, int nblk,
                   int32_t *__restrict__ hist /*[kRadix][nblk]*/) {
  __shared__ int lds_hist[kRadix];
  for (int d = threadIdx.x; d < kRadix; d += kBlock) lds_hist[d] = 0;
  __syncthreads();
  const int begin = blockIdx.x * kItems;
  for (int it = 0; it < kItems / kBlock; ++it) {
    const int e = begin + it * kBlock + threadIdx.x;
    if (e < n) atomicAdd(&lds_hist[(keys[e] >> shift) & (kRadix - 1)], 1);
  }
  __syncthreads();
  for (int d = threadIdx.x; d < kRadix; d += kBlock)
    hist[static_cast<size_t>(d) * nblk + blockIdx.x] = lds_hist[d];
}

// Stable scatter: processes the block's entries in order, 256 at a time; the
// rank of an entry among equal digits inside the 256-entry tile comes from a
// per-digit match over wave ballots.
__global__ void __launch_bounds__(kBlock)
radix_scatter_kernel(const uint32_t *__restrict__ keys_in, const int32_t *__restrict__ vals_in,
                     int n, int shift, int nblk, const int32_t *__restrict__ hist_off,
                     uint32_t *__restrict__ keys_out, int32_t *__restrict__ vals_out) {
  __shared__ int lds_base[kRadix];                 // running output offset per digit
  __shared__ int lds_cnt[kBlock / 64][kRadix];     // per-wave digit counts of this tile
  for (int d = threadIdx.x; d < kRadix; d += kBlock)
    lds_base[d] = hist_off[static_cast<size_t>(d) * nblk + blockIdx.x];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int begin = blockIdx.x * kItems;
  for (int it = 0; it < kItems / kBlock; ++it) {
    for (int d = threadIdx.x; d < kRadix; d += kBlock)
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) lds_cnt[w][d] = 0;
    __syncthreads();
    const int e = begin + it * kBlock + threadIdx.x;
    const bool valid = e < n;
    const uint32_t key = valid ? keys_in[e] : 0u;
    const int val = (valid && vals_in) ? vals_in[e] : e;
    const int digit = valid ? static_cast<int>((key >> shift) & (kRadix - 1)) : -1;
    // lanes of this wave holding the same digit (bitwise match over 8 ballots)
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < kRadixBits; ++bit) {
      const unsigned long long bal = __ballot((digit >> bit) & 1);
      same &= ((digit >> bit) & 1) ? bal : ~bal;
    }
    const int rank_in_wave = __popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank_in_wave == 0) lds_cnt[wave][digit] = __popcll(same);
    __syncthreads();
    if (valid) {
      int prior = 0;
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w)
        if (w < wave) prior += lds_cnt[w][digit];
      const int dst = lds_base[digit] + prior + rank_in_wave;
      keys_out[dst] = key;
      vals_out[dst] = val;
    }
    __syncthreads();
    for (int d = threadIdx.x; d < kRadix; d += kBlock) {
      int s = 0;
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) s += lds_cnt[w][d];
      lds_base[d] += s;
    }
    __syncthreads();
  }
}

struct P2VWs {
  Table t;
  int32_t *slot_of, *slot_vid, *blockcount, *blockoff, *total, *n_voxels, *seg_start, *order, *hist, *hist_off;
  uint32_t *key32, *kA, *kB;
  int32_t *vB;
  int nblk;
  // key order of the static form: a rank map of the call's own for a caller that keeps none, and the occupied cells
  // of each 2048-word block of the map (rank_W words; 0 = not carved)
  void *rankmap;
  int32_t *rank_blockcount;
  size_t bytes;
};

P2VWs carve_p2v_ws(void *ws, int n, int max_voxels, bool packed = false, size_t rank_W = 0) {
  const uint32_t cap = table_capacity(n > 0 ? n : 1);
  const size_t np = n > 0 ? n : 1;
  P2VWs w;
  w.nblk = div_up(static_cast<int>(np), kItems);
  Carver cv(ws);
  {
    hkey_t *keys = cv.take<hkey_t>(cap);
    table_place(w.t, keys, cv.take<int32_t>(cap), cap, packed);
  }
  w.slot_vid = cv.take<int32_t>(cap);
  w.slot_of = cv.take<int32_t>(np);
  w.blockcount = cv.take<int32_t>(w.nblk);
  w.blockoff = cv.take<int32_t>(w.nblk);
  w.total = cv.take<int32_t>(1);
  w.n_voxels = cv.take<int32_t>(2);
  w.seg_start = cv.take<int32_t>(max_voxels > 0 ? max_voxels : 1);
  w.order = cv.take<int32_t>(np);
  w.key32 = cv.take<uint32_t>(np);
  w.kA = cv.take<uint32_t>(np);
  w.kB = cv.take<uint32_t>(np);
  w.vB = cv.take<int32_t>(np);
  w.hist = cv.take<int32_t>(static_cast<size_t>(kRadix) * w.nblk);
  w.hist_off = cv.take<int32_t>(static_cast<size_t>(kRadix) * w.nblk);
  w.rankmap = nullptr;
  w.rank_blockcount = nullptr;
  if (rank_W) {
    w.rankmap = cv.take<uint8_t>(rank_bytes(rank_W));
    w.rank_blockcount = cv.take<int32_t>(rank_blocks(rank_W));
  }
  w.bytes = cv.off;
  return w;
}

P2VGeom make_p2v_geom(int ndim, int batch_size, const float *vsize, const float *coors_range, const int *grid_size) {
  P2VGeom g;
  g.ndim = ndim;
  g.batch = batch_size;
  for (int j = 0; j < 4; ++j) {
    g.vsize[j] = j < ndim ? vsize[j] : 1.f;
    g.lo[j] = j < ndim ? coors_range[j] : 0.f;
    g.grid[j] = j < ndim ? grid_size[j] : 1;
  }
  return g;
}

// Points behind their voxel ids: stable sort by key32 (`passes` 8-bit LSD passes, as mask_argsort; the result lands in
// kA / order), then the slot of each point inside its voxel, the stored points (voxels may be null) and the counts.
void p2v_sort_scatter(const float *points, int n, int nfeat, const P2VWs &w, int passes, uint32_t drop, int max_points,
                      float *voxels, int32_t *num_per_voxel, hipStream_t s) {
  const dim3 gp(div_up(n, kBlock));
  const uint32_t *kin = w.key32;
  const int32_t *vin = nullptr;
  for (int pass = 0; pass < passes; ++pass) {
    const bool last = ((passes - 1 - pass) & 1) == 0;
    uint32_t *kout = last ? w.kA : w.kB;
    int32_t *vout = last ? w.order : w.vB;
    hipLaunchKernelGGL(radix_count_kernel, dim3(w.nblk), dim3(kBlock), 0, s, kin, n, pass * kRadixBits,
                       w.nblk, w.hist);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kBlock), 0, s, w.hist, w.hist_off, kRadix * w.nblk,
                       static_cast<int32_t *>(nullptr));
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(w.nblk), dim3(kBlock), 0, s, kin, vin, n,
                       pass * kRadixBits, w.nblk, w.hist_off, kout, vout);
    kin = kout;
    vin = vout;
  }
  hipLaunchKernelGGL(p2v_segment_kernel, gp, dim3(kBlock), 0, s, w.kA, n, drop, w.seg_start);
  hipLaunchKernelGGL(p2v_scatter_kernel, gp, dim3(kBlock), 0, s, points, nfeat, w.kA, w.order, n, drop,
                     w.seg_start, max_points, voxels, num_per_voxel);
}

// The rank map of a key-ordered call: W words, 0 when the key space of batch x grid has no map (rank_words) or exceeds
// the 32-bit keys of the level builders behind it.
size_t p2v_rank_words(int ndim, int batch_size, const int *grid_size) {
  if (batch_size < 1 || !grid_size) return 0;
  const size_t W = rank_words(ndim, batch_size, grid_size);
  unsigned long long cells = static_cast<unsigned long long>(batch_size);
  for (int i = 0; W && i < ndim; ++i) cells *= static_cast<unsigned long long>(grid_size[i]);
  return (W && cells <= 0xffe00000ull && rank_bytes(W) <= (1ull << 30)) ? W : 0;
}
}  // namespace
}  // namespace spx

using namespace spx;

extern "C" {

size_t spx_point2voxel_ws_bytes(int n_points, int max_voxels) {
  return carve_p2v_ws(nullptr, n_points, max_voxels).bytes + 256;
}

int spx_point2voxel(const float *points, int n, int nfeat, int ndim, const float *vsize,
                    const float *coors_range, const int *grid_size, int max_voxels, int max_points,
                    int empty_mean, int clear_voxels, float *voxels, int32_t *indices,
                    int32_t *num_per_voxel, long long *pc_voxel_id, int *n_voxels_h, void *ws,
                    size_t ws_bytes, spx_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  SPX_CHECK(nfeat >= ndim, "points need at least %d columns, got %d", ndim, nfeat);
  SPX_CHECK(max_voxels > 0 && max_points > 0 && n >= 0, "bad sizes");
  SPX_CHECK(voxels && indices && num_per_voxel && (pc_voxel_id || n == 0) && n_voxels_h, "null pointer");
  SPX_CHECK(ws_bytes >= spx_point2voxel_ws_bytes(n, max_voxels), "workspace too small");
  *n_voxels_h = 0;
  SPX_HIP(hipMemsetAsync(num_per_voxel, 0, sizeof(int32_t) * max_voxels, s));
  if (clear_voxels)
    SPX_HIP(hipMemsetAsync(voxels, 0, sizeof(float) * static_cast<size_t>(max_voxels) * max_points * nfeat, s));
  if (n == 0) return 0;
  SPX_CHECK(points, "null pointer");
  const P2VGeom g = make_p2v_geom(ndim, 1, vsize, coors_range, grid_size);
  P2VWs w = carve_p2v_ws(ws, n, max_voxels, keys_fit_u32(1, g.grid, 4));
  const size_t cap = static_cast<size_t>(w.t.mask) + 1;
  SPX_HIP(table_clear(w.t, s));
  SPX_HIP(hipMemsetAsync(w.slot_vid, 0xFF, sizeof(int32_t) * cap, s));
  const dim3 gp(div_up(n, kBlock));
  const int32_t *no_batch = nullptr, *host_n_points = nullptr;
  hipLaunchKernelGGL(p2v_insert_kernel, gp, dim3(kBlock), 0, s, points, no_batch, n, host_n_points, nfeat, g, w.t,
                     w.slot_of);
  hipLaunchKernelGGL(p2v_count_first_kernel, dim3(w.nblk), dim3(kBlock), 0, s, w.slot_of, w.t, n,
                     w.blockcount);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kBlock), 0, s, w.blockcount, w.blockoff, w.nblk, w.total);
  hipLaunchKernelGGL(p2v_clamp_count_kernel, dim3(1), dim3(1), 0, s, w.total, max_voxels, w.n_voxels);
  hipLaunchKernelGGL(p2v_assign_kernel, dim3(w.nblk), dim3(kBlock), 0, s, points, no_batch, n, nfeat, g, w.slot_of,
                     w.t, w.blockoff, max_voxels, w.slot_vid, indices, 0, static_cast<uint2 *>(nullptr));
  hipLaunchKernelGGL(p2v_point_vid_kernel, gp, dim3(kBlock), 0, s, w.slot_of, w.slot_vid, n, 0xffffffffu,
                     pc_voxel_id, w.key32);
  p2v_sort_scatter(points, n, nfeat, w, 4, 0xffffffffu, max_points, voxels, num_per_voxel, s);
  if (empty_mean == 2) {
    SPX_CHECK(nfeat <= 1024, "reference-quirk mean fill: at most 1024 point features");
    hipLaunchKernelGGL(p2v_mean_carry_kernel, dim3(1), dim3(((nfeat + 63) / 64) * 64), 0, s, voxels, num_per_voxel,
                       w.n_voxels, max_points, nfeat);
  } else if (empty_mean) {
    const long long total = static_cast<long long>(max_voxels) * nfeat;
    hipLaunchKernelGGL(p2v_mean_kernel, dim3(static_cast<unsigned>((total + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, s, voxels, num_per_voxel, w.n_voxels, max_points, nfeat);
  }
  SPX_LAUNCH_CHECK();
  int32_t host_n = 0;
  SPX_HIP(hipMemcpyAsync(&host_n, w.n_voxels, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  SPX_HIP(hipStreamSynchronize(s));
  *n_voxels_h = host_n;
  return 0;
}

size_t spx_point2voxel_static_ws_bytes(int n_cap, int max_voxels, int ndim, int batch_size, const int *grid_size,
                                       int key_order) {
  const size_t W = key_order ? p2v_rank_words(ndim, batch_size, grid_size) : 0;
  if (key_order && W == 0) return 0;
  return carve_p2v_ws(nullptr, n_cap, max_voxels, false, W).bytes + 256;
}

int spx_point2voxel_static(const float *points, const int32_t *point_batch, int n_cap, const int32_t *n_points_dev,
                           int nfeat, int ndim, const float *vsize, const float *coors_range, const int *grid_size,
                           int batch_size, int max_voxels, int max_points, int empty_mean, int key_order,
                           float *voxels, int32_t *indices, int32_t *num_per_voxel, long long *pc_voxel_id,
                           int32_t *n_voxels_dev, void *mean_out, int mean_dtype, void *rankmap, size_t rankmap_bytes,
                           void *ws, size_t ws_bytes, spx_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  SPX_CHECK(ndim >= 1 && ndim <= kMaxNdim, "ndim must be in [1,4], got %d", ndim);
  SPX_CHECK(nfeat >= ndim, "points need at least %d columns, got %d", ndim, nfeat);
  SPX_CHECK(n_cap > 0 && max_voxels > 0 && max_points > 0 && batch_size > 0, "bad sizes");
  SPX_CHECK(points && n_points_dev && indices && num_per_voxel && pc_voxel_id && n_voxels_dev && vsize && coors_range &&
            grid_size, "null pointer");
  SPX_CHECK(empty_mean == 0 || empty_mean == 1,
            "empty_mean must be 0 or 1 (2, the reference-quirk recurrence, is sequential: spx_point2voxel has it)");
  SPX_CHECK(!empty_mean || voxels, "empty_mean fills the unused slots of `voxels`, which is NULL");
  SPX_CHECK(!mean_out || mean_dtype == SPX_F32 || mean_dtype == SPX_F16 || mean_dtype == SPX_BF16,
            "mean_dtype must be SPX_F32, SPX_F16 or SPX_BF16, got %d", mean_dtype);
  for (int j = 0; j < ndim; ++j) SPX_CHECK(grid_size[j] > 0, "grid_size[%d] = %d", j, grid_size[j]);
  const size_t W = key_order ? p2v_rank_words(ndim, batch_size, grid_size) : 0;
  SPX_CHECK(!key_order || W > 0,
            "key order numbers voxels through the level's rank map: batch x grid beyond 0xffe00000 cells (or a map "
            "beyond 1 GiB) has none -- use key_order = 0 and sort behind it");
  SPX_CHECK(key_order || !rankmap, "a rank map is left behind by key_order = 1 only");
  SPX_CHECK(!rankmap || rankmap_bytes >= rank_bytes(W), "rank map too small (%zu bytes needed)", rank_bytes(W));
  SPX_CHECK(ws && ws_bytes >= spx_point2voxel_static_ws_bytes(n_cap, max_voxels, ndim, batch_size, grid_size, key_order),
            "workspace too small");
  const P2VGeom g = make_p2v_geom(ndim, batch_size, vsize, coors_range, grid_size);
  P2VWs w = carve_p2v_ws(ws, n_cap, max_voxels, keys_fit_u32(batch_size, g.grid, 4), W);
  if (!rankmap) rankmap = w.rankmap;
  const size_t cap = static_cast<size_t>(w.t.mask) + 1;
  {
    // every fill of the call in one launch: an empty table, no slot numbered, every row dead (indices -1, count 0,
    // stored points 0) until a voxel claims it, no bit of the rank map set
    FillList fills;
    table_fill(fills, w.t);
    fills.add(w.slot_vid, sizeof(int32_t) * cap, 0xFFFFFFFFu);
    fills.add(indices, sizeof(int32_t) * static_cast<size_t>(max_voxels) * (ndim + 1), 0xFFFFFFFFu);
    fills.add(num_per_voxel, sizeof(int32_t) * max_voxels, 0u);
    if (voxels) fills.add(voxels, sizeof(float) * static_cast<size_t>(max_voxels) * max_points * nfeat, 0u);
    if (W) fills.add(rankmap, W * sizeof(uint2), 0u);
    SPX_HIP(fills.launch(s));
  }
  const dim3 gp(div_up(n_cap, kBlock));
  hipLaunchKernelGGL(p2v_insert_kernel, gp, dim3(kBlock), 0, s, points, point_batch, n_cap, n_points_dev, nfeat, g,
                     w.t, w.slot_of);
  hipLaunchKernelGGL(p2v_count_first_kernel, dim3(w.nblk), dim3(kBlock), 0, s, w.slot_of, w.t, n_cap, w.blockcount);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kBlock), 0, s, w.blockcount, w.blockoff, w.nblk, w.total);
  hipLaunchKernelGGL(p2v_clamp_count_kernel, dim3(1), dim3(1), 0, s, w.total, max_voxels, n_voxels_dev);
  hipLaunchKernelGGL(p2v_assign_kernel, dim3(w.nblk), dim3(kBlock), 0, s, points, point_batch, n_cap, nfeat, g,
                     w.slot_of, w.t, w.blockoff, max_voxels, w.slot_vid, indices, 1, W ? static_cast<uint2 *>(rankmap) : nullptr);
  if (W) {
    // bits -> rank map (prefix inside each 2048-word block, then the scan over the blocks), rank of a key -> row
    const int nblkW = static_cast<int>(rank_blocks(W));
    hipLaunchKernelGGL(p2v_rank_prefix_kernel, dim3(nblkW), dim3(kRankThreads), 0, s, static_cast<uint2 *>(rankmap),
                       static_cast<unsigned>(W), w.rank_blockcount);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kBlock), 0, s, w.rank_blockcount, rank_blockoff(rankmap, W), nblkW,
                       static_cast<int32_t *>(nullptr));
    hipLaunchKernelGGL(p2v_renumber_kernel, gp, dim3(kBlock), 0, s, points, point_batch, n_cap, nfeat, g, w.slot_of,
                       w.t, static_cast<const uint2 *>(rankmap),
                       static_cast<const int32_t *>(rank_blockoff(rankmap, W)), max_voxels, w.slot_vid, indices);
  }
  // a point without a voxel sorts behind voxel max_voxels - 1: the sort looks at the bytes of max_voxels only
  const uint32_t drop = static_cast<uint32_t>(max_voxels);
  int passes = 1;
  while (passes < 4 && (drop >> (passes * kRadixBits)) != 0) ++passes;
  hipLaunchKernelGGL(p2v_point_vid_kernel, gp, dim3(kBlock), 0, s, w.slot_of, w.slot_vid, n_cap, drop, pc_voxel_id,
                     w.key32);
  p2v_sort_scatter(points, n_cap, nfeat, w, passes, drop, max_points, voxels, num_per_voxel, s);
  const long long total = static_cast<long long>(max_voxels) * nfeat;
  const dim3 gm(static_cast<unsigned>((total + kBlock - 1) / kBlock));
  if (mean_out) {
    if (mean_dtype == SPX_F32)
      hipLaunchKernelGGL(p2v_voxel_mean_kernel<float>, gm, dim3(kBlock), 0, s, points, nfeat, w.order, w.seg_start,
                         num_per_voxel, max_voxels, static_cast<float *>(mean_out));
    else if (mean_dtype == SPX_F16)
      hipLaunchKernelGGL(p2v_voxel_mean_kernel<_Float16>, gm, dim3(kBlock), 0, s, points, nfeat, w.order, w.seg_start,
                         num_per_voxel, max_voxels, static_cast<_Float16 *>(mean_out));
    else
      hipLaunchKernelGGL(p2v_voxel_mean_kernel<__bf16>, gm, dim3(kBlock), 0, s, points, nfeat, w.order, w.seg_start,
                         num_per_voxel, max_voxels, static_cast<__bf16 *>(mean_out));
  }
  if (empty_mean)
    hipLaunchKernelGGL(p2v_mean_kernel, gm, dim3(kBlock), 0, s, voxels, num_per_voxel, n_voxels_dev, max_points, nfeat);
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
