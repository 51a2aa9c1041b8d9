// Block-level prefix primitives of the count -> scan -> scatter pipelines: the rank of a thread among the flagged
// threads of its workgroup, and the exclusive scan of a sequence of int32 counts by one workgroup.  Shared by the
// translation units that number rows (rulebook_*.hip through rulebook.h, voxelize.hip, hash.hip, rowsort.hip, dense.hip,
// union.hip, collapse.hip, select.hip) and, through rankmap.h, by every unit that includes that (interp.hip); every
// definition has internal linkage.  Workgroups are kScanThreads wide: a unit asserts that its own kBlock agrees.
#pragma once
#include "common.h"

namespace spx {
namespace {
constexpr int kScanThreads = 256;
constexpr int kScanPer = 32;          // items per thread of the one-pass form

// Exclusive rank of this thread among the threads of the block with pred set,
// plus the block total.  wave64 ballot + mbcnt; wave totals through LDS.
__device__ __forceinline__ int block_rank(bool pred, int &total, int *lds_wave /*[4]*/) {
  const unsigned long long bal = __ballot(pred);
  const int lane_rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bal >> 32),
                            __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bal), 0u));
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // protect lds_wave reuse across calls
  if ((threadIdx.x & 63) == 0) lds_wave[wave] = __popcll(bal);
  __syncthreads();
  int prefix = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    const int c = lds_wave[w];
    if (w < wave) prefix += c;
    total += c;
  }
  return prefix + lane_rank;
}

// Exclusive scan of c[0 .. len) into o by the whole block, kScanThreads items per round with the carry in a
// register; returns the sum (to every thread).
__device__ __forceinline__ int block_scan_loop(const int32_t *__restrict__ c, int32_t *__restrict__ o, int len,
                                               int *lds_wave /*[4]*/) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < len; base += kScanThreads) {
    const int idx = base + threadIdx.x;
    const int v = idx < len ? c[idx] : 0;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    __syncthreads();                      // (lds_wave of the previous round has been read)
    if (lane == 63) lds_wave[wave] = incl;
    __syncthreads();
    int prefix = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
      const int s = lds_wave[w];
      if (w < wave) prefix += s;
      total += s;
    }
    if (idx < len) o[idx] = carry + prefix + incl - v;
    carry += total;
  }
  return carry;
}

// seq-wise exclusive scan of `cnt` (length len per sequence), one block per
// sequence; totals[seq] receives the sequence sum (totals may be null).
__global__ void __launch_bounds__(kScanThreads)
scan_kernel(const int32_t *__restrict__ cnt, int32_t *__restrict__ off, int len,
            int32_t *__restrict__ totals) {
  __shared__ int lds_wave[kScanThreads / 64];
  const int seq = blockIdx.x;
  const int32_t *c = cnt + static_cast<size_t>(seq) * len;
  int32_t *o = off + static_cast<size_t>(seq) * len;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (len <= kScanThreads * kScanPer) {
    // one pass: every thread owns `per` consecutive items (all loads in flight together), one block
    // scan of the thread sums -- the loop form pays a load -> barrier -> store round per 256 items
    const int per = (len + kScanThreads - 1) / kScanThreads, base = threadIdx.x * per;
    int v[kScanPer];
    int sum = 0;
#pragma unroll
    for (int e = 0; e < kScanPer; ++e) {
      v[e] = (e < per && base + e < len) ? c[base + e] : 0;
      sum += v[e];
    }
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
    for (int w = 0; w < kScanThreads / 64; ++w) {
      const int x = lds_wave[w];
      if (w < wave) prefix += x;
      total += x;
    }
    int run = prefix + incl - sum;
#pragma unroll
    for (int e = 0; e < kScanPer; ++e) {
      if (e < per && base + e < len) o[base + e] = run;
      run += v[e];
    }
    if (threadIdx.x == 0 && totals) totals[seq] = total;
    return;
  }
  const int carry = block_scan_loop(c, o, len, lds_wave);
  if (threadIdx.x == 0 && totals) totals[seq] = carry;
}
}  // namespace
}  // namespace spx
