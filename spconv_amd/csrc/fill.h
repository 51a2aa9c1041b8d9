// Range fills shared by the translation units that build index structures (rulebook_*.hip through table.h,
// voxelize.hip, hash.hip, union.hip, collapse.hip, select.hip, interp.hip); every definition has internal linkage.
#pragma once
#include "common.h"

namespace spx {
namespace {
constexpr int kFillThreads = 256;

// ------------------------------------------------------------ range fills
// Every "memset" of a rulebook build in ONE launch: on a host-bound pipeline (a single scene per
// step) a rulebook is a dozen launches of ~6 us of host time each, and hipMemsetAsync costs a
// launch like any kernel.  Ranges are 4-byte aligned multiples of 4 bytes; the 16-byte aligned
// middle of each goes out as dwordx4 stores.
constexpr int kMaxFills = 8;
struct FillJobs {
  uint32_t *ptr[kMaxFills];
  unsigned long long words[kMaxFills];
  uint32_t value[kMaxFills];
  int n;
};

__global__ void __launch_bounds__(kFillThreads)
fill_ranges_kernel(FillJobs jobs) {
  const unsigned long long t = static_cast<unsigned long long>(blockIdx.x) * kFillThreads + threadIdx.x;
  const unsigned long long T = static_cast<unsigned long long>(gridDim.x) * kFillThreads;
  for (int j = 0; j < jobs.n; ++j) {
    uint32_t *p = jobs.ptr[j];
    const unsigned long long w = jobs.words[j];
    const uint32_t v = jobs.value[j];
    unsigned long long head = (4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3;
    if (head > w) head = w;
    const unsigned long long body = (w - head) >> 2, tail = (w - head) & 3;
    if (t < head) p[t] = v;
    uint4 *q = reinterpret_cast<uint4 *>(p + head);
    const uint4 vv = make_uint4(v, v, v, v);
    for (unsigned long long i = t; i < body; i += T) q[i] = vv;
    if (t < tail) p[head + 4 * body + t] = v;
  }
}

struct FillList {
  FillJobs jobs;
  FillList() { jobs.n = 0; }
  // adjacent ranges with the same value merge (tables carved from one buffer: one range)
  void add(void *ptr, size_t bytes, uint32_t value) {
    if (!ptr || bytes == 0) return;
    uint32_t *p = static_cast<uint32_t *>(ptr);
    for (int j = 0; j < jobs.n; ++j) {
      if (jobs.value[j] != value) continue;
      if (jobs.ptr[j] + jobs.words[j] == p) { jobs.words[j] += bytes / 4; return; }
      if (p + bytes / 4 == jobs.ptr[j]) { jobs.ptr[j] = p; jobs.words[j] += bytes / 4; return; }
    }
    jobs.ptr[jobs.n] = p;
    jobs.words[jobs.n] = bytes / 4;
    jobs.value[jobs.n] = value;
    ++jobs.n;
  }
  // another list's ranges, in its order (a caller's fills riding in a pass's launch)
  void add(const FillList &more) {
    for (int j = 0; j < more.jobs.n; ++j) add(more.jobs.ptr[j], more.jobs.words[j] * 4, more.jobs.value[j]);
  }
  hipError_t launch(hipStream_t s) const {
    if (jobs.n == 0) return hipSuccess;
    unsigned long long most = 0;
    for (int j = 0; j < jobs.n; ++j) most = jobs.words[j] > most ? jobs.words[j] : most;
    // 16 words (four dwordx4) per thread of the longest range, at most 2048 workgroups
    unsigned long long blocks = (most + 16ull * kFillThreads - 1) / (16ull * kFillThreads);
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(fill_ranges_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kFillThreads), 0, s, jobs);
    return hipGetLastError();
  }
};
}  // namespace
}  // namespace spx
