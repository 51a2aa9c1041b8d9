// Conversions between the two list forms of a rulebook: spx_native_to_table, spx_table_to_native.  The compaction
// kernels and their launcher are shared with the builders: rulebook.h.
#include "rulebook.h"

namespace spx {
namespace {

__global__ void __launch_bounds__(kBlock)
subm_center_list_kernel(int32_t *__restrict__ native, int kv, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const size_t c = static_cast<size_t>(kv / 2) * n + i;
  native[c] = i;
  native[static_cast<size_t>(kv) * n + c] = i;
}

// Dense table from ConvAlgo.Native lists (for callers that only hold the lists):
// table[k][dst_j] = src_j for j < count(k).  count(): SubM mirror rule (ops.py:962-968).
__global__ void __launch_bounds__(kBlock)
native_to_table_kernel(const int32_t *__restrict__ native, const int32_t *__restrict__ num,
                       int kv, int n_in, int n_dst, int subm, int inverse,
                       int32_t *__restrict__ table) {
  const int k = blockIdx.y;
  const int j = blockIdx.x * kBlock + threadIdx.x;
  int cnt;
  if (!subm) cnt = num[k];
  else if (k == kv / 2) cnt = n_in;
  else cnt = k < kv / 2 ? num[k] : num[kv - 1 - k];
  if (cnt > n_in) cnt = n_in;  // convops.py:1592 clamp
  if (j >= cnt) return;
  const size_t plane = static_cast<size_t>(kv) * n_in;
  const size_t e = static_cast<size_t>(k) * n_in + j;
  const int in_idx = native[e], out_idx = native[plane + e];
  const int src = inverse ? out_idx : in_idx, dst = inverse ? in_idx : out_idx;
  table[static_cast<size_t>(k) * n_dst + dst] = src;
}

struct ListsWs {
  int32_t *blockcount, *blockoff;
  int nblk;
  size_t bytes;
};
ListsWs carve_lists_ws(void *ws, int n, int kv) {
  ListsWs w;
  w.nblk = div_up(n > 0 ? n : 1, kItems);
  Carver cv(ws);
  w.blockcount = cv.take<int32_t>(static_cast<size_t>(kv) * w.nblk);
  w.blockoff = cv.take<int32_t>(static_cast<size_t>(kv) * w.nblk);
  w.bytes = cv.off;
  return w;
}

}  // namespace
}  // namespace spx

using namespace spx;

extern "C" {

int spx_native_to_table(const int32_t *pair_native, const int32_t *num_per_loc, int n_in, int n_dst, int kv, int subm,
                        int inverse, int32_t *table, uint32_t *mask, spx_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  SPX_CHECK(pair_native && num_per_loc && table, "null pointer");
  if (n_dst == 0) return 0;
  SPX_HIP(hipMemsetAsync(table, 0xFF, sizeof(int32_t) * static_cast<size_t>(kv) * n_dst, s));
  if (n_in > 0)
    hipLaunchKernelGGL(native_to_table_kernel, dim3(div_up(n_in, kBlock), kv), dim3(kBlock), 0, s, pair_native,
                       num_per_loc, kv, n_in, n_dst, subm, inverse, table);
  if (mask)
    hipLaunchKernelGGL(mask_from_table_kernel, dim3(div_up(n_dst, kBlock)), dim3(kBlock), 0, s, table, kv, n_dst,
                       div_up(kv, 32), mask);
  SPX_LAUNCH_CHECK();
  return 0;
}

size_t spx_table_to_native_ws_bytes(int n, int kv) { return carve_lists_ws(nullptr, n, kv).bytes + 256; }

int spx_table_to_native(const int32_t *table, int subm, int kv, int n, int32_t *pair_native, int32_t *num_per_loc,
                        void *ws, size_t ws_bytes, spx_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  SPX_CHECK(table && pair_native && num_per_loc && ws, "null pointer");
  SPX_CHECK(ws_bytes >= spx_table_to_native_ws_bytes(n, kv), "workspace too small");
  SPX_HIP(hipMemsetAsync(num_per_loc, 0, sizeof(int32_t) * kv, s));
  if (n == 0) return 0;
  SPX_HIP(hipMemsetAsync(pair_native, 0xFF, sizeof(int32_t) * 2 * static_cast<size_t>(kv) * n, s));
  const ListsWs w = carve_lists_ws(ws, n, kv);
  if (subm)
    hipLaunchKernelGGL(subm_center_list_kernel, dim3(div_up(n, kBlock)), dim3(kBlock), 0, s, pair_native, kv, n);
  return launch_native_lists(table, subm ? 0 : 1, kv, n, subm ? kv / 2 : kv, w.nblk, w.blockcount, w.blockoff,
                             pair_native, num_per_loc, s);
}

}  // extern "C"
