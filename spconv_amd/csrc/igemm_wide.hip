// Column-blocked direct-fragment gather-GEMM: output widths beyond 256 (multiples of 128) on the MFMA kernels, forward
// and dgrad of f16 / bf16 / fp32 and the int8 forward, in ONE launch per layer and direction.  The kernel body is
// igemm_v4_body (igemm_v4.h) with WIDE = true: a workgroup owns 64 rows x kWideNT columns, rows of `out` (and of the
// fp32 scratch of grouped kernel volumes, and of the int8 residual input) are p.COUT wide, and the workgroup's first
// column moves the weight slice and the per-channel vectors.  The reduction of an output element is the one of the
// narrow kernels: results are bit-identical to 128- / 256-wide launches over slices of the weights.
//
// Block order.  Workgroups are dealt round-robin to the 8 XCDs (block b runs on XCD b % 8) and every XCD has an L2 of
// its own.  The column blocks of one row tile read the same table rows and gather the same feature rows, so they are
// folded into the block index as  b = (row_block / 8 * ncb + column_block) * 8 + row_block % 8:  the ncb column blocks
// of a row tile are dispatched back to back on ONE XCD (the first one's gathers fill the L2 the others hit), and row
// block r still runs on XCD r % 8, which is what xcd_tile / the appendix order of igemm_v4_body assume.  The row-block
// count is rounded up to a multiple of 8; the surplus workgroups leave at once.
#include "igemm_v4.h"

namespace spx {
namespace {

template <int NT, int DT, bool BT, int NKS, int PK>
__global__ void __launch_bounds__(kThreads)
igemm_v4w_kernel(const void *argA, const void *argB, const uint32_t *arg_mask, const int32_t *arg_argsort,
                 const int32_t *arg_pair, int n_dst, int n_src, int CIN, int kv, int identity_k, int b_reverse,
                 GemmRest rest) {
  GemmParams p;
  unpack_gemm_args(p, argA, argB, arg_mask, arg_argsort, arg_pair, n_dst, n_src, CIN, kv, identity_k, b_reverse, rest);
  const int ncb = rest.COUT / NT;                                    // (uniform: scalar arithmetic)
  const int b = static_cast<int>(blockIdx.x);
  const int row_block = (b / (8 * ncb)) * 8 + (b & 7);
  const int row_blocks = (p.cls ? p.app_rows : 0) + (n_dst + 63) / 64;   // appendix workgroups + 64-row tiles
  if (row_block >= row_blocks) return;
  p.n0 = ((b >> 3) % ncb) * NT;
  igemm_v4_body<NT, 1, DT, BT, NKS, PK, true>(p, row_block);
}

template <int DT>
int launch_v4w(const GemmParams &p, hipStream_t s) {
  constexpr int NT = kWideNT;
  const int ntiles = div_up(p.n_dst, 64);
  const int napp = p.cls ? (p.app_rows > 0 ? div_up(p.app_rows, 64) : layout_app_tiles(p.n_dst, 64)) : 0;
  const int ncb = p.COUT / NT;
  const long long grid = static_cast<long long>((napp + ntiles + 7) & ~7) * ncb;
  if (grid >= 0x7fffffffll) {
    set_error("gather-GEMM grid too large (%lld workgroups)", grid);
    return -1;
  }
  GemmParams q = p;
  // more workgroups than the chip holds at once.  512 is the threshold of the 128- / 256-wide instances (launch_v4),
  // inherited, not measured here: these instances hold 3 (16-bit, fp32) to 5 (int8) workgroups per CU.  Results do not
  // depend on it.  Likewise the tile is always 64 rows (the narrow kernels take 128 rows beyond 32 k rows).
  q.lpt = p.tile_order && static_cast<long long>(ntiles) * ncb > 512;
  GemmRest r = rest_of(p);
  r.napp = p.cls ? napp : -1;
  r.stats = nullptr;                         // no BatchNorm statistics out of this epilogue: the caller's sink stays empty
  r.n_live = nullptr;
  if (p.grid_out) *p.grid_out = 0;
  constexpr int es = DT == 2 ? 1 : (DT == 3 ? 4 : 2);
  const bool half = p.CIN * es <= 64;
  int pk = v4_pack(p, DT, es);
  if (pk >= 8) pk = pk == 32 ? 4 : (pk == 16 ? 2 : 1);       // (SPX_PK = 3: the one-piece forms are what exists here)
  count(kFamV4w);
#define SPX_LAUNCH_V4W(BTV, NKSV, PKV)                                                                       \
  do {                                                                                                       \
    count_inst<inst::v4w(DT, BTV, NKSV, PKV)>();                                                             \
    hipLaunchKernelGGL((igemm_v4w_kernel<NT, DT, BTV, NKSV, PKV>), dim3(static_cast<unsigned>(grid)),        \
                       dim3(kThreads), (v4_smem_bytes<NT, 1, DT>()), s, p.A, p.B, p.mask, p.argsort, p.pair, \
                       p.n_dst, p.n_src, p.CIN, p.kv, p.identity_k, v4_flags(q), r);                         \
  } while (0)
  if (DT == 2 || p.strideD == 1) {
    if constexpr (DT == 0 || DT == 1) {
      if (pk == 4) SPX_LAUNCH_V4W(false, 1, 4);
      else if (pk == 2) SPX_LAUNCH_V4W(false, 1, 2);
      else if (half) SPX_LAUNCH_V4W(false, 1, 1);
      else SPX_LAUNCH_V4W(false, 2, 1);
    } else {
      if (half) SPX_LAUNCH_V4W(false, 1, 1);
      else SPX_LAUNCH_V4W(false, 2, 1);
    }
  } else if constexpr (DT != 2) {
    if constexpr (DT == 0 || DT == 1) {
      if (pk == 4) SPX_LAUNCH_V4W(true, 1, 4);
      else if (pk == 2) SPX_LAUNCH_V4W(true, 1, 2);
      else if (half) SPX_LAUNCH_V4W(true, 1, 1);
      else SPX_LAUNCH_V4W(true, 2, 1);
    } else {
      if (half) SPX_LAUNCH_V4W(true, 1, 1);
      else SPX_LAUNCH_V4W(true, 2, 1);
    }
  }
#undef SPX_LAUNCH_V4W
  SPX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

int launch_gather_gemm_wide(const GemmParams &p, int dt, hipStream_t s) {
  if (!wide_cout(p.COUT)) {
    set_error("column-blocked gather-GEMM: output width %d is not a multiple of %d beyond 256", p.COUT, kWideNT);
    return -1;
  }
  GemmParams q = p;
  q.dense_hint = 0;
  switch (dt) {
    case 0: return launch_v4w<0>(q, s);
    case 1: return launch_v4w<1>(q, s);
    case 2: return launch_v4w<2>(q, s);
    case 3: return launch_v4w<3>(q, s);
  }
  set_error("column-blocked gather-GEMM: bad operand type %d", dt);
  return -1;
}

}  // namespace spx
