// Shared host/device helpers for the gfx950 kernels.  wave = 64 lanes everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>

#include <atomic>

#include "../../include/spconv_amd.h"

namespace spx {

constexpr int kWave = 64;
constexpr int kMaxNdim = SPX_MAX_NDIM;

void set_error(const char *fmt, ...);

// Integer tuning knob from the environment (A/B measurements; defaults are the shipped choice).
inline int env_int(const char *name, int dflt) {
  const char *v = getenv(name);
  return v ? atoi(v) : dflt;
}

// The same, read at every call and overridable at run time through spx_set_option (switches a test or a
// benchmark flips inside one process; env_int values are usually cached in function-local statics).
int option_int(const char *name, int dflt);

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int div_up(int a, int b) { return (a + b - 1) / b; }
// bytes of one element of a feature dtype (SPX_F32 / SPX_F16 / SPX_BF16 / SPX_I8 / SPX_F64)
inline int elem_bytes(int dtype) { return dtype == SPX_F64 ? 8 : (dtype == SPX_F32 ? 4 : (dtype == SPX_I8 ? 1 : 2)); }

// Carves 256-byte aligned sub-buffers out of the caller's scratch.
struct Carver {
  char *base;
  size_t off = 0;
  explicit Carver(void *p) : base(static_cast<char *>(p)) {}
  template <typename T> T *take(size_t count) {
    T *r = reinterpret_cast<T *>(base + off);
    off += align_up(count * sizeof(T), 256);
    return r;
  }
};

#define SPX_CHECK(cond, ...)                 \
  do {                                       \
    if (!(cond)) {                           \
      ::spx::set_error(__VA_ARGS__);         \
      return -1;                             \
    }                                        \
  } while (0)

#define SPX_HIP(expr)                                                         \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) {                                                   \
      ::spx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                       __FILE__, __LINE__);                                   \
      return -2;                                                              \
    }                                                                         \
  } while (0)

#define SPX_LAUNCH_CHECK() SPX_HIP(hipGetLastError())

// A kernel that needs more than 64 KB of dynamic LDS raises hipFuncAttributeMaxDynamicSharedMemorySize first.  The
// attribute belongs to (function, DEVICE): `done` keeps one bit per device index, so a process that drives several
// GPUs sets it on each of them, from any thread (round-5 ADVICE: a plain static flag set it on the first device only).
inline hipError_t ensure_dynamic_lds(const void *fn, int bytes, std::atomic<uint64_t> &done) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
  return e;
}

// Canonical 4-d description of a 1..4-d problem: leading dims are padded with
// size-1 / ksize-1 entries so one kernel serves every ndim.  Column c of an
// index row (batch at column 0) maps to canonical spatial dim c-1+(4-ndim).
struct Geom {
  int ndim;           // user ndim
  int batch;
  int in_dims[4];
  int out_dims[4];
  int ksize[4], stride[4], padding[4], dilation[4];
  int kv;
};

inline Geom make_geom(int ndim, int batch, const int *in_dims, const int *out_dims,
                      const int *ksize, const int *stride, const int *padding,
                      const int *dilation) {
  Geom g;
  g.ndim = ndim;
  g.batch = batch;
  const int lead = 4 - ndim;
  g.kv = 1;
  for (int i = 0; i < 4; ++i) {
    const bool pad = i < lead;
    const int j = i - lead;
    g.in_dims[i] = pad ? 1 : in_dims[j];
    g.out_dims[i] = pad ? 1 : out_dims[j];
    g.ksize[i] = pad ? 1 : ksize[j];
    g.stride[i] = pad ? 1 : (stride ? stride[j] : 1);
    g.padding[i] = pad ? 0 : (padding ? padding[j] : 0);
    g.dilation[i] = pad ? 1 : (dilation ? dilation[j] : 1);
    g.kv *= g.ksize[i];
  }
  return g;
}

}  // namespace spx

// ---- launch counters (diagnostics: which kernel family a call dispatched; spx_launch_count) --------
namespace spx {
enum LaunchFamily { kFamV4 = 0, kFamWs, kFamBwdFused, kFamBwdRows, kFamI8Stream, kFamGeneric, kFamStage2, kFamStage2Batch,
                    kFamF64, kFamV4w, kFamCount };
extern std::atomic<long long> g_launches[kFamCount];
inline void count_launch(LaunchFamily f) { g_launches[f].fetch_add(1, std::memory_order_relaxed); }

// Launches shaped by the host's exact appendix row count (SPX_SPARSE_ROWS_HINT), counted NEXT TO their family: keys
// sparse_hint/v4 (forward and dgrad launches of igemm_v4_kernel) and sparse_hint/bwd (fused backward).
enum HintInst { kHintV4 = 0, kHintBwd, kHintCount };
extern std::atomic<long long> g_hint_launches[kHintCount];
inline void count_hint(HintInst i) { g_hint_launches[i].fetch_add(1, std::memory_order_relaxed); }

// Per-INSTANCE counters (the keys with a '/' of spx_launch_count): one flat table, each template instance a slot whose
// index is a constant expression of its template parameters, so a launch site adds one relaxed increment and formats
// nothing.  dt codes are the kernels' DT parameter: 0 f16, 1 bf16, 2 i8, 3 f32.  common.cpp parses the keys.
namespace inst {
constexpr int cout_slot(int c) { return c == 16 ? 0 : c == 32 ? 1 : c == 64 ? 2 : c == 128 ? 3 : c == 256 ? 4 : -1; }
constexpr int pk_slot(int pk) {
  return pk == 1 ? 0 : pk == 2 ? 1 : pk == 4 ? 2 : pk == 8 ? 3 : pk == 16 ? 4 : pk == 32 ? 5 : -1;
}
constexpr int sl_slot(int sl) { return sl == 2 ? 0 : sl == 4 ? 1 : sl == 8 ? 2 : -1; }
constexpr int kCouts = 5, kDts = 4, kPks = 6;
constexpr int kV4 = 0;                                                    // COUT x MB x dt x BT x NKS x PK
constexpr int kBwd = kV4 + kCouts * 2 * kDts * 2 * 2 * kPks;              // COUT x MB x dt x NKS x PK
constexpr int kWs = kBwd + kCouts * 2 * kDts * 2 * kPks;                  // dt
constexpr int kBwdRows = kWs + kDts;                                      // C x K x dt x W8
constexpr int kWgradTr = kBwdRows + 2 * 2 * kDts * 2;                     // dt x SL
constexpr int kWgradF32 = kWgradTr + kDts * 3;
constexpr int kWgradMfma = kWgradF32 + 1;                                 // dt
constexpr int kWgradGeneric = kWgradMfma + kDts;                          // dt
constexpr int kGeneric = kWgradGeneric + kDts;                            // dt
constexpr int kGen1 = kGeneric + kDts;                                    // COUT x dt
constexpr int kV4w = kGen1 + kCouts * kDts;                               // dt x BT x NKS x PK (1, 2, 4)
constexpr int kWidePks = 3;
constexpr int kCount = kV4w + kDts * 2 * 2 * kWidePks;

constexpr int v4(int cout, int mb, int dt, bool bt, int nks, int pk) {
  return kV4 + ((((cout_slot(cout) * 2 + (mb - 1)) * kDts + dt) * 2 + (bt ? 1 : 0)) * 2 + (nks - 1)) * kPks + pk_slot(pk);
}
constexpr int bwd(int cout, int mb, int dt, int nks, int pk) {
  return kBwd + (((cout_slot(cout) * 2 + (mb - 1)) * kDts + dt) * 2 + (nks - 1)) * kPks + pk_slot(pk);
}
constexpr int ws(int dt) { return kWs + dt; }
constexpr int bwd_rows(int c, int k, int dt, bool w8) {
  return kBwdRows + (((c == 32 ? 1 : 0) * 2 + (k == 32 ? 1 : 0)) * kDts + dt) * 2 + (w8 ? 1 : 0);
}
constexpr int wgrad_tr(int dt, int sl) { return kWgradTr + dt * 3 + sl_slot(sl); }
constexpr int wgrad_mfma(int dt) { return kWgradMfma + dt; }
constexpr int wgrad_generic(int dt) { return kWgradGeneric + dt; }
constexpr int generic(int dt) { return kGeneric + dt; }
constexpr int gen1(int cout, int dt) { return kGen1 + cout_slot(cout) * kDts + dt; }
// column-blocked launches (igemm_wide.hip; the tile is 128 columns x 64 rows).  Instances that exist: pk 2 / 4 with
// nks 1 and a 16-bit type only; int8 forward only.
constexpr bool v4w_exists(int dt, bool bt, int nks, int pk) {
  return dt >= 0 && dt < kDts && (nks == 1 || nks == 2) && (pk == 1 || ((pk == 2 || pk == 4) && nks == 1 && dt <= 1)) &&
         !(dt == 2 && bt);
}
constexpr int v4w(int dt, bool bt, int nks, int pk) {
  return kV4w + ((dt * 2 + (bt ? 1 : 0)) * 2 + (nks - 1)) * kWidePks + pk_slot(pk);
}
}  // namespace inst

extern std::atomic<long long> g_inst_launches[inst::kCount];
template <int I>
inline void count_inst() {
  static_assert(I >= 0 && I < inst::kCount, "instance counter slot");
  g_inst_launches[I].fetch_add(1, std::memory_order_relaxed);
}

// float64 kernels (igemm_f64.hip, pool.hip): a table of their own, outside the dt vocabulary of the instances above.
// Keys igemm_f64/fwd, igemm_f64/dgrad, wgrad_f64, pool/f64.
enum F64Inst { kF64Fwd = 0, kF64Dgrad, kF64Wgrad, kF64Pool, kF64Count };
extern std::atomic<long long> g_f64_launches[kF64Count];
inline void count_f64(F64Inst i) { g_f64_launches[i].fetch_add(1, std::memory_order_relaxed); }

// sparse <-> dense conversion (dense.hip): one counter per entry point and layout.
// Keys dense/map, dense/scatter_cl, dense/scatter_cf, dense/gather_cl, dense/gather_cf, dense/compact.
enum DenseInst { kDenseMap = 0, kDenseScatterCl, kDenseScatterCf, kDenseGatherCl, kDenseGatherCf, kDenseCompact, kDenseCount };
extern std::atomic<long long> g_dense_launches[kDenseCount];
inline void count_dense(DenseInst i) { g_dense_launches[i].fetch_add(1, std::memory_order_relaxed); }

// misaligned add (union.hip): one counter per stage.
// Keys union/mark, union/prefix, union/claim, union/fill, union/add_fwd, union/add_bwd.
enum UnionInst { kUnionMark = 0, kUnionPrefix, kUnionClaim, kUnionFill, kUnionAddFwd, kUnionAddBwd, kUnionCount };
extern std::atomic<long long> g_union_launches[kUnionCount];
inline void count_union(UnionInst i) { g_union_launches[i].fetch_add(1, std::memory_order_relaxed); }

// axis collapse (collapse.hip): one counter per pass.
// Keys collapse/mark, collapse/prefix, collapse/rank, collapse/list, collapse/fwd, collapse/bwd.
enum CollapseInst { kCollapseMark = 0, kCollapsePrefix, kCollapseRank, kCollapseList, kCollapseFwd, kCollapseBwd,
                    kCollapseCount };
extern std::atomic<long long> g_collapse_launches[kCollapseCount];
inline void count_collapse(CollapseInst i) { g_collapse_launches[i].fetch_add(1, std::memory_order_relaxed); }

// point <-> voxel features (pointvoxel.hip): one counter per entry point.
// Keys pointvoxel/groups, pointvoxel/gather, pointvoxel/decorate.
enum PointVoxelInst { kPvGroups = 0, kPvGather, kPvDecorate, kPvCount };
extern std::atomic<long long> g_pointvoxel_launches[kPvCount];
inline void count_pointvoxel(PointVoxelInst i) { g_pointvoxel_launches[i].fetch_add(1, std::memory_order_relaxed); }

// trilinear devoxelisation (interp.hip): one counter per entry point and lookup form.
// Keys interp/corners_ranked, interp/corners_hash, interp/fwd, interp/bwd.
enum InterpInst { kInterpCornersRanked = 0, kInterpCornersHash, kInterpFwd, kInterpBwd, kInterpCount };
extern std::atomic<long long> g_interp_launches[kInterpCount];
inline void count_interp(InterpInst i) { g_interp_launches[i].fetch_add(1, std::memory_order_relaxed); }

// voxel query and neighbour grouping (query.hip): one counter per entry point and lookup form.
// Keys query/ranked, query/hash, query/group_fwd, query/group_bwd.
enum QueryInst { kQueryRanked = 0, kQueryHash, kQueryGroupFwd, kQueryGroupBwd, kQueryCount };
extern std::atomic<long long> g_query_launches[kQueryCount];
inline void count_query(QueryInst i) { g_query_launches[i].fetch_add(1, std::memory_order_relaxed); }

// farthest-point sampling and ball query over raw points (sample.hip) and the k-nearest-neighbour query (knn.hip): one
// counter per entry point.  Keys sample/fps, sample/ball_query, sample/knn_query.
enum SampleInst { kSampleFps = 0, kSampleBallQuery, kSampleKnnQuery, kSampleCount };
extern std::atomic<long long> g_sample_launches[kSampleCount];
inline void count_sample(SampleInst i) { g_sample_launches[i].fetch_add(1, std::memory_order_relaxed); }

// rotated boxes (box.hip): one counter per kernel, counted once per launch.
// Keys box/corners, box/pairs, box/aligned, box/key, box/mask, box/reduce.
enum BoxInst { kBoxCorners = 0, kBoxPairs, kBoxAligned, kBoxKey, kBoxMask, kBoxReduce, kBoxCount };
extern std::atomic<long long> g_box_launches[kBoxCount];
inline void count_box(BoxInst i) { g_box_launches[i].fetch_add(1, std::memory_order_relaxed); }

// voxel serialisation (serialize.hip): keys once per spx_curve_keys call, sort once per sorted order, offsets once per
// spx_serialize call, plan once per spx_patch_plan call, bwd once per spx_patch_rows_bwd call.
// Keys serialize/keys, serialize/sort, serialize/offsets, serialize/plan, serialize/bwd.
enum SerializeInst { kSerKeys = 0, kSerSort, kSerOffsets, kSerPlan, kSerBwd, kSerCount };
extern std::atomic<long long> g_serialize_launches[kSerCount];
inline void count_serialize(SerializeInst i) { g_serialize_launches[i].fetch_add(1, std::memory_order_relaxed); }

// voxel pruning (select.hip): one counter per pass, counted once per launch (a top-k call counts hist and pick four
// times each: once per digit).
// Keys select/score, select/hist, select/pick, select/ties, select/flags, select/count, select/scan, select/scatter,
// select/map.
enum SelectInst { kSelScore = 0, kSelHist, kSelPick, kSelTies, kSelFlags, kSelCount, kSelScan, kSelScatter, kSelMap,
                  kSelInstCount };
extern std::atomic<long long> g_select_launches[kSelInstCount];
inline void count_select(SelectInst i) { g_select_launches[i].fetch_add(1, std::memory_order_relaxed); }

// pooling (pool.hip): one counter per kernel instance, op x dtype x piece.
// Keys pool/<op>/<dt>/<piece>: op max_fwd | max_bwd | avg_fwd | avg_bwd (PoolOp order), dt f16 | bf16 | f32 | f64 | i8,
// piece v (16-byte pieces) | s (one element).  int8 is built for max_fwd only; its other keys count 0.
enum PoolDt { kPoolF16 = 0, kPoolBf16, kPoolF32, kPoolF64, kPoolI8, kPoolDts };
constexpr int kPoolOps = 4, kPoolCount = kPoolOps * kPoolDts * 2;
extern std::atomic<long long> g_pool_launches[kPoolCount];
constexpr int pool_slot(int op, int dt, bool scalar) { return (op * kPoolDts + dt) * 2 + (scalar ? 1 : 0); }
inline void count_pool(int op, int dt, bool scalar) {
  g_pool_launches[pool_slot(op, dt, scalar)].fetch_add(1, std::memory_order_relaxed);
}

// rulebook builders over the hash table (rulebook_subm.hip: spx_subm_rulebook; rulebook_conv.hip: spx_conv_rulebook_count /
// _fill / _static):
// one counter per dispatch decision, counted on the host where the launch is issued.
// Keys rulebook/<pass>: subm_probe3 | subm_probe4 | subm_probe5 (form of the SubM probe pass), subm_mask_pass (masks
// from a pass over the finished table), subm_lists (lists from the probe's group counts), native_lists_v1 (SubM lists by
// count -> scan -> scatter), conv3/1 | conv3/2 | conv3/4 | conv3/8 (compact-candidate passes, by candidates per input)
// and conv_generic (thread per (offset, input)) -- both once in the count pass and once in the fill pass --,
// conv_lists_v1 (conv lists by count -> scan -> scatter), conv_shrunk (table sized for an expectation), conv_retry
// (count pass run again at the guaranteed size after an overflow), conv3_shares/1 | 2 | 4 | 8 (grid.y of the compact
// passes, once per count pass and once per fill pass: the two must agree).
enum RulebookPass { kRbSubmProbe3 = 0, kRbSubmProbe4, kRbSubmProbe5, kRbSubmMaskPass, kRbSubmLists, kRbNativeListsV1,
                    kRbConv3_1, kRbConv3_2, kRbConv3_4, kRbConv3_8, kRbConvGeneric, kRbConvListsV1, kRbConvShrunk,
                    kRbConvRetry, kRbShares1, kRbShares2, kRbShares4, kRbShares8, kRbCount };
extern std::atomic<long long> g_rulebook_launches[kRbCount];
inline void count_rulebook(RulebookPass p) { g_rulebook_launches[p].fetch_add(1, std::memory_order_relaxed); }
}  // namespace spx

// ---- row orders (rowsort.hip) and the row gather (pointvoxel.hip) ----------------------------------
namespace spx {
// out[i] = src[rows[i]] or the fill element (fill16: it repeated over 16 bytes) where rows[i] is outside [0, n_src);
// rows of C elements of elem_bytes bytes, the bits moved unchanged.  Neither counts nor validates.  0 = ok.
int gather_rows(const void *src, int n_src, const int32_t *rows, long long n_rows, int C, int elem_bytes,
                const void *fill16, void *out, hipStream_t s);
// stable LSD radix argsort behind spx_mask_argsort (rowsort.hip)
size_t radix_argsort_ws_bytes(int n);
int radix_argsort(const uint32_t *keys, int n, int nbits, int32_t *order_out, void *ws, hipStream_t s);
// the same over 64-bit keys (1 .. 64 bits), `sorts` independent sorts of n keys each ([sorts, n] arrays) pass by pass
// together; inverse_out (or null): inverse_out[k, order_out[k, t]] = t
size_t radix_argsort64_ws_bytes(int n, int sorts);
int radix_argsort64(const uint64_t *keys, int n, int sorts, int nbits, int32_t *order_out, int32_t *inverse_out, void *ws,
                    hipStream_t s);

}  // namespace spx
