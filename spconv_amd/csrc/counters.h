// Launch counters (diagnostics: which kernel a call dispatched; spx_launch_count, whose comment in the public header is
// the contract for every key).  One storage array in three segments: the fixed-name keys declared below, the gather-GEMM
// template instances (inst::) and the pooling instances.  A count is one relaxed increment of a fixed slot at the launch
// site; counters.cpp turns a key into its slot.
#pragma once
#include <atomic>

namespace spx {

// Every fixed-name key, declared ONCE: X(enumerator, key).  A new key is one entry here.
#define SPX_COUNTERS(X)                                                                                               \
  X(kFamV4, "igemm_v4") X(kFamWs, "igemm_ws") X(kFamBwdFused, "igemm_bwd") X(kFamBwdRows, "igemm_bwd_rows")           \
  X(kFamI8Stream, "igemm_i8_stream") X(kFamGeneric, "generic") X(kFamStage2, "wgrad_stage2")                          \
  X(kFamStage2Batch, "wgrad_stage2_batch") X(kFamF64, "igemm_f64") X(kFamV4w, "igemm_v4w")                            \
  X(kHintV4, "sparse_hint/v4") X(kHintBwd, "sparse_hint/bwd")                                                         \
  X(kF64Fwd, "igemm_f64/fwd") X(kF64Dgrad, "igemm_f64/dgrad") X(kF64Wgrad, "wgrad_f64") X(kF64Pool, "pool/f64")       \
  X(kDenseMap, "dense/map") X(kDenseScatterCl, "dense/scatter_cl") X(kDenseScatterCf, "dense/scatter_cf")             \
  X(kDenseGatherCl, "dense/gather_cl") X(kDenseGatherCf, "dense/gather_cf") X(kDenseCompact, "dense/compact")         \
  X(kUnionMark, "union/mark") X(kUnionPrefix, "union/prefix") X(kUnionClaim, "union/claim")                           \
  X(kUnionFill, "union/fill") X(kUnionAddFwd, "union/add_fwd") X(kUnionAddBwd, "union/add_bwd")                       \
  X(kCollapseMark, "collapse/mark") X(kCollapsePrefix, "collapse/prefix") X(kCollapseRank, "collapse/rank")           \
  X(kCollapseList, "collapse/list") X(kCollapseFwd, "collapse/fwd") X(kCollapseBwd, "collapse/bwd")                   \
  X(kPvGroups, "pointvoxel/groups") X(kPvGather, "pointvoxel/gather") X(kPvDecorate, "pointvoxel/decorate")           \
  X(kInterpCornersRanked, "interp/corners_ranked") X(kInterpCornersHash, "interp/corners_hash")                       \
  X(kInterpFwd, "interp/fwd") X(kInterpBwd, "interp/bwd")                                                             \
  X(kQueryRanked, "query/ranked") X(kQueryHash, "query/hash") X(kQueryGroupFwd, "query/group_fwd")                    \
  X(kQueryGroupBwd, "query/group_bwd")                                                                                \
  X(kSampleFps, "sample/fps") X(kSampleBallQuery, "sample/ball_query") X(kSampleKnnQuery, "sample/knn_query")         \
  X(kBoxCorners, "box/corners") X(kBoxPairs, "box/pairs") X(kBoxAligned, "box/aligned") X(kBoxKey, "box/key")         \
  X(kBoxMask, "box/mask") X(kBoxReduce, "box/reduce")                                                                 \
  X(kSerKeys, "serialize/keys") X(kSerSort, "serialize/sort") X(kSerOffsets, "serialize/offsets")                     \
  X(kSerPlan, "serialize/plan") X(kSerBwd, "serialize/bwd")                                                           \
  X(kSelScore, "select/score") X(kSelHist, "select/hist") X(kSelPick, "select/pick") X(kSelTies, "select/ties")       \
  X(kSelFlags, "select/flags") X(kSelCount, "select/count") X(kSelScan, "select/scan")                                \
  X(kSelScatter, "select/scatter") X(kSelMap, "select/map")                                                           \
  X(kRbSubmProbe3, "rulebook/subm_probe3") X(kRbSubmProbe4, "rulebook/subm_probe4")                                   \
  X(kRbSubmProbe5, "rulebook/subm_probe5") X(kRbSubmMaskPass, "rulebook/subm_mask_pass")                              \
  X(kRbSubmLists, "rulebook/subm_lists") X(kRbNativeListsV1, "rulebook/native_lists_v1")                              \
  X(kRbConv3_1, "rulebook/conv3/1") X(kRbConv3_2, "rulebook/conv3/2") X(kRbConv3_4, "rulebook/conv3/4")               \
  X(kRbConv3_8, "rulebook/conv3/8") X(kRbConvGeneric, "rulebook/conv_generic")                                        \
  X(kRbConvListsV1, "rulebook/conv_lists_v1") X(kRbConvShrunk, "rulebook/conv_shrunk")                                \
  X(kRbConvRetry, "rulebook/conv_retry") X(kRbShares1, "rulebook/conv3_shares/1")                                     \
  X(kRbShares2, "rulebook/conv3_shares/2") X(kRbShares4, "rulebook/conv3_shares/4")                                   \
  X(kRbShares8, "rulebook/conv3_shares/8")

#define SPX_COUNTER_ENUM(e, key) e,
enum Counter { SPX_COUNTERS(SPX_COUNTER_ENUM) kNamed };
#undef SPX_COUNTER_ENUM

// Gather-GEMM template instances: each a slot whose index is a constant expression of its template parameters, so a
// launch site formats nothing.  dt codes are the kernels' DT parameter: 0 f16, 1 bf16, 2 i8, 3 f32.
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

// Pooling instances (pool.hip), op x dtype x piece: op in PoolOp order, piece v (16-byte pieces) | s (one element).
enum PoolDt { kPoolF16 = 0, kPoolBf16, kPoolF32, kPoolF64, kPoolI8, kPoolDts };
constexpr int kPoolOps = 4, kPoolCount = kPoolOps * kPoolDts * 2;
constexpr int pool_slot(int op, int dt, bool scalar) { return (op * kPoolDts + dt) * 2 + (scalar ? 1 : 0); }

constexpr int kInstBase = kNamed, kPoolBase = kInstBase + inst::kCount, kCounterSlots = kPoolBase + kPoolCount;
extern std::atomic<long long> g_counters[kCounterSlots];

inline void count(Counter c) { g_counters[c].fetch_add(1, std::memory_order_relaxed); }
template <int I>
inline void count_inst() {
  static_assert(I >= 0 && I < inst::kCount, "instance counter slot");
  g_counters[kInstBase + I].fetch_add(1, std::memory_order_relaxed);
}
inline void count_pool(int op, int dt, bool scalar) {
  g_counters[kPoolBase + pool_slot(op, dt, scalar)].fetch_add(1, std::memory_order_relaxed);
}

// Key of a named slot (0 <= c < kNamed), as declared above; slot of a key in g_counters, or -1.
const char *counter_name(int c);
int counter_slot(const char *key);

}  // namespace spx
