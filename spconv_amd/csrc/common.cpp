// Host-only pieces of the C ABI: error channel, version, output-shape math.
#include "common.h"

#include <string.h>

#include <mutex>
#include <string>

namespace spx {
namespace {
thread_local std::string g_error;
}

void set_error(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}

namespace {
struct Option {
  char name[48];
  int value;
};
Option g_options[32];
int g_noptions = 0;
std::mutex g_option_mutex;
}  // namespace

std::atomic<long long> g_launches[kFamCount];
std::atomic<long long> g_inst_launches[inst::kCount];
std::atomic<long long> g_hint_launches[kHintCount];
std::atomic<long long> g_f64_launches[kF64Count];
std::atomic<long long> g_dense_launches[kDenseCount];
std::atomic<long long> g_union_launches[kUnionCount];
std::atomic<long long> g_collapse_launches[kCollapseCount];
std::atomic<long long> g_pointvoxel_launches[kPvCount];
std::atomic<long long> g_interp_launches[kInterpCount];
std::atomic<long long> g_query_launches[kQueryCount];
std::atomic<long long> g_sample_launches[kSampleCount];
std::atomic<long long> g_box_launches[kBoxCount];
std::atomic<long long> g_serialize_launches[kSerCount];
std::atomic<long long> g_select_launches[kSelInstCount];
std::atomic<long long> g_pool_launches[kPoolCount];
std::atomic<long long> g_rulebook_launches[kRbCount];

namespace {
// "f16" | "bf16" | "i8" | "f32" -> the kernels' DT code, or -1
int parse_dt(const char *t) {
  static const char *names[inst::kDts] = {"f16", "bf16", "i8", "f32"};
  for (int i = 0; i < inst::kDts; ++i)
    if (strcmp(t, names[i]) == 0) return i;
  return -1;
}

// a decimal token, or -1
int parse_int(const char *t) {
  if (!*t || strlen(t) > 6) return -1;
  int v = 0;
  for (; *t; ++t) {
    if (*t < '0' || *t > '9') return -1;
    v = v * 10 + (*t - '0');
  }
  return v;
}

// slot of an instance key (spx_launch_count), or -1
int instance_slot(const char *key) {
  char buf[96];
  if (strlen(key) >= sizeof(buf)) return -1;
  strcpy(buf, key);
  const char *tok[8];
  int n = 0;
  for (char *c = buf, *start = buf;; ++c) {
    if (*c == '/' || *c == 0) {
      if (n == 8) return -1;
      const bool end = *c == 0;
      *c = 0;
      tok[n++] = start;
      start = c + 1;
      if (end) break;
    }
  }
  const char *fam = tok[0];
  auto is = [&](const char *name, int ntok) { return strcmp(fam, name) == 0 && n == ntok; };
  auto cout_ok = [](int c) { return inst::cout_slot(c) >= 0; };
  if (is("igemm_v4", 7)) {
    const int cout = parse_int(tok[1]), mb = parse_int(tok[2]), dt = parse_dt(tok[3]);
    const int bt = strcmp(tok[4], "bt") == 0 ? 1 : (strcmp(tok[4], "fwd") == 0 ? 0 : -1);
    const int nks = parse_int(tok[5]), pk = parse_int(tok[6]);
    if (!cout_ok(cout) || (mb != 1 && mb != 2) || dt < 0 || bt < 0 || (nks != 1 && nks != 2) || inst::pk_slot(pk) < 0)
      return -1;
    return inst::v4(cout, mb, dt, bt == 1, nks, pk);
  }
  if (is("igemm_v4w", 6)) {                   // igemm_v4w/128/<dt>/<fwd|bt>/<nks>/<pk>
    const int nt = parse_int(tok[1]), dt = parse_dt(tok[2]);
    const int bt = strcmp(tok[3], "bt") == 0 ? 1 : (strcmp(tok[3], "fwd") == 0 ? 0 : -1);
    const int nks = parse_int(tok[4]), pk = parse_int(tok[5]);
    if (nt != 128 || bt < 0 || !inst::v4w_exists(dt, bt == 1, nks, pk)) return -1;
    return inst::v4w(dt, bt == 1, nks, pk);
  }
  if (is("igemm_bwd", 6)) {
    const int cout = parse_int(tok[1]), mb = parse_int(tok[2]), dt = parse_dt(tok[3]);
    const int nks = parse_int(tok[4]), pk = parse_int(tok[5]);
    if (!cout_ok(cout) || (mb != 1 && mb != 2) || dt < 0 || (nks != 1 && nks != 2) || inst::pk_slot(pk) < 0) return -1;
    return inst::bwd(cout, mb, dt, nks, pk);
  }
  if (is("igemm_ws", 2)) return parse_dt(tok[1]) < 0 ? -1 : inst::ws(parse_dt(tok[1]));
  if (is("igemm_bwd_rows", 5)) {
    const int c = parse_int(tok[1]), k = parse_int(tok[2]), dt = parse_dt(tok[3]), w8 = parse_int(tok[4]);
    if ((c != 16 && c != 32) || (k != 16 && k != 32) || dt < 0 || (w8 != 0 && w8 != 1)) return -1;
    return inst::bwd_rows(c, k, dt, w8 == 1);
  }
  if (is("wgrad_tr", 3)) {
    const int dt = parse_dt(tok[1]), sl = parse_int(tok[2]);
    return dt < 0 || inst::sl_slot(sl) < 0 ? -1 : inst::wgrad_tr(dt, sl);
  }
  if (is("wgrad_f32", 1)) return inst::kWgradF32;
  if (is("wgrad_mfma", 2)) return parse_dt(tok[1]) < 0 ? -1 : inst::wgrad_mfma(parse_dt(tok[1]));
  if (is("wgrad_generic", 2)) return parse_dt(tok[1]) < 0 ? -1 : inst::wgrad_generic(parse_dt(tok[1]));
  if (is("generic", 2)) return parse_dt(tok[1]) < 0 ? -1 : inst::generic(parse_dt(tok[1]));
  if (is("gen1", 3)) {
    const int cout = parse_int(tok[1]), dt = parse_dt(tok[2]);
    return !cout_ok(cout) || dt < 0 ? -1 : inst::gen1(cout, dt);
  }
  return -1;
}

// counter of a float64 key (spx_launch_count), or null
std::atomic<long long> *f64_counter(const char *key) {
  if (strcmp(key, "igemm_f64/fwd") == 0) return &g_f64_launches[kF64Fwd];
  if (strcmp(key, "igemm_f64/dgrad") == 0) return &g_f64_launches[kF64Dgrad];
  if (strcmp(key, "wgrad_f64") == 0) return &g_f64_launches[kF64Wgrad];
  if (strcmp(key, "pool/f64") == 0) return &g_f64_launches[kF64Pool];
  return nullptr;
}

// counter of a dense-conversion key (spx_launch_count), or null
std::atomic<long long> *dense_counter(const char *key) {
  static const char *names[kDenseCount] = {"dense/map", "dense/scatter_cl", "dense/scatter_cf", "dense/gather_cl",
                                           "dense/gather_cf", "dense/compact"};
  for (int i = 0; i < kDenseCount; ++i)
    if (strcmp(key, names[i]) == 0) return &g_dense_launches[i];
  return nullptr;
}

// counter of a misaligned-add key (spx_launch_count), or null
std::atomic<long long> *union_counter(const char *key) {
  static const char *names[kUnionCount] = {"union/mark", "union/prefix", "union/claim", "union/fill", "union/add_fwd",
                                           "union/add_bwd"};
  for (int i = 0; i < kUnionCount; ++i)
    if (strcmp(key, names[i]) == 0) return &g_union_launches[i];
  return nullptr;
}

// counter of an axis-collapse key (spx_launch_count), or null
std::atomic<long long> *collapse_counter(const char *key) {
  static const char *names[kCollapseCount] = {"collapse/mark", "collapse/prefix", "collapse/rank", "collapse/list",
                                              "collapse/fwd", "collapse/bwd"};
  for (int i = 0; i < kCollapseCount; ++i)
    if (strcmp(key, names[i]) == 0) return &g_collapse_launches[i];
  return nullptr;
}

// counter of a point <-> voxel key (spx_launch_count), or null
std::atomic<long long> *pointvoxel_counter(const char *key) {
  static const char *names[kPvCount] = {"pointvoxel/groups", "pointvoxel/gather", "pointvoxel/decorate"};
  for (int i = 0; i < kPvCount; ++i)
    if (strcmp(key, names[i]) == 0) return &g_pointvoxel_launches[i];
  return nullptr;
}

// counter of a voxel-serialisation key (spx_launch_count), or null
std::atomic<long long> *serialize_counter(const char *key) {
  static const char *names[kSerCount] = {"serialize/keys", "serialize/sort", "serialize/offsets", "serialize/plan",
                                         "serialize/bwd"};
  for (int i = 0; i < kSerCount; ++i)
    if (strcmp(key, names[i]) == 0) return &g_serialize_launches[i];
  return nullptr;
}

// counter of a trilinear-devoxelisation key (spx_launch_count), or null
std::atomic<long long> *interp_counter(const char *key) {
  static const char *names[kInterpCount] = {"interp/corners_ranked", "interp/corners_hash", "interp/fwd", "interp/bwd"};
  for (int i = 0; i < kInterpCount; ++i)
    if (strcmp(key, names[i]) == 0) return &g_interp_launches[i];
  return nullptr;
}

// counter of a voxel-query key (spx_launch_count), or null
std::atomic<long long> *query_counter(const char *key) {
  static const char *names[kQueryCount] = {"query/ranked", "query/hash", "query/group_fwd", "query/group_bwd"};
  for (int i = 0; i < kQueryCount; ++i)
    if (strcmp(key, names[i]) == 0) return &g_query_launches[i];
  return nullptr;
}

// counter of a rotated-box key (spx_launch_count), or null
std::atomic<long long> *box_counter(const char *key) {
  static const char *names[kBoxCount] = {"box/corners", "box/pairs", "box/aligned", "box/key", "box/mask", "box/reduce"};
  for (int i = 0; i < kBoxCount; ++i)
    if (strcmp(key, names[i]) == 0) return &g_box_launches[i];
  return nullptr;
}

// counter of a raw-point sampling key (spx_launch_count), or null
std::atomic<long long> *sample_counter(const char *key) {
  static const char *names[kSampleCount] = {"sample/fps", "sample/ball_query", "sample/knn_query"};
  for (int i = 0; i < kSampleCount; ++i)
    if (strcmp(key, names[i]) == 0) return &g_sample_launches[i];
  return nullptr;
}

// counter of a voxel-pruning key (spx_launch_count), or null
std::atomic<long long> *select_counter(const char *key) {
  static const char *names[kSelInstCount] = {"select/score", "select/hist", "select/pick", "select/ties", "select/flags",
                                             "select/count", "select/scan", "select/scatter", "select/map"};
  for (int i = 0; i < kSelInstCount; ++i)
    if (strcmp(key, names[i]) == 0) return &g_select_launches[i];
  return nullptr;
}

// counter of a rulebook-builder key rulebook/<pass> (spx_launch_count), or null
std::atomic<long long> *rulebook_counter(const char *key) {
  static const char *names[kRbCount] = {"subm_probe3", "subm_probe4", "subm_probe5", "subm_mask_pass", "subm_lists",
                                        "native_lists_v1", "conv3/1", "conv3/2", "conv3/4", "conv3/8", "conv_generic",
                                        "conv_lists_v1", "conv_shrunk", "conv_retry", "conv3_shares/1", "conv3_shares/2",
                                        "conv3_shares/4", "conv3_shares/8"};
  if (strncmp(key, "rulebook/", 9) != 0) return nullptr;
  for (int i = 0; i < kRbCount; ++i)
    if (strcmp(key + 9, names[i]) == 0) return &g_rulebook_launches[i];
  return nullptr;
}

// counter of a pooling key pool/<op>/<dt>/<piece> (spx_launch_count), or null
std::atomic<long long> *pool_counter(const char *key) {
  static const char *ops[kPoolOps] = {"max_fwd", "max_bwd", "avg_fwd", "avg_bwd"};
  static const char *dts[kPoolDts] = {"f16", "bf16", "f32", "f64", "i8"};
  if (strncmp(key, "pool/", 5) != 0) return nullptr;
  key += 5;
  for (int op = 0; op < kPoolOps; ++op) {
    const size_t n = strlen(ops[op]);
    if (strncmp(key, ops[op], n) != 0 || key[n] != '/') continue;
    const char *rest = key + n + 1;
    for (int dt = 0; dt < kPoolDts; ++dt) {
      const size_t m = strlen(dts[dt]);
      if (strncmp(rest, dts[dt], m) != 0 || rest[m] != '/') continue;
      const char *piece = rest + m + 1;
      if (strcmp(piece, "v") == 0) return &g_pool_launches[pool_slot(op, dt, false)];
      if (strcmp(piece, "s") == 0) return &g_pool_launches[pool_slot(op, dt, true)];
    }
  }
  return nullptr;
}
}  // namespace

int option_int(const char *name, int dflt) {
  {
    std::lock_guard<std::mutex> lock(g_option_mutex);
    for (int i = 0; i < g_noptions; ++i)
      if (strcmp(g_options[i].name, name) == 0) return g_options[i].value;
  }
  return env_int(name, dflt);
}
}  // namespace spx

extern "C" {

int spx_set_option(const char *name_h, int value) {
  SPX_CHECK(name_h && strlen(name_h) < sizeof(spx::Option::name), "bad option name");
  std::lock_guard<std::mutex> lock(spx::g_option_mutex);
  for (int i = 0; i < spx::g_noptions; ++i)
    if (strcmp(spx::g_options[i].name, name_h) == 0) {
      spx::g_options[i].value = value;
      return 0;
    }
  SPX_CHECK(spx::g_noptions < 32, "too many options");
  strcpy(spx::g_options[spx::g_noptions].name, name_h);
  spx::g_options[spx::g_noptions++].value = value;
  return 0;
}

const char *spx_last_error(void) { return spx::g_error.c_str(); }

long long spx_launch_count(const char *family_h) {
  static const char *names[spx::kFamCount] = {"igemm_v4", "igemm_ws", "igemm_bwd", "igemm_bwd_rows", "igemm_i8_stream",
                                              "generic", "wgrad_stage2", "wgrad_stage2_batch", "igemm_f64",
                                              "igemm_v4w"};
  if (!family_h) return -1;
  for (int i = 0; i < spx::kFamCount; ++i)
    if (strcmp(names[i], family_h) == 0) return spx::g_launches[i].load(std::memory_order_relaxed);
  if (strcmp(family_h, "sparse_hint/v4") == 0) return spx::g_hint_launches[spx::kHintV4].load(std::memory_order_relaxed);
  if (strcmp(family_h, "sparse_hint/bwd") == 0) return spx::g_hint_launches[spx::kHintBwd].load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::f64_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::dense_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::union_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::collapse_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::pointvoxel_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::interp_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::query_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::sample_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::box_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::serialize_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::select_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::pool_counter(family_h)) return c->load(std::memory_order_relaxed);
  if (std::atomic<long long> *c = spx::rulebook_counter(family_h)) return c->load(std::memory_order_relaxed);
  const int slot = spx::instance_slot(family_h);
  return slot < 0 ? -1 : spx::g_inst_launches[slot].load(std::memory_order_relaxed);
}

int spx_version(void) { return 1000; }

// ops.get_conv_output_size / get_deconv_output_size (pytorch/ops.py:73-96)
int spx_conv_out_shape(int ndim, const int *in_shape, const int *ksize, const int *stride,
                       const int *padding, const int *dilation, const int *out_padding,
                       int transposed, int *out_shape) {
  SPX_CHECK(ndim >= 1 && ndim <= SPX_MAX_NDIM, "ndim must be in [1,4], got %d", ndim);
  for (int i = 0; i < ndim; ++i) {
    SPX_CHECK(stride[i] > 0, "stride must be positive");
    if (transposed) {
      SPX_CHECK(ksize[i] != -1, "deconv don't support kernel_size < 0");
      out_shape[i] = (in_shape[i] - 1) * stride[i] - 2 * padding[i] + ksize[i] +
                     (out_padding ? out_padding[i] : 0);
    } else if (ksize[i] == -1) {
      out_shape[i] = 1;
    } else {
      const int num = in_shape[i] + 2 * padding[i] - dilation[i] * (ksize[i] - 1) - 1;
      int q = num / stride[i];
      if (num % stride[i] != 0 && num < 0) --q;  // python floor division
      out_shape[i] = q + 1;
    }
  }
  return 0;
}

}  // extern "C"
