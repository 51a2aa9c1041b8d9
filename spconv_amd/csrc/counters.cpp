// Launch counters: the storage and the key -> slot lookup behind spx_launch_count.  Host only.
#include "counters.h"

#include <string.h>

#include "../../include/spconv_amd.h"

namespace spx {
std::atomic<long long> g_counters[kCounterSlots];

namespace {
#define SPX_COUNTER_NAME(e, key) key,
const char *const kNames[] = {SPX_COUNTERS(SPX_COUNTER_NAME)};
#undef SPX_COUNTER_NAME
static_assert(sizeof(kNames) / sizeof(kNames[0]) == kNamed, "one name per enumerator");

// index of a token in a list of names, or -1
template <int N>
int index_of(const char *t, const char *const (&names)[N]) {
  for (int i = 0; i < N; ++i)
    if (strcmp(t, names[i]) == 0) return i;
  return -1;
}

// "f16" | "bf16" | "i8" | "f32" -> the kernels' DT code, or -1
int parse_dt(const char *t) {
  static const char *const names[inst::kDts] = {"f16", "bf16", "i8", "f32"};
  return index_of(t, names);
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

// "fwd" | "bt" -> 0 | 1, or -1
int parse_bt(const char *t) { return strcmp(t, "bt") == 0 ? 1 : (strcmp(t, "fwd") == 0 ? 0 : -1); }

// slot in the instance segment of the n tokens of an instance key, or -1
int instance_slot(const char *const *tok, int n) {
  auto is = [&](const char *name, int ntok) { return strcmp(tok[0], name) == 0 && n == ntok; };
  auto cout_ok = [](int c) { return inst::cout_slot(c) >= 0; };
  auto dt_slot = [&](int base) { return parse_dt(tok[1]) < 0 ? -1 : base + parse_dt(tok[1]); };
  if (is("igemm_v4", 7)) {
    const int cout = parse_int(tok[1]), mb = parse_int(tok[2]), dt = parse_dt(tok[3]), bt = parse_bt(tok[4]);
    const int nks = parse_int(tok[5]), pk = parse_int(tok[6]);
    if (!cout_ok(cout) || (mb != 1 && mb != 2) || dt < 0 || bt < 0 || (nks != 1 && nks != 2) || inst::pk_slot(pk) < 0)
      return -1;
    return inst::v4(cout, mb, dt, bt == 1, nks, pk);
  }
  if (is("igemm_v4w", 6)) {                   // igemm_v4w/128/<dt>/<fwd|bt>/<nks>/<pk>
    const int nt = parse_int(tok[1]), dt = parse_dt(tok[2]), bt = parse_bt(tok[3]);
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
  if (is("igemm_ws", 2)) return dt_slot(inst::kWs);
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
  if (is("wgrad_mfma", 2)) return dt_slot(inst::kWgradMfma);
  if (is("wgrad_generic", 2)) return dt_slot(inst::kWgradGeneric);
  if (is("generic", 2)) return dt_slot(inst::kGeneric);
  if (is("gen1", 3)) {
    const int cout = parse_int(tok[1]), dt = parse_dt(tok[2]);
    return !cout_ok(cout) || dt < 0 ? -1 : inst::gen1(cout, dt);
  }
  return -1;
}

// slot in the pooling segment of the tokens of pool/<op>/<dt>/<piece>, or -1
int pool_key_slot(const char *const *tok, int n) {
  static const char *const ops[kPoolOps] = {"max_fwd", "max_bwd", "avg_fwd", "avg_bwd"};
  static const char *const dts[kPoolDts] = {"f16", "bf16", "f32", "f64", "i8"};
  static const char *const pieces[2] = {"v", "s"};
  if (n != 4 || strcmp(tok[0], "pool") != 0) return -1;
  const int op = index_of(tok[1], ops), dt = index_of(tok[2], dts), piece = index_of(tok[3], pieces);
  return op < 0 || dt < 0 || piece < 0 ? -1 : pool_slot(op, dt, piece == 1);
}
}  // namespace

const char *counter_name(int c) { return c >= 0 && c < kNamed ? kNames[c] : nullptr; }

int counter_slot(const char *key) {
  const int named = index_of(key, kNames);
  if (named >= 0) return named;
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
  const int i = instance_slot(tok, n);
  if (i >= 0) return kInstBase + i;
  const int p = pool_key_slot(tok, n);
  return p < 0 ? -1 : kPoolBase + p;
}
}  // namespace spx

extern "C" long long spx_launch_count(const char *family_h) {
  const int slot = family_h ? spx::counter_slot(family_h) : -1;
  return slot < 0 ? -1 : spx::g_counters[slot].load(std::memory_order_relaxed);
}
