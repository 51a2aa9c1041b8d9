// Stand-alone host check of the launch-counter table (tests/test_counters_host.py builds and runs it).  Links
// counters.cpp and common.cpp only, as plain host C++; never opens a GPU.  Keys come on stdin, one per line.
//   --classify    print the keys spx_launch_count accepts (answer >= 0), in input order
//   --bijection   stdin is the inventory of every key: bump each storage slot in turn and see which keys move
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "counters.h"
#include "spconv_amd.h"

static std::vector<std::string> read_keys() {
  std::vector<std::string> keys;
  char line[512];
  while (fgets(line, sizeof(line), stdin)) {
    line[strcspn(line, "\n")] = 0;
    keys.push_back(line);
  }
  return keys;
}

static int classify(const std::vector<std::string> &keys) {
  for (const std::string &k : keys)
    if (spx_launch_count(k.c_str()) >= 0) puts(k.c_str());
  return 0;
}

#define FAIL(...) (fprintf(stderr, __VA_ARGS__), fputc('\n', stderr), 1)

static int bijection(const std::vector<std::string> &keys) {
  const int n = (int)keys.size();
  std::vector<long long> seen(n);
  std::vector<int> moved(n, 0);
  for (int i = 0; i < n; ++i) {
    seen[i] = spx_launch_count(keys[i].c_str());
    if (seen[i] != 0) return FAIL("inventory key %s answers %lld before any count", keys[i].c_str(), seen[i]);
  }
  // the slots no key reaches: igemm_v4w instances that are never built
  std::vector<bool> unbuilt_v4w(spx::kCounterSlots, false);
  for (int dt = 0; dt < spx::inst::kDts; ++dt)
    for (int bt = 0; bt < 2; ++bt)
      for (int nks = 1; nks <= 2; ++nks)
        for (int pk = 1; pk <= 4; pk *= 2)
          if (!spx::inst::v4w_exists(dt, bt == 1, nks, pk)) unbuilt_v4w[spx::kInstBase + spx::inst::v4w(dt, bt == 1, nks, pk)] = true;
  int dead = 0, dead_outside_v4w = 0;
  for (int s = 0; s < spx::kCounterSlots; ++s) {
    spx::g_counters[s].fetch_add(1, std::memory_order_relaxed);
    int changed = -1;
    for (int i = 0; i < n; ++i) {
      const long long v = spx_launch_count(keys[i].c_str());
      if (v == seen[i]) continue;
      if (v != seen[i] + 1) return FAIL("slot %d moved %s by %lld", s, keys[i].c_str(), v - seen[i]);
      if (changed >= 0) return FAIL("slot %d moved %s and %s", s, keys[changed].c_str(), keys[i].c_str());
      changed = i;
      seen[i] = v;
    }
    if (s < spx::kNamed && (changed < 0 || keys[changed] != spx::counter_name(s)))
      return FAIL("named slot %d is declared as %s but moved %s", s, spx::counter_name(s),
                  changed < 0 ? "nothing" : keys[changed].c_str());
    if (changed >= 0) {
      ++moved[changed];
    } else {
      ++dead;
      if (!unbuilt_v4w[s]) ++dead_outside_v4w;
    }
  }
  for (int i = 0; i < n; ++i)
    if (moved[i] != 1) return FAIL("key %s was moved by %d slots", keys[i].c_str(), moved[i]);
  printf("slots %d named %d keys %d dead %d dead_outside_v4w %d\n", spx::kCounterSlots, (int)spx::kNamed, n, dead,
         dead_outside_v4w);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "--classify") == 0) return classify(read_keys());
  if (argc == 2 && strcmp(argv[1], "--bijection") == 0) return bijection(read_keys());
  return FAIL("usage: %s --classify | --bijection  (keys on stdin)", argv[0]);
}
