// Stand-alone ASan/UBSan harness for the host purge-by-pod sweep
// (purge_pods_host in ops/csrc/kvidx_common.h, the core of the
// cpu_purge_pods op).  torch-free:
//
//   make asan   (exits nonzero on any finding)
//
// The table is seven heap arrays sized exactly capacity (x pods_per_key
// for pods) and the bitmap is exactly W words, so a read or write one
// element past any of them is a sanitizer report.  Every pods_per_key
// from 1 to 17 runs with bitmaps of 1, 2 and 64 words, entries whose ids
// lie past the bitmap's end, and ids at every word edge; the counts are
// held against a direct recount.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../llmd_kvcache_amd/ops/csrc/kvidx_common.h"

using namespace kvidx;

static int fail(const char* what, int P, int W) {
  fprintf(stderr, "purge check failed: %s (P=%d W=%d)\n", what, P, W);
  return 1;
}

int main() {
  std::mt19937_64 rng(4242);
  const uint64_t cap = 64;
  const uint32_t edge_ids[] = {0, 1, 62, 63, 64, 65, 126, 127, 128,
                               4094, 4095, 4096, 0x00FFFFFEu};
  for (int P = 1; P <= 17; ++P) {
    for (int W : {1, 2, 64}) {
      for (int64_t model_id : {(int64_t)-1, (int64_t)0, (int64_t)1}) {
        std::vector<uint64_t> keys(cap), e_keys(cap), e_vals(cap);
        std::vector<uint32_t> meta(cap), e_meta(cap), pods(cap * P);
        std::vector<int32_t> stamp(cap, 3);
        std::vector<uint64_t> words(W);
        for (auto& w : words) w = rng() & rng();  // about a quarter set
        words[0] |= 1;                            // pod 0 always purged
        for (uint64_t i = 0; i < cap; ++i) {
          keys[i] = e_keys[i] = rng() | 1;
          e_vals[i] = rng();
          const int kind = (int)(rng() % 5);
          meta[i] = kind == 0   ? 0u
                    : kind == 1 ? (META_OCC | META_TOMB | (uint32_t)(i & 1))
                                : (META_OCC | (uint32_t)(i & 1));
          e_meta[i] = META_OCC;
          for (int k = 0; k < P; ++k) {
            const uint64_t r = rng();
            if (r % 3 == 0) continue;  // empty slot
            const uint32_t pid = (r % 3 == 1)
                                     ? edge_ids[(r >> 8) % 13]
                                     : (uint32_t)((r >> 8) % (64u * W + 70u));
            pods[i * P + k] = make_pod_entry(pid, (uint32_t)((r >> 40) % 4));
          }
        }
        const auto meta0 = meta;
        const auto pods0 = pods;
        const auto keys0 = keys;
        const auto stamp0 = stamp;
        const auto e_keys0 = e_keys;
        const auto e_meta0 = e_meta;
        const auto e_vals0 = e_vals;
        Table v{keys.data(),   meta.data(),   stamp.data(), pods.data(),
                e_keys.data(), e_meta.data(), e_vals.data(), cap - 1, P};
        const PurgeCounts got = purge_pods_host(v, words.data(), W, model_id);

        // recount from the copies
        int64_t entries = 0, tombs = 0;
        for (uint64_t i = 0; i < cap; ++i) {
          const uint32_t m = meta0[i];
          const bool elig = (m & META_OCC) &&
                            (model_id < 0 || (int64_t)(m & 0xFFFF) == model_id);
          int cleared = 0, left = 0;
          for (int k = 0; k < P; ++k) {
            const uint32_t e = pods0[i * P + k];
            const uint32_t pid = (e & 0x00FFFFFFu) - 1;
            const bool sel = e != 0 && pid < 64u * W &&
                             ((words[pid / 64] >> (pid % 64)) & 1);
            if (elig && sel) {
              ++cleared;
              if (pods[i * P + k] != 0) return fail("entry not cleared", P, W);
            } else {
              if (e) ++left;
              if (pods[i * P + k] != e) return fail("entry changed", P, W);
            }
          }
          entries += cleared;
          const bool tomb_now = cleared && !left && !(m & META_TOMB);
          tombs += tomb_now;
          if (meta[i] != (tomb_now ? (m | META_TOMB) : m))
            return fail("meta", P, W);
        }
        if (got.entries_cleared != entries || got.keys_tombstoned != tombs)
          return fail("counts", P, W);
        if (keys != keys0 || stamp != stamp0 || e_keys != e_keys0 ||
            e_meta != e_meta0 || e_vals != e_vals0)
          return fail("untouched arrays", P, W);
        // a second sweep finds nothing
        const PurgeCounts again =
            purge_pods_host(v, words.data(), W, model_id);
        if (again.entries_cleared || again.keys_tombstoned)
          return fail("second sweep", P, W);
      }
    }
  }
  printf("purge_asan_check OK\n");
  return 0;
}
