// Stand-alone ASan/UBSan harness for the host pod census
// (pod_census_host in ops/csrc/kvidx_common.h, the core of the
// cpu_pod_census op).  torch-free:
//
//   make asan   (exits nonzero on any finding)
//
// meta, pods and e_meta are heap arrays sized exactly capacity (x
// pods_per_key for pods) and counts is exactly num_pods * n_tiers words,
// so a read past a table array or a bin past the histogram is a sanitizer
// report.  The arrays the census must not look at are null.  Every
// pods_per_key from 1 to 17 runs with fleets of 1, 64, 130 and MAX_PODS
// pods, 1 to MAX_TIERS tiers, entries whose id or tier lies past them, and
// ids at every edge; the result is held against a direct recount.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../llmd_kvcache_amd/ops/csrc/kvidx_common.h"

using namespace kvidx;

static int fail(const char* what, int P, int num_pods, int n_tiers) {
  fprintf(stderr, "census check failed: %s (P=%d pods=%d tiers=%d)\n", what, P,
          num_pods, n_tiers);
  return 1;
}

int main() {
  std::mt19937_64 rng(777);
  const uint64_t cap = 64;
  const uint32_t edge_ids[] = {0, 1, 63, 64, 129, 130, 4094, 4095, 4096,
                               0x00FFFFFEu};
  for (int P = 1; P <= 17; ++P) {
    for (int num_pods : {1, 64, 130, (int)MAX_PODS}) {
      for (int n_tiers = 1; n_tiers <= MAX_TIERS; ++n_tiers) {
        for (int64_t model_id : {(int64_t)-1, (int64_t)0, (int64_t)1}) {
          std::vector<uint32_t> meta(cap), e_meta(cap), pods(cap * P);
          for (uint64_t i = 0; i < cap; ++i) {
            const uint32_t kinds[] = {
                0u, META_OCC | META_TOMB | (uint32_t)(i & 1),
                META_OCC | (uint32_t)(i & 1), META_OCC | (uint32_t)(i & 1),
                (uint32_t)(i & 1) /* model bits, never published */};
            meta[i] = kinds[rng() % 5];
            e_meta[i] = kinds[rng() % 5];
            const bool full = rng() % 4 == 0;
            for (int k = 0; k < P; ++k) {
              const uint64_t r = rng();
              if (!full && r % 3 == 0) continue;  // empty entry
              const uint32_t pid =
                  (r % 3 == 1) ? edge_ids[(r >> 8) % 10]
                               : (uint32_t)((r >> 8) % (num_pods + 3u));
              pods[i * P + k] = make_pod_entry(pid, (uint32_t)((r >> 40) % 4));
            }
          }
          const auto meta0 = meta, e_meta0 = e_meta, pods0 = pods;
          Table v{nullptr,     meta.data(),   nullptr, pods.data(),
                  nullptr,     e_meta.data(), nullptr, cap - 1,
                  P};
          std::vector<int64_t> counts(num_pods * n_tiers, -1);
          CensusSummary got;
          got.entries = -1;
          pod_census_host(v, model_id, num_pods, n_tiers, counts.data(), &got);

          std::vector<int64_t> want(num_pods * n_tiers, 0);
          CensusSummary w;
          auto match = [&](uint32_t m) {
            return (m & 0x80000000u) &&
                   (model_id < 0 || (int64_t)(m & 0xFFFF) == model_id);
          };
          for (uint64_t i = 0; i < cap; ++i) {
            if (match(e_meta0[i]) && !(e_meta0[i] & 0x40000000u))
              ++w.emap_occupied;
            if (!match(meta0[i])) continue;
            if (meta0[i] & 0x40000000u) {
              ++w.keys_tombstoned;
              continue;
            }
            ++w.keys_live;
            int nz = 0;
            for (int k = 0; k < P; ++k) {
              const uint32_t e = pods0[i * P + k];
              if (!e) continue;
              ++nz;
              const uint32_t pid = (e & 0x00FFFFFFu) - 1, tier = e >> 24;
              if (pid < (uint32_t)num_pods && tier < (uint32_t)n_tiers)
                ++want[pid * n_tiers + tier];
              else
                ++w.entries_unknown;
            }
            w.entries += nz;
            w.keys_full += nz == P;
          }
          if (counts != want) return fail("counts", P, num_pods, n_tiers);
          if (got.keys_live != w.keys_live ||
              got.keys_tombstoned != w.keys_tombstoned ||
              got.keys_full != w.keys_full || got.entries != w.entries ||
              got.entries_unknown != w.entries_unknown ||
              got.emap_occupied != w.emap_occupied)
            return fail("summary", P, num_pods, n_tiers);
          int64_t sum = 0;
          for (int64_t c : counts) sum += c;
          if (sum + got.entries_unknown != got.entries)
            return fail("entries != sum(counts) + unknown", P, num_pods,
                        n_tiers);
          if (meta != meta0 || e_meta != e_meta0 || pods != pods0)
            return fail("table written", P, num_pods, n_tiers);
        }
      }
    }
  }
  printf("census_asan_check OK\n");
  return 0;
}
