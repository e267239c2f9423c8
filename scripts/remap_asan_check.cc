// Stand-alone ASan/UBSan harness for the host pod-id remap sweep
// (remap_pods_host in ops/csrc/kvidx_common.h, the core of the
// cpu_remap_pods op).  torch-free:
//
//   make asan   (exits nonzero on any finding)
//
// The table is seven heap arrays sized exactly capacity (x pods_per_key
// for pods) and the map is exactly n ints, so a read or write one element
// past any of them is a sanitizer report.  The hand cases of
// tests/pod_remap_cases.py run first, against values written out here;
// then every pods_per_key from 1 to 17 at capacities 1, 2 and 64 runs
// with maps of 1, 66 and 4096 ids (identity, swap, drops, compaction),
// entries whose ids lie past the map's end, and the results are held
// against a direct recount.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../llmd_kvcache_amd/ops/csrc/kvidx_common.h"

using namespace kvidx;

static int fail(const char* what, int P, int n) {
  fprintf(stderr, "remap check failed: %s (P=%d n=%d)\n", what, P, n);
  return 1;
}

static uint32_t E(uint32_t pid, uint32_t tier) {
  return make_pod_entry(pid, tier);
}

struct Arrays {
  std::vector<uint64_t> keys, e_keys, e_vals;
  std::vector<uint32_t> meta, e_meta, pods;
  std::vector<int32_t> stamp;
  int P;
  Arrays(uint64_t cap, int P_)
      : keys(cap, 1), e_keys(cap, 2), e_vals(cap, 3), meta(cap, 0),
        e_meta(cap, META_OCC), pods(cap * P_, 0), stamp(cap, 7), P(P_) {}
  Table view() {
    return Table{keys.data(),   meta.data(),   stamp.data(), pods.data(),
                 e_keys.data(), e_meta.data(), e_vals.data(),
                 (uint64_t)keys.size() - 1, P};
  }
};

// The hand rows (P = 3, capacity 8) and what each map must leave.
static int hand_cases() {
  const int P = 3;
  auto build = [&]() {
    Arrays a(8, P);
    // 0: held only by dropped pods        1: survivors only
    // 2: a dropped and a moved one        3: tombstoned, stale entry
    // 4: another model's row              5: never published
    // 6: an id past a short map           7: empty live row
    const uint32_t meta[8] = {META_OCC, META_OCC, META_OCC,
                              META_OCC | META_TOMB, META_OCC | 1, 0,
                              META_OCC, META_OCC};
    const uint32_t pods[8][3] = {
        {E(0, 0), E(63, 3), E(4095, 0)}, {E(5, 0), E(62, 3), E(4094, 0)},
        {E(63, 2), E(62, 1), 0},         {E(64, 0), 0, 0},
        {E(4095, 3), 0, 0},              {E(0, 0), 0, 0},
        {E(70, 1), 0, E(5, 2)},          {0, 0, 0}};
    for (int i = 0; i < 8; ++i) {
      a.meta[i] = meta[i];
      for (int k = 0; k < P; ++k) a.pods[i * P + k] = pods[i][k];
    }
    return a;
  };
  auto expect = [&](const char* what, Arrays& a, std::vector<int32_t> remap,
                    const uint32_t (*pods)[3], const uint32_t* meta,
                    int64_t moved, int64_t cleared, int64_t tombs) {
    const RemapCounts c =
        remap_pods_host(a.view(), remap.data(), (int)remap.size());
    for (int i = 0; i < 8; ++i) {
      if (a.meta[i] != meta[i]) return fail(what, P, -(i + 1));
      for (int k = 0; k < P; ++k)
        if (a.pods[i * P + k] != pods[i][k]) return fail(what, P, i);
    }
    if (c.entries_moved != moved || c.entries_cleared != cleared ||
        c.keys_tombstoned != tombs)
      return fail(what, P, (int)remap.size());
    return 0;
  };
  std::vector<int32_t> ident(4096);
  for (int i = 0; i < 4096; ++i) ident[i] = i;
  const uint32_t m0[8] = {META_OCC, META_OCC, META_OCC, META_OCC | META_TOMB,
                          META_OCC | 1, 0, META_OCC, META_OCC};
  int rc = 0;
  {  // identity, n = 4096: nothing changes
    Arrays a = build();
    const uint32_t pods[8][3] = {
        {E(0, 0), E(63, 3), E(4095, 0)}, {E(5, 0), E(62, 3), E(4094, 0)},
        {E(63, 2), E(62, 1), 0},         {E(64, 0), 0, 0},
        {E(4095, 3), 0, 0},              {E(0, 0), 0, 0},
        {E(70, 1), 0, E(5, 2)},          {0, 0, 0}};
    rc |= expect("identity", a, ident, pods, m0, 0, 0, 0);
  }
  {  // compaction: 5, 62, 70, 4094 -> 0..3, everything else dropped
    Arrays a = build();
    std::vector<int32_t> r(4096, -1);
    r[5] = 0; r[62] = 1; r[70] = 2; r[4094] = 3;
    const uint32_t pods[8][3] = {
        {0, 0, 0},          {E(0, 0), E(1, 3), E(3, 0)}, {0, E(1, 1), 0},
        {0, 0, 0},          {0, 0, 0},                   {E(0, 0), 0, 0},
        {E(2, 1), 0, E(0, 2)}, {0, 0, 0}};
    const uint32_t meta[8] = {META_OCC | META_TOMB, META_OCC, META_OCC,
                              META_OCC | META_TOMB, META_OCC | META_TOMB | 1,
                              0, META_OCC, META_OCC};
    rc |= expect("compaction", a, r, pods, meta, 6, 6, 2);
  }
  {  // swap 5 <-> 4094: each entry looked up once by its old id
    Arrays a = build();
    std::vector<int32_t> r = ident;
    r[5] = 4094; r[4094] = 5;
    const uint32_t pods[8][3] = {
        {E(0, 0), E(63, 3), E(4095, 0)}, {E(4094, 0), E(62, 3), E(5, 0)},
        {E(63, 2), E(62, 1), 0},         {E(64, 0), 0, 0},
        {E(4095, 3), 0, 0},              {E(0, 0), 0, 0},
        {E(70, 1), 0, E(4094, 2)},       {0, 0, 0}};
    rc |= expect("swap", a, r, pods, m0, 3, 0, 0);
  }
  {  // n = 1 dropping id 0; every other id lies past the map
    Arrays a = build();
    const uint32_t pods[8][3] = {
        {0, E(63, 3), E(4095, 0)}, {E(5, 0), E(62, 3), E(4094, 0)},
        {E(63, 2), E(62, 1), 0},   {E(64, 0), 0, 0},
        {E(4095, 3), 0, 0},        {E(0, 0), 0, 0},
        {E(70, 1), 0, E(5, 2)},    {0, 0, 0}};
    rc |= expect("n = 1", a, {-1}, pods, m0, 0, 1, 0);
  }
  {  // n = 64: ids 64, 70, 4094, 4095 are >= n and stay; 63 -> 0, 0 -> 63
    Arrays a = build();
    std::vector<int32_t> r(ident.begin(), ident.begin() + 64);
    r[63] = 0; r[0] = 63; r[62] = -1;
    const uint32_t pods[8][3] = {
        {E(63, 0), E(0, 3), E(4095, 0)}, {E(5, 0), 0, E(4094, 0)},
        {E(0, 2), 0, 0},                 {E(64, 0), 0, 0},
        {E(4095, 3), 0, 0},              {E(0, 0), 0, 0},
        {E(70, 1), 0, E(5, 2)},          {0, 0, 0}};
    rc |= expect("id >= n", a, r, pods, m0, 3, 2, 0);
  }
  return rc;
}

int main() {
  if (hand_cases()) return 1;
  std::mt19937_64 rng(9090);
  const uint32_t edge_ids[] = {0, 1, 62, 63, 64, 65, 66, 127, 128,
                               4094, 4095, 4096, 0x00FFFFFEu};
  for (uint64_t cap : {(uint64_t)1, (uint64_t)2, (uint64_t)64}) {
    for (int P = 1; P <= 17; ++P) {
      for (int n : {1, 66, 4096}) {
        for (int kind = 0; kind < 4; ++kind) {
          // 0 identity, 1 reversal (swaps), 2 random drops, 3 compaction
          std::vector<int32_t> remap(n);
          for (int i = 0; i < n; ++i) remap[i] = i;
          if (kind == 1) {
            for (int i = 0; i < n; ++i) remap[i] = n - 1 - i;
          } else if (kind == 2) {
            for (int i = 0; i < n; ++i)
              if (rng() % 3 == 0) remap[i] = -1;
          } else if (kind == 3) {
            int next = 0;
            for (int i = 0; i < n; ++i)
              remap[i] = (rng() % 3 == 0) ? -1 : next++;
          }
          Arrays a(cap, P);
          for (uint64_t i = 0; i < cap; ++i) {
            a.keys[i] = a.e_keys[i] = rng() | 1;
            a.e_vals[i] = rng();
            const int mk = (int)(rng() % 5);
            a.meta[i] = mk == 0 ? 0u
                        : mk == 1
                            ? (META_OCC | META_TOMB | (uint32_t)(i & 1))
                            : (META_OCC | (uint32_t)(i & 1));
            // an injective map keeps distinct ids distinct, so rows hold
            // each id once, as in a real table
            std::vector<uint32_t> used;
            for (int k = 0; k < P; ++k) {
              const uint64_t r = rng();
              if (r % 3 == 0) continue;  // empty slot
              const uint32_t pid =
                  (r % 3 == 1) ? edge_ids[(r >> 8) % 13]
                               : (uint32_t)((r >> 8) % ((uint32_t)n + 70u));
              bool dup = false;
              for (uint32_t u : used) dup |= u == pid;
              if (dup) continue;
              used.push_back(pid);
              a.pods[i * P + k] = E(pid, (uint32_t)((r >> 40) % 4));
            }
          }
          const Arrays b = a;  // what it was
          const RemapCounts got =
              remap_pods_host(a.view(), remap.data(), n);

          int64_t moved = 0, cleared = 0, tombs = 0;
          for (uint64_t i = 0; i < cap; ++i) {
            const uint32_t m = b.meta[i];
            int row_cleared = 0, left = 0;
            for (int k = 0; k < P; ++k) {
              const uint32_t e = b.pods[i * P + k];
              const uint32_t now = a.pods[i * P + k];
              const uint32_t pid = (e & 0x00FFFFFFu) - 1;
              if (!(m & META_OCC) || e == 0 || pid >= (uint32_t)n ||
                  remap[pid] == (int32_t)pid) {
                if (now != e) return fail("entry changed", P, n);
                left += (m & META_OCC) && e != 0;
              } else if (remap[pid] < 0) {
                if (now != 0) return fail("entry not dropped", P, n);
                ++row_cleared;
              } else {
                if (now != ((e & 0xFF000000u) | (uint32_t)(remap[pid] + 1)))
                  return fail("entry not moved", P, n);
                ++moved;
                ++left;
              }
            }
            cleared += row_cleared;
            const bool tomb_now = row_cleared && !left && !(m & META_TOMB);
            tombs += tomb_now;
            if (a.meta[i] != (tomb_now ? (m | META_TOMB) : m))
              return fail("meta", P, n);
          }
          if (got.entries_moved != moved || got.entries_cleared != cleared ||
              got.keys_tombstoned != tombs)
            return fail("counts", P, n);
          if (kind == 0 && (moved || cleared || tombs))
            return fail("identity", P, n);
          if (a.keys != b.keys || a.stamp != b.stamp ||
              a.e_keys != b.e_keys || a.e_meta != b.e_meta ||
              a.e_vals != b.e_vals)
            return fail("untouched arrays", P, n);
        }
      }
    }
  }
  printf("remap_asan_check OK\n");
  return 0;
}
