// cpu_ops.cpp - CPU reference implementation of the kvidx table ops.
//
// Operates on the exact same tensor layout as the HIP kernels
// (kvidx_common.h) so CPU<->GPU differential tests are bit-exact, and
// serves as the fast CPU backend (the pure-Python in-memory index is the
// behavioral reference; this is the performance path on CPU-only hosts).
// Thread-safety is provided by the Python-side caller (one writer at a
// time); the GPU path uses atomics instead (hip_ops.hip).

#include <cstring>

#include "kvidx_ops.h"

namespace kvidx {

static int64_t table_find(const Table& v, uint64_t h, uint32_t model) {
  return probe_find(v.keys, v.meta, v.cap_mask, h, model);
}
static int64_t emap_find(const Table& v, uint64_t h, uint32_t model) {
  return probe_find(v.e_keys, v.e_meta, v.cap_mask, h, model);
}

// Probe-or-insert. Window-full policy: reuse first tombstone, else
// overwrite the lowest-stamp live slot (approximate LRU eviction, the
// CPU analog of the reference's LRU-under-pressure, in_memory.go:32-35).
static int64_t table_put(const Table& v, uint64_t h, uint32_t model,
                         int32_t epoch) {
  h = remap_hash(h);
  uint64_t s = probe_start(h, v.cap_mask);
  int64_t first_tomb = -1;
  int64_t victim = -1;
  int32_t victim_stamp = 0;
  for (int t = 0; t < PROBE_MAX; ++t) {
    uint64_t i = (s + t) & v.cap_mask;
    uint64_t k = v.keys[i];
    uint32_t m = v.meta[i];
    if (k == 0) {  // free: claim
      if (first_tomb >= 0) { i = (uint64_t)first_tomb; }
      v.keys[i] = h;
      std::memset(v.pods + i * v.pods_per_key, 0,
                  sizeof(uint32_t) * v.pods_per_key);
      v.meta[i] = META_OCC | (model & META_MODEL_MASK);
      v.stamp[i] = epoch;
      return (int64_t)i;
    }
    if ((m & META_OCC) && !(m & META_TOMB)) {
      if (k == h && (m & META_MODEL_MASK) == model) {
        v.stamp[i] = epoch;
        return (int64_t)i;
      }
      if (victim < 0 || v.stamp[i] < victim_stamp) {
        victim = (int64_t)i;
        victim_stamp = v.stamp[i];
      }
    } else if ((m & META_TOMB) && first_tomb < 0) {
      first_tomb = (int64_t)i;
    }
  }
  int64_t i = first_tomb >= 0 ? first_tomb : victim;
  if (i < 0) i = (int64_t)s;
  v.keys[i] = h;
  std::memset(v.pods + i * v.pods_per_key, 0,
              sizeof(uint32_t) * v.pods_per_key);
  v.meta[i] = META_OCC | (model & META_MODEL_MASK);
  v.stamp[i] = epoch;
  return i;
}

static void pod_set_add(const Table& v, int64_t slot, uint32_t entry,
                        int32_t epoch) {
  uint32_t* p = v.pods + slot * v.pods_per_key;
  for (int j = 0; j < v.pods_per_key; ++j)
    if (p[j] == entry) return;
  for (int j = 0; j < v.pods_per_key; ++j)
    if (p[j] == 0) {
      p[j] = entry;
      return;
    }
  p[(uint32_t)epoch % v.pods_per_key] = entry;  // full: pseudo-LRU overwrite
}

// ---- engine map (same probing, value payload) ------------------------

static int64_t emap_put(const Table& v, uint64_t h, uint32_t model,
                        uint64_t val, int32_t epoch) {
  h = remap_hash(h);
  uint64_t s = probe_start(h, v.cap_mask);
  int64_t first_tomb = -1;
  int64_t victim = -1;
  int32_t victim_stamp = 0;
  for (int t = 0; t < PROBE_MAX; ++t) {
    uint64_t i = (s + t) & v.cap_mask;
    uint64_t k = v.e_keys[i];
    uint32_t m = v.e_meta[i];
    if (k == 0) {
      if (first_tomb >= 0) i = (uint64_t)first_tomb;
      v.e_keys[i] = h;
      v.e_vals[i] = val;
      v.e_meta[i] = META_OCC | (model & META_MODEL_MASK);
      return (int64_t)i;
    }
    if ((m & META_OCC) && !(m & META_TOMB)) {
      if (k == h && (m & META_MODEL_MASK) == model) {
        v.e_vals[i] = val;
        return (int64_t)i;
      }
      if (victim < 0) victim = (int64_t)i;  // first as victim (no stamps)
      (void)victim_stamp;
    } else if ((m & META_TOMB) && first_tomb < 0) {
      first_tomb = (int64_t)i;
    }
  }
  int64_t i = first_tomb >= 0 ? first_tomb : victim;
  if (i < 0) i = (int64_t)s;
  v.e_keys[i] = h;
  v.e_vals[i] = val;
  v.e_meta[i] = META_OCC | (model & META_MODEL_MASK);
  (void)epoch;
  return i;
}

}  // namespace kvidx

// ---- public ops ------------------------------------------------------
// Definitions of what kvidx_ops.h declares.  The names are qualified, so
// a signature that drifts from its declaration does not compile.

std::vector<uint64_t> kvidx::tokens_to_chunk_hashes(
    std::vector<uint64_t> tokens, uint64_t parent, int64_t block_size,
    int64_t algo) {
  TORCH_CHECK(block_size > 0 && block_size <= 256,
              "block_size must be in (0, 256]");
  std::vector<uint32_t> toks(tokens.begin(), tokens.end());
  int64_t n_chunks = (int64_t)toks.size() / block_size;
  std::vector<uint64_t> out;
  out.reserve(n_chunks);
  uint64_t h = parent;
  dispatch_algo(algo, [&](auto A) {
    for (int64_t c = 0; c < n_chunks; ++c) {
      const uint32_t* t = toks.data() + c * block_size;
      if constexpr (decltype(A)::value == ALGO_FNV64A)
        h = chunk_hash(h, t, (int)block_size);
      else
        h = chunk_hash_sha256(h, t, (int)block_size,
                              sha_digest_word(decltype(A)::value));
      out.push_back(h);
    }
  });
  return out;
}

// Twin of tokens_to_chunk_hashes over the code the GPU hot path runs, so
// tests can verify it on every CBOR / SHA padding boundary without a
// GPU: chunk_hash_fast (branchless FNV) for algo 0, and the
// encode-whole-payload-then-compress shape of k_sha_chain_tr
// (chunk_hash_sha256_wave) for the SHA algos.
std::vector<uint64_t> kvidx::tokens_to_chunk_hashes_fast(
    std::vector<uint64_t> tokens, uint64_t parent, int64_t block_size,
    int64_t algo) {
  TORCH_CHECK(block_size > 0, "block_size must be positive");
  std::vector<uint32_t> toks(tokens.begin(), tokens.end());
  int64_t n_chunks = (int64_t)toks.size() / block_size;
  std::vector<uint64_t> out;
  out.reserve(n_chunks);
  uint64_t h = parent;
  std::vector<uint32_t> words(
      16 * sha_blocks_for(sha_max_payload((int)block_size)));
  dispatch_algo(algo, [&](auto A) {
    for (int64_t c = 0; c < n_chunks; ++c) {
      const uint32_t* t = toks.data() + c * block_size;
      if constexpr (decltype(A)::value == ALGO_FNV64A) {
        // the wide-parent path whenever it applies, as a wave of the
        // kernel whose parents are all wide takes it
        h = chunk_hash_fast(h, t, (int)block_size, h > 0xFFFFFFFFull);
      } else {
        ShaHostBuf buf{words.data()};
        h = chunk_hash_sha256_wave(h, t, (int)block_size,
                                   sha_digest_word(decltype(A)::value), buf, true,
                                   ShaHostAny{});
      }
      out.push_back(h);
    }
  });
  return out;
}

// Batched chain hashing: tokens (int64 [total]), offsets (int64 [B+1]),
// parents (int64 [B], u64 bits) -> per-prompt chunk hashes, flat, with
// chunk-count offsets returned alongside.
std::vector<at::Tensor> kvidx::hash_chain_batch(
    at::Tensor tokens, at::Tensor offsets, at::Tensor parents,
    int64_t block_size, int64_t algo) {
  TORCH_CHECK(tokens.dtype() == at::kLong && offsets.dtype() == at::kLong &&
              parents.dtype() == at::kLong);
  TORCH_CHECK(block_size > 0, "block_size must be positive");
  auto tok = tokens.contiguous();
  auto off = offsets.contiguous();
  auto par = parents.contiguous();
  int64_t B = par.numel();
  const int64_t* offp = off.data_ptr<int64_t>();
  const int64_t* tokp = tok.data_ptr<int64_t>();
  const uint64_t* parp = u64p(par);

  auto chunk_off = at::zeros({B + 1}, tokens.options());
  int64_t* cop = chunk_off.data_ptr<int64_t>();
  for (int64_t b = 0; b < B; ++b)
    cop[b + 1] = cop[b] + (offp[b + 1] - offp[b]) / block_size;
  auto out = at::empty({cop[B]}, tokens.options());
  uint64_t* outp = u64p(out);

  dispatch_algo(algo, [&](auto A) {
    at::parallel_for(0, B, 1, [&](int64_t begin, int64_t end) {
      std::vector<uint32_t> buf(block_size);
      for (int64_t b = begin; b < end; ++b) {
        uint64_t h = parp[b];
        int64_t n_chunks = cop[b + 1] - cop[b];
        const int64_t* t0 = tokp + offp[b];
        for (int64_t c = 0; c < n_chunks; ++c) {
          for (int64_t j = 0; j < block_size; ++j)
            buf[j] = (uint32_t)t0[c * block_size + j];
          if constexpr (decltype(A)::value == ALGO_FNV64A)
            h = chunk_hash(h, buf.data(), (int)block_size);
          else
            h = chunk_hash_sha256(h, buf.data(), (int)block_size,
                                  sha_digest_word(decltype(A)::value));
          outp[cop[b] + c] = h;
        }
      }
    });
  });
  return {out, chunk_off};
}

// Tombstone compaction (ROADMAP #9): rehash every live entry of `old`
// into the freshly-zeroed `nw` bundle (optionally a different power-of-
// two capacity). Stamps (approximate-LRU epochs) and pod rows are
// carried over verbatim; tombstones and dead probe windows disappear.
void kvidx::cpu_compact(KVIDX_TABLE_PARAMS, at::Tensor n_keys,
                        at::Tensor n_meta, at::Tensor n_stamp,
                        at::Tensor n_pods, at::Tensor n_e_keys,
                        at::Tensor n_e_meta, at::Tensor n_e_vals) {
  auto ov = make_table_view(KVIDX_TABLE_ARGS, false);
  auto nv = make_table_view(n_keys, n_meta, n_stamp, n_pods, n_e_keys,
                            n_e_meta, n_e_vals, pods_per_key, false);
  int64_t cap = keys.numel();
  for (int64_t i = 0; i < cap; ++i) {
    uint32_t m = ov.meta[i];
    if (!(m & META_OCC) || (m & META_TOMB)) continue;
    int64_t s2 = table_put(nv, (uint64_t)ov.keys[i], m & META_MODEL_MASK,
                           ov.stamp[i]);
    std::memcpy(nv.pods + s2 * nv.pods_per_key,
                ov.pods + i * ov.pods_per_key,
                sizeof(uint32_t) * nv.pods_per_key);
  }
  for (int64_t i = 0; i < cap; ++i) {
    uint32_t m = ov.e_meta[i];
    if (!(m & META_OCC) || (m & META_TOMB)) continue;
    emap_put(nv, (uint64_t)ov.e_keys[i], m & META_MODEL_MASK,
             (uint64_t)ov.e_vals[i], 0);
  }
}

// shard_id/num_shards: the main table stores only keys it owns
// (request_hash % num_shards == shard_id); the engine->request map is
// replicated on every shard so parent-chain stitching never needs a
// cross-rank lookup (see parallel/sharded.py).
void kvidx::cpu_insert(KVIDX_TABLE_PARAMS, at::Tensor engine_hashes,
                       at::Tensor request_hashes, int64_t model_id,
                       at::Tensor pod_entries, int64_t epoch, int64_t shard_id,
                       int64_t num_shards, int64_t emap_write) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, false);
  auto eh = engine_hashes.contiguous();
  auto rh = request_hashes.contiguous();
  auto pe = pod_entries.contiguous();
  const uint64_t* ehp = u64p(eh);
  const uint64_t* rhp = u64p(rh);
  const uint32_t* pep = u32p(pe);
  int64_t n = eh.numel();
  int64_t m = pe.numel();
  TORCH_CHECK(rh.numel() == n, "engine/request key length mismatch");
  for (int64_t i = 0; i < n; ++i) {
    if (emap_write)
      emap_put(v, ehp[i], (uint32_t)model_id, remap_hash(rhp[i]),
               (int32_t)epoch);
    if (!owns_key(rhp[i], (int)shard_id, (int)num_shards)) continue;
    int64_t slot = table_put(v, rhp[i], (uint32_t)model_id, (int32_t)epoch);
    for (int64_t j = 0; j < m; ++j)
      pod_set_add(v, slot, pep[j], (int32_t)epoch);
  }
}

// Walk precomputed (possibly all-reduce-merged) masks -> scores; CPU twin
// of k_score_from_masks for gloo-backed multi-process tests.
at::Tensor kvidx::cpu_score_from_masks(at::Tensor masks, at::Tensor offsets,
                                       at::Tensor weights, int64_t num_pods) {
  auto m = masks.contiguous();
  auto off = offsets.contiguous();
  TORCH_CHECK(m.dim() == 3, "masks must be [Ktot, T, W]");
  const int64_t T = m.size(1);  // tier planes (sized by caller)
  const uint64_t* mp = u64p(m);
  const int32_t* op = off.data_ptr<int32_t>();
  const float* wts = weights.data_ptr<float>();
  int64_t B = off.numel() - 1;
  int64_t W = pod_words(num_pods);
  TORCH_CHECK(W <= 64, "num_pods > 4096 not supported");
  auto scores = at::zeros({B, num_pods}, at::kFloat);
  float* sp = scores.data_ptr<float>();
  at::parallel_for(0, B, 1, [&](int64_t begin, int64_t end) {
    for (int64_t b = begin; b < end; ++b) {
      uint64_t active[64];
      float* out = sp + b * num_pods;
      int64_t K = op[b + 1] - op[b];
      for (int64_t k = 0; k < K; ++k) {
        const uint64_t* mk = mp + (size_t)(op[b] + k) * T * W;
        bool any = false;
        for (int64_t w = 0; w < W; ++w) {
          uint64_t cur = 0;
          for (int t = 0; t < T; ++t) cur |= mk[t * W + w];
          uint64_t act = (k == 0) ? cur : (active[w] & cur);
          active[w] = act;
          if (act) any = true;
          uint64_t bits = act;
          while (bits) {
            int bit = __builtin_ctzll(bits);
            bits &= bits - 1;
            float wmax = 0.f;
            for (int t = 0; t < T; ++t)
              if ((mk[t * W + w] >> bit) & 1) wmax = std::max(wmax, wts[t]);
            out[w * 64 + bit] += wmax;
          }
        }
        if (!any) break;
      }
    }
  });
  return scores;
}

void kvidx::cpu_evict(KVIDX_TABLE_PARAMS, at::Tensor engine_hashes,
                      int64_t model_id, at::Tensor pod_entries) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, false);
  auto eh = engine_hashes.contiguous();
  auto pe = pod_entries.contiguous();
  const uint64_t* ehp = u64p(eh);
  const uint32_t* pep = u32p(pe);
  // Engine->request mappings are deliberately RETAINED on eviction
  // (unlike in_memory.go:252-255): with the sharded deployment the emap
  // is replicated while the main table is ownership-filtered, so only
  // the owning shard can observe "pod set now empty" - dropping the
  // mapping locally would diverge the replicas and break parent-chain
  // stitching after removals.  A retained mapping also keeps child
  // chains content-consistent (the reference restarts them from the
  // root); stale entries are reclaimed by the emap's own slot-steal.
  for (int64_t i = 0; i < eh.numel(); ++i) {
    int64_t ei = emap_find(v, ehp[i], (uint32_t)model_id);
    if (ei < 0) continue;
    uint64_t req = v.e_vals[ei];
    int64_t slot = table_find(v, req, (uint32_t)model_id);
    if (slot < 0) continue;
    uint32_t* p = v.pods + slot * v.pods_per_key;
    for (int64_t j = 0; j < pe.numel(); ++j)
      for (int k = 0; k < v.pods_per_key; ++k)
        if (p[k] == pep[j]) p[k] = 0;
    bool empty = true;
    for (int k = 0; k < v.pods_per_key; ++k)
      if (p[k] != 0) { empty = false; break; }
    if (empty) v.meta[slot] |= META_TOMB;
  }
}

// Purge by pod: the sweep itself is purge_pods_host (kvidx_common.h,
// torch-free so that a stand-alone sanitizer build can call it).
std::vector<int64_t> kvidx::cpu_purge_pods(KVIDX_TABLE_PARAMS,
                                           at::Tensor purge_words,
                                           int64_t model_id) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, false);
  const int W = purge_words_checked(purge_words, model_id);
  TORCH_CHECK(pods.numel() == keys.numel() * pods_per_key,
              "pods must hold capacity * pods_per_key entries");
  const PurgeCounts c = purge_pods_host(v, u64p(purge_words), W, model_id);
  return {c.entries_cleared, c.keys_tombstoned};
}

// Remap pod ids: the sweep is remap_pods_host (kvidx_common.h, torch-free
// like the purge's).
std::vector<int64_t> kvidx::cpu_remap_pods(KVIDX_TABLE_PARAMS,
                                           at::Tensor remap) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, false);
  TORCH_CHECK(!remap.is_cuda(), "remap must be a CPU tensor");
  const int n = remap_checked(remap);
  TORCH_CHECK(pods.numel() == keys.numel() * pods_per_key,
              "pods must hold capacity * pods_per_key entries");
  const RemapCounts c = remap_pods_host(v, i32p(remap), n);
  return {c.entries_moved, c.entries_cleared, c.keys_tombstoned};
}

// found: 0 absent, 1 present-with-visible-pods, 2 present-but-empty
// (chain-cut marker, in_memory.go:118-121).
std::vector<at::Tensor> kvidx::cpu_lookup(KVIDX_TABLE_PARAMS,
                                          at::Tensor request_hashes,
                                          int64_t model_id,
                                          at::Tensor filter_words,
                                          int64_t num_pods, int64_t epoch,
                                          int64_t shard_id, int64_t num_shards,
                                          int64_t n_tiers) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, false);
  auto rh = request_hashes.contiguous();
  const uint64_t* rhp = u64p(rh);
  int64_t K = rh.numel();
  int64_t W = pod_words(num_pods);
  bool has_filter = filter_words.numel() > 0;
  const uint64_t* fw = has_filter ? u64p(filter_words) : nullptr;

  n_tiers = clamp_tiers(n_tiers);
  auto found = at::zeros({K}, at::kByte);
  // masks sized by the REGISTERED tier count (usually 1-2): halves-to-
  // quarters the fallback path's mask traffic and the sharded
  // all_reduce bytes vs a fixed MAX_TIERS=4 plane count.
  auto masks = at::zeros({K, n_tiers, W}, at::kLong);
  uint8_t* fp = found.data_ptr<uint8_t>();
  uint64_t* mp = u64p(masks);

  for (int64_t k = 0; k < K; ++k) {
    if (!owns_key(rhp[k], (int)shard_id, (int)num_shards))
      continue;  // unowned key: another shard's mask contribution
    int64_t slot = table_find(v, rhp[k], (uint32_t)model_id);
    if (slot < 0) continue;
    v.stamp[slot] = (int32_t)epoch;  // LRU touch on read
    const uint32_t* p = v.pods + slot * v.pods_per_key;
    bool any_raw = false, any_visible = false;
    for (int j = 0; j < v.pods_per_key; ++j) {
      uint32_t e = p[j];
      if (e == 0) continue;
      any_raw = true;
      uint32_t pid = pod_entry_id(e);
      uint32_t tier = pod_entry_tier(e);
      if (pid >= (uint32_t)num_pods || tier >= (uint32_t)n_tiers) continue;
      if (has_filter && !((fw[pid / 64] >> (pid % 64)) & 1)) continue;
      mp[(k * n_tiers + tier) * W + pid / 64] |= 1ull << (pid % 64);
      any_visible = true;
    }
    (void)any_visible;
    fp[k] = any_raw ? 1 : 2;  // 2 = present-but-empty (chain cut)
  }
  return {found, masks};
}

// Fused probe + longest-prefix score (the read-path hot loop, scoring
// parity with kvblock_scorer.go:108-151).
at::Tensor kvidx::cpu_fused_score(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                  at::Tensor counts, int64_t model_id,
                                  at::Tensor filter_words, at::Tensor weights,
                                  int64_t num_pods, int64_t epoch) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, false);
  auto h = hashes.contiguous();
  auto cnt = counts.contiguous();
  const uint64_t* hp = u64p(h);
  const int32_t* cp = cnt.data_ptr<int32_t>();
  int64_t B = cnt.numel();
  int64_t W = pod_words(num_pods);
  bool has_filter = filter_words.numel() > 0;
  const uint64_t* fw = has_filter ? u64p(filter_words) : nullptr;
  const float* wts = weights.data_ptr<float>();

  TORCH_CHECK(W <= 64, "num_pods > 4096 not supported");
  auto scores = at::zeros({B, num_pods}, at::kFloat);
  float* sp = scores.data_ptr<float>();

  std::vector<int64_t> bases(B + 1, 0);
  for (int64_t b = 0; b < B; ++b) bases[b + 1] = bases[b] + cp[b];

  at::parallel_for(0, B, 1, [&](int64_t begin, int64_t end) {
    for (int64_t b = begin; b < end; ++b) {
      uint64_t tier_masks[MAX_TIERS * 64];
      uint64_t active[64];
      uint64_t cur[64];
      int64_t base = bases[b];
      int64_t K = cp[b];
      float* out = sp + b * num_pods;
      bool first = true;
      for (int64_t k = 0; k < K; ++k) {
        for (int64_t x = 0; x < MAX_TIERS * W; ++x) tier_masks[x] = 0;
        for (int64_t w = 0; w < W; ++w) cur[w] = 0;
        int64_t slot = table_find(v, hp[base + k], (uint32_t)model_id);
        if (slot >= 0) {
          v.stamp[slot] = (int32_t)epoch;
          const uint32_t* p = v.pods + slot * v.pods_per_key;
          for (int j = 0; j < v.pods_per_key; ++j) {
            uint32_t e = p[j];
            if (e == 0) continue;
            uint32_t pid = pod_entry_id(e);
            uint32_t tier = pod_entry_tier(e);
            if (pid >= (uint32_t)num_pods || tier >= MAX_TIERS) continue;
            if (has_filter && !((fw[pid / 64] >> (pid % 64)) & 1)) continue;
            tier_masks[tier * W + pid / 64] |= 1ull << (pid % 64);
            cur[pid / 64] |= 1ull << (pid % 64);
          }
        }
        if (first) {
          for (int64_t w = 0; w < W; ++w) active[w] = cur[w];
          first = false;
        } else {
          for (int64_t w = 0; w < W; ++w) active[w] &= cur[w];
        }
        bool any = false;
        for (int64_t w = 0; w < W; ++w) {
          uint64_t a = active[w];
          if (!a) continue;
          any = true;
          uint64_t bits = a;
          while (bits) {
            int bit = __builtin_ctzll(bits);
            bits &= bits - 1;
            int64_t pid = w * 64 + bit;
            float wmax = 0.f;
            for (int t = 0; t < MAX_TIERS; ++t)
              if ((tier_masks[t * W + w] >> bit) & 1)
                wmax = std::max(wmax, wts[t]);
            out[pid] += wmax;
          }
        }
        if (!any) break;
      }
    }
  });
  return scores;
}

std::vector<at::Tensor> kvidx::cpu_get_request_keys(
    KVIDX_TABLE_PARAMS, at::Tensor engine_hashes, int64_t model_id) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, false);
  auto eh = engine_hashes.contiguous();
  const uint64_t* ehp = u64p(eh);
  int64_t n = eh.numel();
  auto found = at::zeros({n}, at::kByte);
  auto out = at::zeros({n}, at::kLong);
  uint8_t* fp = found.data_ptr<uint8_t>();
  uint64_t* op = u64p(out);
  for (int64_t i = 0; i < n; ++i) {
    int64_t ei = emap_find(v, ehp[i], (uint32_t)model_id);
    if (ei >= 0) {
      fp[i] = 1;
      op[i] = v.e_vals[ei];
    }
  }
  return {found, out};
}
