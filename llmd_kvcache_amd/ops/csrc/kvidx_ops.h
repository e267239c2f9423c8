// kvidx_ops.h - the one declaration of every native op, plus the host
// helpers the CPU and HIP translation units share.  bindings.cpp,
// wirefront.cpp, cpu_ops.cpp and hip_ops.hip all include it, so a
// definition that drifts from its declaration fails to compile.

#pragma once

#include <torch/extension.h>

#include <type_traits>
#include <vector>

#include "kvidx_common.h"

// Every table op starts with the table bundle (kvidx_common.h layout).
#define KVIDX_TABLE_PARAMS                                                  \
  at::Tensor keys, at::Tensor meta, at::Tensor stamp, at::Tensor pods,      \
      at::Tensor e_keys, at::Tensor e_meta, at::Tensor e_vals,              \
      int64_t pods_per_key
#define KVIDX_TABLE_ARGS \
  keys, meta, stamp, pods, e_keys, e_meta, e_vals, pods_per_key

namespace kvidx {

// ---- chain ops (cpu_ops.cpp) -----------------------------------------
std::vector<uint64_t> tokens_to_chunk_hashes(std::vector<uint64_t> tokens,
                                             uint64_t parent,
                                             int64_t block_size, int64_t algo);
std::vector<uint64_t> tokens_to_chunk_hashes_fast(std::vector<uint64_t> tokens,
                                                  uint64_t parent,
                                                  int64_t block_size,
                                                  int64_t algo);
std::vector<at::Tensor> hash_chain_batch(at::Tensor tokens, at::Tensor offsets,
                                         at::Tensor parents,
                                         int64_t block_size, int64_t algo);

// ---- table ops, CPU (cpu_ops.cpp) ------------------------------------
void cpu_insert(KVIDX_TABLE_PARAMS, at::Tensor engine_hashes,
                at::Tensor request_hashes, int64_t model_id,
                at::Tensor pod_entries, int64_t epoch, int64_t shard_id,
                int64_t num_shards, int64_t emap_write);
void cpu_compact(KVIDX_TABLE_PARAMS, at::Tensor n_keys, at::Tensor n_meta,
                 at::Tensor n_stamp, at::Tensor n_pods, at::Tensor n_e_keys,
                 at::Tensor n_e_meta, at::Tensor n_e_vals);
void cpu_evict(KVIDX_TABLE_PARAMS, at::Tensor engine_hashes, int64_t model_id,
               at::Tensor pod_entries);
// Purge by pod: purge_words int64 [W], 1 <= W <= 64, bit pid % 64 of word
// pid / 64 selects pod id pid; model_id -1 = every model.
// -> {entries_cleared, keys_tombstoned}.
std::vector<int64_t> cpu_purge_pods(KVIDX_TABLE_PARAMS, at::Tensor purge_words,
                                    int64_t model_id);
// Remap pod ids: remap int32 [n] contiguous, 1 <= n <= MAX_PODS, remap[old]
// = new id in 0..MAX_PODS-1 or -1 = drop, the non-negative values pairwise
// distinct.  Entries whose id is >= n stay.  Every occupied slot takes part,
// whatever its model.  -> {entries_moved, entries_cleared, keys_tombstoned}.
//
// Concurrency contract - NOT the purge's: the caller guarantees that no
// other writer touches the table for the duration (the registry's id gate,
// held exclusively, provides this).  A remap is not idempotent, and an
// insert that carries a pre-remap id and races with it cannot be repaired
// by a compare-and-swap the way a raced purge can, so the sweeps use plain
// stores.
std::vector<int64_t> cpu_remap_pods(KVIDX_TABLE_PARAMS, at::Tensor remap);
std::vector<at::Tensor> cpu_lookup(KVIDX_TABLE_PARAMS,
                                   at::Tensor request_hashes, int64_t model_id,
                                   at::Tensor filter_words, int64_t num_pods,
                                   int64_t epoch, int64_t shard_id,
                                   int64_t num_shards, int64_t n_tiers);
at::Tensor cpu_fused_score(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                           at::Tensor counts, int64_t model_id,
                           at::Tensor filter_words, at::Tensor weights,
                           int64_t num_pods, int64_t epoch);
at::Tensor cpu_score_from_masks(at::Tensor masks, at::Tensor offsets,
                                at::Tensor weights, int64_t num_pods);
std::vector<at::Tensor> cpu_get_request_keys(KVIDX_TABLE_PARAMS,
                                             at::Tensor engine_hashes,
                                             int64_t model_id);

#ifdef KVIDX_WITH_HIP
// ---- table and chain ops, gfx950 (hip_ops.hip) -----------------------
void gpu_insert(KVIDX_TABLE_PARAMS, at::Tensor engine_hashes,
                at::Tensor request_hashes, int64_t model_id,
                at::Tensor pod_entries, int64_t epoch, int64_t shard_id,
                int64_t num_shards, int64_t emap_write);
void gpu_compact(KVIDX_TABLE_PARAMS, at::Tensor n_keys, at::Tensor n_meta,
                 at::Tensor n_stamp, at::Tensor n_pods, at::Tensor n_e_keys,
                 at::Tensor n_e_meta, at::Tensor n_e_vals);
void gpu_evict(KVIDX_TABLE_PARAMS, at::Tensor engine_hashes, int64_t model_id,
               at::Tensor pod_entries);
std::vector<int64_t> gpu_purge_pods(KVIDX_TABLE_PARAMS, at::Tensor purge_words,
                                    int64_t model_id);
// remap on the table's device; the sweep has completed on return
std::vector<int64_t> gpu_remap_pods(KVIDX_TABLE_PARAMS, at::Tensor remap);
std::vector<at::Tensor> gpu_get_request_keys(KVIDX_TABLE_PARAMS,
                                             at::Tensor engine_hashes,
                                             int64_t model_id);
std::vector<at::Tensor> gpu_lookup(KVIDX_TABLE_PARAMS,
                                   at::Tensor request_hashes, int64_t model_id,
                                   at::Tensor filter_words, int64_t num_pods,
                                   int64_t epoch, int64_t shard_id,
                                   int64_t num_shards, int64_t n_tiers);
at::Tensor gpu_fused_score(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                           at::Tensor offsets, int64_t model_id,
                           at::Tensor filter_words, at::Tensor weights,
                           int64_t num_pods, int64_t epoch, int64_t max_k,
                           int64_t n_tiers);
at::Tensor gpu_fused_score_rows(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                at::Tensor n_keys, int64_t model_id,
                                at::Tensor filter_words, at::Tensor weights,
                                int64_t num_pods, int64_t epoch, int64_t max_k,
                                int64_t n_tiers);
at::Tensor gpu_score_from_masks(at::Tensor masks, at::Tensor offsets,
                                at::Tensor weights, int64_t num_pods);
// The one place that decides between the fused kernel and lookup + mask
// walk: gpu_fused_score where its LDS holds the batch, else gpu_lookup
// (unsharded) + gpu_score_from_masks.  hashes int64 flat, offsets int32
// [B+1], both on the device.
at::Tensor gpu_score_hashes(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                            at::Tensor offsets, int64_t model_id,
                            at::Tensor filter_words, at::Tensor weights,
                            int64_t num_pods, int64_t epoch, int64_t max_k,
                            int64_t n_tiers);
std::vector<at::Tensor> gpu_hash_chain(at::Tensor tokens, at::Tensor tok_off,
                                       at::Tensor parents, int64_t block_size,
                                       int64_t algo);
// ilp: a retired tuning knob kept in place for positional callers; 0 or 1.
at::Tensor gpu_hash_chain_tr(at::Tensor tokens_t, at::Tensor parents,
                             at::Tensor n_chunks, int64_t block_size,
                             int64_t max_chunks, int64_t ilp,
                             int64_t row_major, int64_t algo);
std::vector<at::Tensor> gpu_stage_ragged_tokens(at::Tensor tokens,
                                                at::Tensor offsets,
                                                int64_t block_size);
at::Tensor gpu_score_flat_tokens(KVIDX_TABLE_PARAMS, at::Tensor tokens_flat,
                                 at::Tensor offsets, int64_t model_id,
                                 at::Tensor filter_words, at::Tensor weights,
                                 int64_t num_pods, int64_t epoch,
                                 int64_t init_hash_bits, int64_t block_size,
                                 int64_t n_tiers, int64_t algo);
void gpu_apply_events(KVIDX_TABLE_PARAMS, at::Tensor tokens,
                      at::Tensor tok_off, at::Tensor ehashes,
                      at::Tensor eh_off, at::Tensor parents,
                      at::Tensor has_parent, at::Tensor ev_type,
                      at::Tensor pod_entry, at::Tensor grp_off,
                      at::Tensor model_of, int64_t init_hash_bits,
                      int64_t block_size, int64_t epoch, int64_t shard_id,
                      int64_t num_shards, int64_t algo);
void gpu_apply_events_split(KVIDX_TABLE_PARAMS, at::Tensor tokens,
                            at::Tensor tok_off, at::Tensor ehashes,
                            at::Tensor eh_off, at::Tensor parents,
                            at::Tensor has_parent, at::Tensor ev_type,
                            at::Tensor pod_entry, at::Tensor grp_off,
                            at::Tensor ev_of, at::Tensor model_of,
                            int64_t init_hash_bits, int64_t block_size,
                            int64_t epoch, int64_t shard_id,
                            int64_t num_shards, int64_t algo);
void gpu_apply_events_split_tr(KVIDX_TABLE_PARAMS, at::Tensor tokens_flat,
                               at::Tensor tok_off, at::Tensor ehashes,
                               at::Tensor eh_off, at::Tensor parents,
                               at::Tensor has_parent, at::Tensor ev_type,
                               at::Tensor pod_entry, at::Tensor ev_of,
                               at::Tensor model_of, int64_t init_hash_bits,
                               int64_t block_size, int64_t epoch,
                               int64_t shard_id, int64_t num_shards,
                               int64_t max_tokens, int64_t algo);
#endif

// ---- shared host helpers ---------------------------------------------

// Typed views of tensor storage: int64 / int32 tensors carry u64 / u32 bit
// patterns (torch has no unsigned 64-bit dtype to speak of).
inline uint64_t* u64p(const at::Tensor& t) {
  return reinterpret_cast<uint64_t*>(t.data_ptr<int64_t>());
}
inline uint32_t* u32p(const at::Tensor& t) {
  return reinterpret_cast<uint32_t*>(t.data_ptr<int32_t>());
}
inline int32_t* i32p(const at::Tensor& t) { return t.data_ptr<int32_t>(); }
inline uint8_t* u8p(const at::Tensor& t) { return t.data_ptr<uint8_t>(); }

// Tier planes are sized by the registered tier count, 1..MAX_TIERS.
inline int64_t clamp_tiers(int64_t n_tiers) {
  return std::min<int64_t>(std::max<int64_t>(n_tiers, 1), MAX_TIERS);
}
// 64-pod mask words for a fleet.
inline int64_t pod_words(int64_t num_pods) { return (num_pods + 63) / 64; }

inline Table make_table_view(KVIDX_TABLE_PARAMS, bool on_gpu) {
  TORCH_CHECK(!on_gpu || keys.is_cuda(), "table must live on the GPU");
  TORCH_CHECK(keys.is_contiguous() && meta.is_contiguous() &&
                  stamp.is_contiguous() && pods.is_contiguous() &&
                  e_keys.is_contiguous() && e_meta.is_contiguous() &&
                  e_vals.is_contiguous(),
              "table tensors must be contiguous");
  int64_t cap = keys.numel();
  TORCH_CHECK((cap & (cap - 1)) == 0, "capacity must be a power of two");
  return Table{u64p(keys),   u32p(meta),   i32p(stamp),
               u32p(pods),   u64p(e_keys), u32p(e_meta),
               u64p(e_vals), (uint64_t)cap - 1, (int)pods_per_key};
}

// Word count of a purge bitmap, after the checks both purge ops share.
inline int purge_words_checked(const at::Tensor& purge_words,
                               int64_t model_id) {
  TORCH_CHECK(purge_words.dtype() == at::kLong && purge_words.dim() == 1 &&
                  purge_words.is_contiguous(),
              "purge_words must be a contiguous int64 [W] tensor");
  const int64_t W = purge_words.numel();
  TORCH_CHECK(W >= 1 && W <= 64, "purge_words must hold 1..64 words");
  TORCH_CHECK(model_id >= -1 && model_id <= (int64_t)META_MODEL_MASK,
              "model_id out of range (-1 = every model)");
  return (int)W;
}

// Length of a pod-id remap, after the checks both remap ops share: shape,
// range of every value, and injectivity of the non-negative ones (so no
// row can end up holding one id twice).  The values are read on the host.
inline int remap_checked(const at::Tensor& remap) {
  TORCH_CHECK(remap.dtype() == at::kInt && remap.dim() == 1 &&
                  remap.is_contiguous(),
              "remap must be a contiguous int32 [n] tensor");
  const int64_t n = remap.numel();
  TORCH_CHECK(n >= 1 && n <= MAX_PODS, "remap must hold 1..", MAX_PODS,
              " ids");
  const at::Tensor host = remap.cpu();
  const int32_t* r = host.data_ptr<int32_t>();
  std::vector<uint8_t> taken(MAX_PODS, 0);
  for (int64_t i = 0; i < n; ++i) {
    TORCH_CHECK(r[i] >= -1 && r[i] < MAX_PODS, "remap[", i, "] = ", r[i],
                " is outside -1..", MAX_PODS - 1);
    if (r[i] < 0) continue;
    TORCH_CHECK(!taken[r[i]], "remap sends two ids to ", r[i]);
    taken[r[i]] = 1;
  }
  return (int)n;
}

// Runs f(std::integral_constant<int, ALGO>) for a native chain algo id
// (0 fnv-64a, 1 sha256-cbor-64, 2 sha256-cbor-64-low) and returns what it
// returns: the id picks an instantiation once per call on the host, never
// a branch inside a kernel or a chunk loop.
template <typename F>
auto dispatch_algo(int64_t algo, F&& f) {
  TORCH_CHECK(algo_valid(algo), "unknown chain hash algo id ", algo);
  switch (algo) {
    case ALGO_SHA256_HI:
      return f(std::integral_constant<int, ALGO_SHA256_HI>{});
    case ALGO_SHA256_LOW:
      return f(std::integral_constant<int, ALGO_SHA256_LOW>{});
    default:
      return f(std::integral_constant<int, ALGO_FNV64A>{});
  }
}

}  // namespace kvidx
