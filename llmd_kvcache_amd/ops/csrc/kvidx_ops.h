// kvidx_ops.h - the one declaration of every native op, plus the host
// helpers the CPU and HIP translation units share.  bindings.cpp,
// wirefront.cpp, cpu_ops.cpp and hip_ops.hip all include it, so a
// definition that drifts from its declaration fails to compile.

#pragma once

#include <torch/extension.h>

#include <algorithm>
#include <type_traits>
#include <unordered_map>
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
// Twin of the stream chain kernels (hip_ops.hip k_*_chain_stream), which
// take the block size at run time: 1 <= block_size <= 65535, a tokens-array
// header of at most three bytes.  In every build.
inline bool stream_chain_block_size_ok(int64_t block_size) {
  return block_size >= 1 && block_size <= 0xFFFF;
}
std::vector<uint64_t> tokens_to_chunk_hashes_stream(
    std::vector<uint64_t> tokens, uint64_t parent, int64_t block_size,
    int64_t algo);
std::vector<at::Tensor> hash_chain_batch(at::Tensor tokens, at::Tensor offsets,
                                         at::Tensor parents,
                                         int64_t block_size, int64_t algo);
// The host plan of the ragged device chain (plan_ragged_waves below) as
// CPU tensors: {perm int32 [64 G], wave_k int32 [G], img_off int64 [G+1],
// tile_start int32 [G+1], h_off int32 [B+1]}.  In every build.
std::vector<at::Tensor> plan_ragged_waves_op(at::Tensor tokens,
                                             at::Tensor offsets,
                                             int64_t block_size);
// The host plan of the wave-tiled ingest chain (plan_event_waves below) as
// CPU tensors: plan_ragged_waves_op's five, lanes = events, and n_chunks
// int32 [E] as the sixth.  In every build.
std::vector<at::Tensor> plan_event_waves_op(at::Tensor tok_off,
                                            at::Tensor eh_off,
                                            at::Tensor ev_type,
                                            int64_t block_size);
// The host plans of the linked wave ingest (plan_event_links and
// plan_linked_event_waves below) as CPU tensors.  plan_event_links_op:
// {link int32 [E], level int32 [E], n_levels int64 [1]}.
// plan_linked_event_waves_op: plan_event_waves_op's six, then level_wave
// int32 [n_levels + 1] and the plan's copy of link.  In every build.
std::vector<at::Tensor> plan_event_links_op(at::Tensor ehashes,
                                            at::Tensor eh_off,
                                            at::Tensor tok_off,
                                            at::Tensor ev_type,
                                            at::Tensor parents,
                                            at::Tensor has_parent,
                                            at::Tensor grp_off,
                                            int64_t block_size);
std::vector<at::Tensor> plan_linked_event_waves_op(
    at::Tensor tok_off, at::Tensor eh_off, at::Tensor ev_type, at::Tensor link,
    at::Tensor level, int64_t block_size);

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
// Pod census (definitions: kvidx_common.h): read-only; model_id -1 = every
// model, 1 <= num_pods <= MAX_PODS, 1 <= n_tiers <= MAX_TIERS.
// -> {counts int64 [num_pods, n_tiers], summary int64 [6] in CensusSummary
// order}, both on the host.  Advisory under concurrent writers: every word
// is read once, a row's meta and entries possibly at different instants.
std::vector<at::Tensor> cpu_pod_census(KVIDX_TABLE_PARAMS, int64_t model_id,
                                       int64_t num_pods, int64_t n_tiers);
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
// Score top-n (the ordering contract: kvidx_common.h rank_key): scores
// float32 [B, P] on the host, 1 <= P <= MAX_PODS, finite and >= 0.
// -> {ids int32 [B, top_n], scores float32 [B, top_n]}.  What the CPU table
// serves top-n with (cpu_fused_score, then this), and the host statement
// of the contract the GPU ops are tested against.
std::vector<at::Tensor> cpu_score_topk(at::Tensor scores, int64_t top_n);
// Top-n straight from (merged) masks: cpu_score_from_masks, then
// cpu_score_topk.  masks int64 [Ktot, n_tiers, pod_words(num_pods)],
// offsets int32 [B+1], weights float32 [n_tiers]; a prompt without keys
// gives a row of (-1, 0.0f), and pod bits at or past num_pods never score.
// The host statement of what gpu_topk_from_masks returns, bit for bit.
std::vector<at::Tensor> cpu_topk_from_masks(at::Tensor masks,
                                            at::Tensor offsets,
                                            at::Tensor weights,
                                            int64_t num_pods, int64_t top_n);

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
// one sweep and one small reduce on the current stream, one readback
std::vector<at::Tensor> gpu_pod_census(KVIDX_TABLE_PARAMS, int64_t model_id,
                                       int64_t num_pods, int64_t n_tiers);
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
// The merged-mask walk with the pick inside (k_topk_from_masks): what
// cpu_topk_from_masks takes, on one device, 1 <= num_pods <= MAX_PODS,
// 1 <= top_n <= MAX_TOPK, 1 <= n_tiers <= MAX_TIERS.  One launch on the
// current stream; the [B, num_pods] matrix never exists.
std::vector<at::Tensor> gpu_topk_from_masks(at::Tensor masks,
                                            at::Tensor offsets,
                                            at::Tensor weights,
                                            int64_t num_pods, int64_t top_n);
// The one place that decides between the resident and the tiled fused
// kernel: gpu_fused_score where its LDS holds the batch, else
// gpu_tiled_score.  hashes int64 flat, offsets int32 [B+1], both on the
// device.
at::Tensor gpu_score_hashes(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                            at::Tensor offsets, int64_t model_id,
                            at::Tensor filter_words, at::Tensor weights,
                            int64_t num_pods, int64_t epoch, int64_t max_k,
                            int64_t n_tiers);
// Score top-n on the device: every op returns {ids int32 [B, top_n],
// scores float32 [B, top_n]} in the kvidx_common.h rank_key order, written
// by the kernels in full (no fill).  gpu_fused_topk[_rows] take what
// gpu_fused_score[_rows] take and pick inside the walk kernel, so the
// [B, num_pods] matrix never exists; they refuse what fused_score_fits
// refuses.  gpu_topk_rows takes any float32 [B, P] device matrix, 1 <= P
// <= MAX_PODS, values finite and >= 0.  gpu_topk_hashes is the chooser
// (gpu_score_hashes' decision): the resident fused kernel where it fits,
// else gpu_tiled_topk.
std::vector<at::Tensor> gpu_fused_topk(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                       at::Tensor offsets, int64_t model_id,
                                       at::Tensor filter_words,
                                       at::Tensor weights, int64_t num_pods,
                                       int64_t epoch, int64_t max_k,
                                       int64_t n_tiers, int64_t top_n);
std::vector<at::Tensor> gpu_fused_topk_rows(
    KVIDX_TABLE_PARAMS, at::Tensor hashes, at::Tensor n_keys, int64_t model_id,
    at::Tensor filter_words, at::Tensor weights, int64_t num_pods,
    int64_t epoch, int64_t max_k, int64_t n_tiers, int64_t top_n);
std::vector<at::Tensor> gpu_topk_rows(at::Tensor scores, int64_t top_n);
std::vector<at::Tensor> gpu_topk_hashes(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                        at::Tensor offsets, int64_t model_id,
                                        at::Tensor filter_words,
                                        at::Tensor weights, int64_t num_pods,
                                        int64_t epoch, int64_t max_k,
                                        int64_t n_tiers, int64_t top_n);
// The tiled fused kernels: what the four gpu_fused_* ops take and return,
// bit for bit, for any max_k >= 0 and 1 <= num_pods <= MAX_PODS in one
// launch and without a global mask tensor.  The keys pass through LDS
// tiled_score_tile_keys(n_tiers, W) at a time (W = pod_words(num_pods));
// every probed key that is stored gets the call's epoch, as on every other
// route.
int64_t tiled_score_tile_keys(int64_t n_tiers, int64_t W);
at::Tensor gpu_tiled_score(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                           at::Tensor offsets, int64_t model_id,
                           at::Tensor filter_words, at::Tensor weights,
                           int64_t num_pods, int64_t epoch, int64_t max_k,
                           int64_t n_tiers);
at::Tensor gpu_tiled_score_rows(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                at::Tensor n_keys, int64_t model_id,
                                at::Tensor filter_words, at::Tensor weights,
                                int64_t num_pods, int64_t epoch, int64_t max_k,
                                int64_t n_tiers);
std::vector<at::Tensor> gpu_tiled_topk(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                       at::Tensor offsets, int64_t model_id,
                                       at::Tensor filter_words,
                                       at::Tensor weights, int64_t num_pods,
                                       int64_t epoch, int64_t max_k,
                                       int64_t n_tiers, int64_t top_n);
std::vector<at::Tensor> gpu_tiled_topk_rows(
    KVIDX_TABLE_PARAMS, at::Tensor hashes, at::Tensor n_keys, int64_t model_id,
    at::Tensor filter_words, at::Tensor weights, int64_t num_pods,
    int64_t epoch, int64_t max_k, int64_t n_tiers, int64_t top_n);
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
// gpu_score_flat_tokens with the pick on the device as well: stage, chain
// (row-major) and the fused top-n over the rows on one stream, no host
// wait in between; where the rows do not fit the resident kernel, the
// tiled one over the same rows.
std::vector<at::Tensor> gpu_topk_flat_tokens(
    KVIDX_TABLE_PARAMS, at::Tensor tokens_flat, at::Tensor offsets,
    int64_t model_id, at::Tensor filter_words, at::Tensor weights,
    int64_t num_pods, int64_t epoch, int64_t init_hash_bits,
    int64_t block_size, int64_t n_tiers, int64_t algo, int64_t top_n);
// The ragged device chain: flat tokens (host or device, int64 or int32) ->
// {hashes int64 [total_chunks], h_off int32 [B+1]} on the device, the
// layout and the content of hash_chain_batch with every parent
// init_hash_bits.  Block sizes 4/8/16/32/64.  Stage and chain run over
// per-wave images (plan_ragged_waves), so nothing is padded to the batch's
// longest prompt and no image cap applies.
std::vector<at::Tensor> gpu_hash_chain_ragged(at::Tensor tokens_flat,
                                              at::Tensor offsets,
                                              int64_t init_hash_bits,
                                              int64_t block_size,
                                              int64_t algo);
// gpu_score_flat_tokens / gpu_topk_flat_tokens over the ragged chain:
// stage -> chain -> gpu_score_hashes / gpu_topk_hashes on the CSR hashes,
// on the current stream with no host wait in between.  Same results bit
// for bit.
at::Tensor gpu_score_flat_tokens_ragged(
    KVIDX_TABLE_PARAMS, at::Tensor tokens_flat, at::Tensor offsets,
    int64_t model_id, at::Tensor filter_words, at::Tensor weights,
    int64_t num_pods, int64_t epoch, int64_t init_hash_bits,
    int64_t block_size, int64_t n_tiers, int64_t algo);
std::vector<at::Tensor> gpu_topk_flat_tokens_ragged(
    KVIDX_TABLE_PARAMS, at::Tensor tokens_flat, at::Tensor offsets,
    int64_t model_id, at::Tensor filter_words, at::Tensor weights,
    int64_t num_pods, int64_t epoch, int64_t init_hash_bits,
    int64_t block_size, int64_t n_tiers, int64_t algo, int64_t top_n);
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
// The wave-tiled ingest chain: gpu_apply_events_split_tr's bursts (no
// batch-local parent, no store+remove conflict; host verified) at any block
// size 1..65535 and without the [max_tokens, E] rectangle.  tokens_flat
// int32 on the device; tok_off, eh_off and ev_type on the HOST (the plan
// reads them, and their device copies ride the plan's one upload); the
// rest on the device.  plan_event_waves -> one upload ->
// k_stage_ragged_waves -> the event-root entry of a wave chain kernel ->
// k_event_inserts, on the current stream with no host wait in between.
void gpu_apply_events_split_waves(KVIDX_TABLE_PARAMS, at::Tensor tokens_flat,
                                  at::Tensor tok_off, at::Tensor ehashes,
                                  at::Tensor eh_off, at::Tensor parents,
                                  at::Tensor has_parent, at::Tensor ev_type,
                                  at::Tensor pod_entry, at::Tensor ev_of,
                                  at::Tensor model_of, int64_t init_hash_bits,
                                  int64_t block_size, int64_t epoch,
                                  int64_t shard_id, int64_t num_shards,
                                  int64_t algo);
// The linked wave ingest: the waves op for bursts whose events chain from
// blocks the same burst stores (no store+remove conflict; host verified).
// The waves op's arguments plus link / level int32 [E] on the HOST, as
// plan_event_links returns them.  plan_linked_event_waves -> one upload ->
// k_stage_ragged_waves -> the linked entry of a wave chain kernel once per
// level, in level order -> k_event_inserts, on the current stream with no
// host wait in between; no batch map, no k_event_chains.  Refuses a bad
// block size or algo and a link that points at or past its own event
// before any launch.
void gpu_apply_events_split_linked(
    KVIDX_TABLE_PARAMS, at::Tensor tokens_flat, at::Tensor tok_off,
    at::Tensor ehashes, at::Tensor eh_off, at::Tensor parents,
    at::Tensor has_parent, at::Tensor ev_type, at::Tensor pod_entry,
    at::Tensor ev_of, at::Tensor model_of, at::Tensor link, at::Tensor level,
    int64_t init_hash_bits, int64_t block_size, int64_t epoch,
    int64_t shard_id, int64_t num_shards, int64_t algo);
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

// Histogram bins of a census, after the checks both census ops share.
inline int64_t census_bins_checked(KVIDX_TABLE_PARAMS, int64_t model_id,
                                   int64_t num_pods, int64_t n_tiers) {
  TORCH_CHECK(num_pods >= 1 && num_pods <= MAX_PODS, "num_pods must be 1..",
              MAX_PODS);
  TORCH_CHECK(n_tiers >= 1 && n_tiers <= MAX_TIERS, "n_tiers must be 1..",
              MAX_TIERS);
  TORCH_CHECK(model_id >= -1 && model_id <= (int64_t)META_MODEL_MASK,
              "model_id out of range (-1 = every model)");
  TORCH_CHECK(pods_per_key >= 1 && pods_per_key <= 4096,
              "pods_per_key out of range");
  TORCH_CHECK(pods.numel() == keys.numel() * pods_per_key,
              "pods must hold capacity * pods_per_key entries");
  TORCH_CHECK(meta.numel() == keys.numel() && e_meta.numel() == keys.numel(),
              "meta and e_meta must hold capacity words");
  return num_pods * n_tiers;
}

// Pod columns P of a score matrix, after the checks cpu_score_topk and
// gpu_topk_rows share.
inline int64_t topk_rows_checked(const at::Tensor& scores, int64_t top_n) {
  TORCH_CHECK(top_n >= 1 && top_n <= MAX_TOPK, "top_n must be 1..", MAX_TOPK);
  TORCH_CHECK(scores.dtype() == at::kFloat && scores.dim() == 2 &&
                  scores.is_contiguous(),
              "scores must be a contiguous float32 [B, P] tensor");
  const int64_t P = scores.size(1);
  TORCH_CHECK(P >= 1 && P <= MAX_PODS, "scores must have 1..", MAX_PODS,
              " pod columns");
  return P;
}

// Host half of the ragged staging: what the offsets say about a batch.
// One int32 buffer [n_chunks (B) | token offsets (B+1)] so that both go
// up in one copy.
struct RaggedPlan {
  int64_t B = 0, max_k = 0, total_chunks = 0;
  at::Tensor host;  // int32 [2B+1]
};

inline RaggedPlan plan_ragged(const at::Tensor& tokens,
                              const at::Tensor& offsets, int64_t block_size) {
  TORCH_CHECK(block_size > 0, "block_size must be positive");
  TORCH_CHECK(offsets.dtype() == at::kLong && offsets.dim() == 1 &&
                  offsets.numel() >= 1,
              "offsets must be an int64 [B+1] tensor");
  TORCH_CHECK(tokens.dim() == 1 &&
                  (tokens.dtype() == at::kLong || tokens.dtype() == at::kInt),
              "tokens must be a flat int64 or int32 tensor");
  auto off = offsets.to(at::kCPU).contiguous();
  const int64_t* offp = off.data_ptr<int64_t>();
  RaggedPlan p;
  p.B = off.numel() - 1;
  // the kernel trusts these: it reads tokens[off[b] + i] unchecked
  TORCH_CHECK(offp[0] >= 0 && offp[p.B] <= tokens.numel(),
              "offsets reach outside the token tensor");
  TORCH_CHECK(offp[p.B] <= INT32_MAX,
              "more than 2^31 - 1 tokens in one batch");
  p.host = at::empty({2 * p.B + 1}, at::kInt);
  int32_t* nc = p.host.data_ptr<int32_t>();
  int32_t* o32 = nc + p.B;
  for (int64_t b = 0; b < p.B; ++b) {
    int64_t len = offp[b + 1] - offp[b];
    TORCH_CHECK(len >= 0, "offsets must not decrease");
    int64_t k = len / block_size;
    nc[b] = (int32_t)k;
    o32[b] = (int32_t)offp[b];
    p.max_k = std::max(p.max_k, k);
    p.total_chunks += k;
  }
  o32[p.B] = (int32_t)offp[p.B];
  return p;
}

// Host half of the ragged (wave-tiled) device chain.  The prompts, sorted
// by whole chunks descending (stable: ties by ascending prompt index), are
// cut into waves of 64; wave g gets a token image int32 [wave_k[g] *
// block_size][64] of its own, only as tall as its longest prompt, and the
// hashes come out in CSR form in the caller's prompt order.  Waves made up
// of zero-chunk prompts alone are not planned: G counts waves with
// wave_k > 0.
// One int32 buffer, so that everything goes up in one copy:
//   [img_off int64 (G+1) | n_chunks (B) | tok_off (B+1) | h_off (B+1) |
//    perm (64 G) | wave_k (G) | tile_start (G+1) | tail]
//  - perm[64 g + r]: the prompt in row r of wave g, -1 past the batch;
//  - wave_k[g]: n_chunks of the wave's first prompt, its maximum;
//  - img_off[g]: element offset of wave g's image, the sum of wave_k *
//    block_size * 64 before it, so every image starts on a 256 B line;
//    img_off[G] is the size of the whole image;
//  - tile_start[g]: 64-position staging tiles before wave g;
//  - h_off: exclusive prefix sum of n_chunks in the caller's order.
// img_off leads the buffer, which keeps its int64 words 8-byte aligned.
struct WavePlan {
  int64_t B = 0, G = 0, max_k = 0, total_chunks = 0;
  int64_t image_elems = 0, tiles = 0;
  int64_t tail = 0;  // caller's int32 words behind tile_start
  // the linked event plan only (plan_linked_event_waves): levels, and where
  // link [B] and level_wave [n_levels + 1] lie in the tail
  int64_t n_levels = 0, at_link = 0, at_level_wave = 0;
  at::Tensor host;   // int32 [2 (G+1) + 3 B + 2 + 66 G + 1 + tail]
  int64_t at_img_off() const { return 0; }
  int64_t at_n_chunks() const { return 2 * (G + 1); }
  int64_t at_tok_off() const { return at_n_chunks() + B; }
  int64_t at_h_off() const { return at_tok_off() + B + 1; }
  int64_t at_perm() const { return at_h_off() + B + 1; }
  int64_t at_wave_k() const { return at_perm() + 64 * G; }
  int64_t at_tile_start() const { return at_wave_k() + G; }
  int64_t at_tail() const { return at_tile_start() + G + 1; }
  int64_t words() const { return at_tail() + tail; }
  // pieces of `buf`, the host buffer or its copy on the device
  at::Tensor i32(const at::Tensor& buf, int64_t at, int64_t n) const {
    return buf.slice(0, at, at + n);
  }
  at::Tensor img_off(const at::Tensor& buf) const {
    return buf.slice(0, 0, 2 * (G + 1)).view(at::kLong);
  }
};

// The wave half of a plan, shared by the prompt plan and the event plans:
// r holds the lanes' n_chunks and tok_off; h_off_src is the lanes' h_off
// [B+1], or null for the exclusive prefix sum of n_chunks; tail_words int32
// words are left to the caller behind tile_start.
// level: null, or the lanes' levels [B] (plan_event_links).  The lanes with
// a whole chunk are then ordered by (level ascending, chunks descending,
// index ascending) and the waves are cut per level: no wave holds two
// levels, a level's last wave is padded with -1 rows, and level_wave [the
// levels' count + 1] gets the first wave of each level.  Lanes without a
// chunk get no row then.
inline WavePlan plan_waves(const RaggedPlan& r, int64_t block_size,
                           const int32_t* h_off_src, int64_t tail_words,
                           const int32_t* level = nullptr,
                           std::vector<int32_t>* level_wave = nullptr) {
  const int32_t* nc = r.host.data_ptr<int32_t>();
  WavePlan p;
  p.B = r.B;
  p.max_k = r.max_k;
  p.total_chunks = r.total_chunks;
  p.tail = tail_words;
  TORCH_CHECK(p.total_chunks <= INT32_MAX,
              "more than 2^31 - 1 chunks in one batch");
  std::vector<int32_t> order(p.B);
  for (int64_t b = 0; b < p.B; ++b) order[b] = (int32_t)b;
  if (level)
    std::stable_sort(order.begin(), order.end(),
                     [nc, level](int32_t a, int32_t b) {
                       if ((nc[a] > 0) != (nc[b] > 0)) return nc[a] > 0;
                       if (nc[a] > 0 && level[a] != level[b])
                         return level[a] < level[b];
                       return nc[a] > nc[b];
                     });
  else
    std::stable_sort(order.begin(), order.end(),
                     [nc](int32_t a, int32_t b) { return nc[a] > nc[b]; });
  int64_t live = 0;  // lanes with a whole chunk: they sort first
  while (live < p.B && nc[order[live]] > 0) ++live;
  // rows[64 g + r]: the lane in row r of wave g.  Without levels the last
  // wave takes chunkless lanes as well, as far as the batch goes.
  std::vector<int32_t> rows;
  if (!level) {
    rows.assign(64 * ((live + 63) / 64), -1);
    std::copy(order.begin(),
              order.begin() + std::min<int64_t>(p.B, (int64_t)rows.size()),
              rows.begin());
  } else {
    level_wave->assign(1, 0);
    for (int64_t i = 0; i < live;) {
      const int32_t lv = level[order[i]];
      TORCH_CHECK(lv >= (int64_t)level_wave->size() - 1,
                  "levels must not be negative");
      int64_t end = i;
      while (end < live && level[order[end]] == lv) ++end;
      level_wave->resize(lv + 1, (int32_t)(rows.size() / 64));  // empty levels
      rows.insert(rows.end(), order.begin() + i, order.begin() + end);
      rows.resize((rows.size() + 63) / 64 * 64, -1);
      level_wave->push_back((int32_t)(rows.size() / 64));
      i = end;
    }
  }
  p.G = (int64_t)rows.size() / 64;
  p.host = at::empty({p.words()}, at::kInt);
  int32_t* w = p.host.data_ptr<int32_t>();
  int64_t* img_off = reinterpret_cast<int64_t*>(w);
  std::copy(nc, nc + 2 * p.B + 1, w + p.at_n_chunks());  // and tok_off
  int32_t* h_off = w + p.at_h_off();
  if (h_off_src) {
    std::copy(h_off_src, h_off_src + p.B + 1, h_off);
  } else {
    h_off[0] = 0;
    for (int64_t b = 0; b < p.B; ++b) h_off[b + 1] = h_off[b] + nc[b];
  }
  std::copy(rows.begin(), rows.end(), w + p.at_perm());
  int32_t* wave_k = w + p.at_wave_k();
  int32_t* tile_start = w + p.at_tile_start();
  img_off[0] = 0;
  tile_start[0] = 0;
  for (int64_t g = 0; g < p.G; ++g) {
    // a wave's first row is its longest lane
    wave_k[g] = nc[rows[64 * g]];
    const int64_t trips = (int64_t)wave_k[g] * block_size;
    img_off[g + 1] = img_off[g] + trips * 64;
    const int64_t tiles = tile_start[g] + (trips + 63) / 64;
    TORCH_CHECK(tiles <= INT32_MAX, "too many staging tiles in one batch");
    tile_start[g + 1] = (int32_t)tiles;
  }
  p.image_elems = img_off[p.G];
  p.tiles = tile_start[p.G];
  return p;
}

inline WavePlan plan_ragged_waves(const at::Tensor& tokens,
                                  const at::Tensor& offsets,
                                  int64_t block_size) {
  return plan_waves(plan_ragged(tokens, offsets, block_size), block_size,
                    nullptr, 0);
}

// Host half of the wave-tiled ingest chain (gpu_apply_events_split_waves):
// plan_ragged_waves with EVENTS as lanes.  tok_off / eh_off int32 [E+1] and
// ev_type uint8 [E] on the host, as FlatEvents holds them.
//  - n_chunks[e] is event_chain_len's value (hip_ops.hip), and 0 for a
//    BlockRemoved event and for a store whose engine-hash count differs
//    from its whole chunks: those sort last and get no wave;
//  - h_off[e] = eh_off[e], not a prefix sum of n_chunks: a removal or a
//    dropped store still owns its engine hashes' slots, so chunk c of
//    event e lies at eh_off[e] + c, where k_event_inserts reads it;
//  - the tail behind tile_start is ev_type, E bytes in (E + 3) / 4 words,
//    so that the one upload carries all k_event_inserts reads as well.
// The stage kernel reads tokens[tok_off[e] + i] and the chain kernels write
// out[eh_off[e] + c] unchecked, so both offset arrays are checked here
// against n_tokens and n_hashes.
// links: null, or what plan_linked_event_waves adds (below).
struct EventLinks {
  int64_t n_levels = 0;
  at::Tensor link, level;  // int32 [E] each, on the host
};
inline WavePlan plan_event_waves(const at::Tensor& tok_off,
                                 const at::Tensor& eh_off,
                                 const at::Tensor& ev_type, int64_t n_tokens,
                                 int64_t n_hashes, int64_t block_size,
                                 const EventLinks* links = nullptr) {
  TORCH_CHECK(stream_chain_block_size_ok(block_size),
              "the wave-tiled ingest chain takes block sizes 1..65535");
  const auto host_1d = [](const at::Tensor& t, at::ScalarType ty) {
    return t.device().is_cpu() && t.dtype() == ty && t.dim() == 1 &&
           t.is_contiguous();
  };
  TORCH_CHECK(host_1d(tok_off, at::kInt) && host_1d(eh_off, at::kInt) &&
                  host_1d(ev_type, at::kByte),
              "tok_off / eh_off must be contiguous int32 and ev_type uint8 "
              "host tensors");
  const int64_t E = ev_type.numel();
  TORCH_CHECK(tok_off.numel() == E + 1 && eh_off.numel() == E + 1,
              "tok_off and eh_off must hold E + 1 offsets");
  const int32_t* to = tok_off.data_ptr<int32_t>();
  const int32_t* eo = eh_off.data_ptr<int32_t>();
  const uint8_t* ty = ev_type.data_ptr<uint8_t>();
  TORCH_CHECK(to[0] >= 0 && to[E] <= n_tokens,
              "tok_off reaches outside the token tensor");
  TORCH_CHECK(eo[0] >= 0 && eo[E] <= n_hashes,
              "eh_off reaches outside the engine hashes");
  RaggedPlan r;
  r.B = E;
  r.host = at::empty({2 * E + 1}, at::kInt);
  int32_t* nc = r.host.data_ptr<int32_t>();
  std::copy(to, to + E + 1, nc + E);
  for (int64_t e = 0; e < E; ++e) {
    TORCH_CHECK(to[e + 1] >= to[e] && eo[e + 1] >= eo[e],
                "event offsets must not decrease");
    const int64_t k = (to[e + 1] - to[e]) / block_size;
    nc[e] = ty[e] != 1 && k == eo[e + 1] - eo[e] ? (int32_t)k : 0;
    r.max_k = std::max<int64_t>(r.max_k, nc[e]);
    r.total_chunks += nc[e];
  }
  const int64_t type_words = (E + 3) / 4;
  WavePlan p;
  if (!links) {
    p = plan_waves(r, block_size, eo, type_words);
  } else {
    // The chain kernels read scratch[link[e]] unchecked and trust the
    // launch order, so: a link names a block before its own event's, of a
    // store with a chain, one level below.
    TORCH_CHECK(host_1d(links->link, at::kInt) && links->link.numel() == E &&
                    host_1d(links->level, at::kInt) &&
                    links->level.numel() == E && links->n_levels >= 0,
                "link and level must be contiguous int32 [E] host tensors");
    const int32_t* link = links->link.data_ptr<int32_t>();
    const int32_t* level = links->level.data_ptr<int32_t>();
    for (int64_t e = 0; e < E; ++e) {
      TORCH_CHECK(level[e] >= 0 && level[e] < links->n_levels,
                  "level[", e, "] is outside the burst's levels");
      if (link[e] < 0) {
        TORCH_CHECK(link[e] == -1 && level[e] == 0,
                    "an event without a link is -1 at level 0");
        continue;
      }
      TORCH_CHECK(link[e] < eo[e], "link[", e,
                  "] points at or past its own event");
      const int64_t src = std::upper_bound(eo, eo + E + 1, link[e]) - eo - 1;
      TORCH_CHECK(nc[src] > 0 && level[e] == level[src] + 1,
                  "link[", e, "] must name a block of a kept store one "
                  "level below");
    }
    std::vector<int32_t> level_wave;
    p = plan_waves(r, block_size, eo, type_words + E + links->n_levels + 1,
                   level, &level_wave);
    level_wave.resize(links->n_levels + 1, (int32_t)p.G);  // chainless levels
    p.n_levels = links->n_levels;
    p.at_link = p.at_tail() + type_words;
    p.at_level_wave = p.at_link + E;
    int32_t* w = p.host.data_ptr<int32_t>();
    std::copy(link, link + E, w + p.at_link);
    std::copy(level_wave.begin(), level_wave.end(), w + p.at_level_wave);
  }
  uint8_t* t8 = reinterpret_cast<uint8_t*>(p.host.data_ptr<int32_t>() +
                                           p.at_tail());
  std::fill(t8 + E, t8 + 4 * type_words, (uint8_t)0);
  std::copy(ty, ty + E, t8);
  return p;
}

// Host half of the linked wave ingest (gpu_apply_events_split_linked), part
// one: which earlier block of its own group each event chains from.  All
// arguments on the host, as FlatEvents holds them (ehashes / parents int64,
// has_parent uint8, grp_off int32 [G+1] covering the E events).
//  - link[e]: the index into ehashes / req_scratch of the block that
//    k_event_chains takes through dev_bmap_find: the LATEST block bi with
//    eh_off[first event of e's group] <= bi < eh_off[e] that belongs to a
//    kept store (ev_type 0, event_chain_len >= 0) and has ehashes[bi] ==
//    parents[e]; -1 for an event without a parent or without such a block
//    (a block of another group, of a later event, of a removed or dropped
//    event: the lane then resolves through the engine map, as RootEvents
//    does), and for an event that is no kept store itself;
//  - level[e]: 0 where link[e] < 0, else level[event of link[e]] + 1;
//  - n_levels: the largest level + 1, 0 for no event.
// One forward pass with one hash map: hash -> its latest block so far.  The
// groups follow each other, so an entry below the current group's first
// block is a stale one of an earlier group and counts as absent.
inline EventLinks plan_event_links(const at::Tensor& ehashes,
                                   const at::Tensor& eh_off,
                                   const at::Tensor& tok_off,
                                   const at::Tensor& ev_type,
                                   const at::Tensor& parents,
                                   const at::Tensor& has_parent,
                                   const at::Tensor& grp_off,
                                   int64_t block_size) {
  TORCH_CHECK(block_size >= 1, "block_size must be positive");
  const auto host_1d = [](const at::Tensor& t, at::ScalarType ty) {
    return t.device().is_cpu() && t.dtype() == ty && t.dim() == 1 &&
           t.is_contiguous();
  };
  TORCH_CHECK(host_1d(ehashes, at::kLong) && host_1d(parents, at::kLong) &&
                  host_1d(eh_off, at::kInt) && host_1d(tok_off, at::kInt) &&
                  host_1d(grp_off, at::kInt) && host_1d(ev_type, at::kByte) &&
                  host_1d(has_parent, at::kByte),
              "plan_event_links takes contiguous host tensors: ehashes / "
              "parents int64, the offsets int32, ev_type / has_parent uint8");
  const int64_t E = ev_type.numel();
  const int64_t G = grp_off.numel() - 1;
  TORCH_CHECK(eh_off.numel() == E + 1 && tok_off.numel() == E + 1 &&
                  parents.numel() == E && has_parent.numel() == E && G >= 0,
              "the event arrays must hold E (offsets: E + 1) entries");
  const uint64_t* eh = u64p(ehashes);
  const uint64_t* par = u64p(parents);
  const int32_t* eo = eh_off.data_ptr<int32_t>();
  const int32_t* to = tok_off.data_ptr<int32_t>();
  const int32_t* go = grp_off.data_ptr<int32_t>();
  const uint8_t* ty = ev_type.data_ptr<uint8_t>();
  const uint8_t* hp = has_parent.data_ptr<uint8_t>();
  TORCH_CHECK(eo[0] >= 0 && eo[E] <= ehashes.numel(),
              "eh_off reaches outside the engine hashes");
  TORCH_CHECK(go[0] == 0 && go[G] == E, "grp_off must cover the events");
  EventLinks r;
  r.link = at::empty({E}, at::kInt);
  r.level = at::empty({E}, at::kInt);
  int32_t* link = r.link.data_ptr<int32_t>();
  int32_t* level = r.level.data_ptr<int32_t>();
  struct Block { int32_t index, event; };
  std::unordered_map<uint64_t, Block> latest;
  latest.reserve((size_t)ehashes.numel());
  for (int64_t g = 0; g < G; ++g) {
    TORCH_CHECK(go[g + 1] >= go[g], "grp_off must not decrease");
    const int32_t first_block = eo[go[g]];
    for (int64_t e = go[g]; e < go[g + 1]; ++e) {
      TORCH_CHECK(to[e + 1] >= to[e] && eo[e + 1] >= eo[e],
                  "event offsets must not decrease");
      link[e] = -1;
      level[e] = 0;
      if (ty[e] != 0 || (to[e + 1] - to[e]) / block_size != eo[e + 1] - eo[e])
        continue;  // no kept store: chains nothing, is nobody's parent
      if (hp[e]) {
        const auto it = latest.find(par[e]);
        if (it != latest.end() && it->second.index >= first_block) {
          link[e] = it->second.index;
          level[e] = level[it->second.event] + 1;
        }
      }
      for (int32_t bi = eo[e]; bi < eo[e + 1]; ++bi)
        latest[eh[bi]] = Block{bi, (int32_t)e};
      r.n_levels = std::max<int64_t>(r.n_levels, level[e] + 1);
    }
  }
  if (E > 0) r.n_levels = std::max<int64_t>(r.n_levels, 1);
  return r;
}

// Part two: plan_event_waves with the lanes ordered by (level ascending,
// chunks descending, index ascending) and the waves cut per level
// (plan_waves), so that the chain kernels can run level by level over one
// set of images: wave g of level l is level_wave[l] <= g < level_wave[l+1].
// The tail behind tile_start is then [ev_type (E + 3) / 4 words | link (E) |
// level_wave (n_levels + 1)] - still one upload.  h_off stays eh_off.
inline WavePlan plan_linked_event_waves(const at::Tensor& tok_off,
                                        const at::Tensor& eh_off,
                                        const at::Tensor& ev_type,
                                        const EventLinks& links,
                                        int64_t n_tokens, int64_t n_hashes,
                                        int64_t block_size) {
  return plan_event_waves(tok_off, eh_off, ev_type, n_tokens, n_hashes,
                          block_size, &links);
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
