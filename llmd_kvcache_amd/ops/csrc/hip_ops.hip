// hip_ops.hip - gfx950 (MI355X/CDNA4) kernels for the KV-block index.
//
// Design (MI355X-first, not a port - the reference does all of this on CPU
// with Go maps + LRU locks):
//  - the block->pod table is HBM3E-resident (288 GB/GPU allows >1e9 keys);
//    probing is lock-free open addressing with device-scope atomics
//    (cross-XCD safe: atomicCAS on global memory is device scope);
//  - read path: one workgroup per prompt; all K key probes issue in
//    PARALLEL (the prefix early-stop is applied after the fact during the
//    in-LDS mask walk), so per-prompt latency is ~2 dependent HBM reads,
//    not K of them - the CPU reference walks keys serially;
//  - per-(key,tier) pod-bitmask accumulation in LDS, then the workgroup's
//    four waves walk the masks in key order, each taking every fourth
//    64-pod word, computing longest-prefix scores with the active pod set
//    in registers (lane l owns pod bit l of its word) - scoring parity
//    with kvblock_scorer.go:108-151;
//  - write path: events arrive grouped by pod (per-pod ordering guarantee
//    of kvevents/pool.go:132-144 preserved).  The usual route is phase
//    split: request-key chains one lane per event (or per pod-group when
//    a batch refers to its own blocks as parents), then one thread per
//    block for the inserts and removals.  A batch that stores and removes
//    the same engine hash takes the serial kernel: one wave per
//    pod-group, lane 0 streams the chain (token_processor.go:94-123)
//    and the block inserts fan out across the 64 lanes;
//  - hash-chain batch kernels: one lane per prompt over transposed
//    tokens, wave64-dense; the FNV chain lives in registers (streaming
//    CBOR->FNV, no scratch), the SHA-256 chain packs its payload into an
//    LDS column per lane.
// Each table decision (probe, remove, store, ownership, parent, event
// length) is one device helper below; the kernels are calls to them.

#include <hip/hip_runtime.h>
#include <ATen/cuda/CUDAContext.h>

#include "kvidx_ops.h"

namespace kvidx {

#define DEV __device__ __forceinline__

DEV int64_t dev_table_find(const Table& v, uint64_t h, uint32_t model) {
  return probe_find(v.keys, v.meta, v.cap_mask, h, model);
}
DEV int64_t dev_emap_find(const Table& v, uint64_t h, uint32_t model) {
  return probe_find(v.e_keys, v.e_meta, v.cap_mask, h, model);
}

// Lock-free probe-or-insert. Claims free slots via atomicCAS on the key
// word (deterministic probe order makes same-key racers converge on the
// same slot); tombstone resurrection via atomicCAS on meta; window-full
// falls back to stealing the lowest-stamp live slot (approx LRU).
DEV int64_t dev_table_put(const Table& v, uint64_t h, uint32_t model,
                          int32_t epoch) {
  h = remap_hash(h);
  uint64_t s = probe_start(h, v.cap_mask);
  int64_t first_tomb = -1;
  int64_t victim = -1;
  int32_t victim_stamp = 0;
  for (int t = 0; t < PROBE_MAX; ++t) {
    uint64_t i = (s + t) & v.cap_mask;
    uint64_t k = v.keys[i];
    if (k == 0) {
      uint64_t prev = atomicCAS((unsigned long long*)&v.keys[i], 0ull,
                                (unsigned long long)h);
      if (prev == 0) {  // claimed fresh slot (pods are zero-initialized)
        __threadfence();
        atomicExch(&v.meta[i], META_OCC | (model & META_MODEL_MASK));
        v.stamp[i] = epoch;
        return (int64_t)i;
      }
      k = prev;  // lost the race; re-evaluate this slot
    }
    if (k == h) {
      uint32_t m = v.meta[i];
      if (!(m & META_OCC)) return (int64_t)i;  // mid-insert by a racer
      if (!(m & META_TOMB)) {
        if ((m & META_MODEL_MASK) == model) {
          v.stamp[i] = epoch;
          return (int64_t)i;
        }
        continue;  // same hash, different model (astronomically rare)
      }
      // tombstone with our key: resurrect
      uint32_t want = META_OCC | (model & META_MODEL_MASK);
      atomicCAS(&v.meta[i], m, want);
      v.stamp[i] = epoch;
      return (int64_t)i;
    }
    uint32_t m = v.meta[i];
    if (m & META_TOMB) {
      if (first_tomb < 0) first_tomb = (int64_t)i;
    } else if (m & META_OCC) {
      int32_t st = v.stamp[i];
      if (victim < 0 || st < victim_stamp) {
        victim = (int64_t)i;
        victim_stamp = st;
      }
    }  // !OCC and k!=0: mid-insert elsewhere; skip
  }
  // Window exhausted: steal (approximate LRU eviction under pressure).
  int64_t i = first_tomb >= 0 ? first_tomb : victim;
  if (i < 0) i = (int64_t)s;
  for (int j = 0; j < v.pods_per_key; ++j) v.pods[i * v.pods_per_key + j] = 0;
  atomicExch((unsigned long long*)&v.keys[i], (unsigned long long)h);
  __threadfence();
  atomicExch(&v.meta[i], META_OCC | (model & META_MODEL_MASK));
  v.stamp[i] = epoch;
  return i;
}

DEV void dev_pod_set_add(const Table& v, int64_t slot, uint32_t entry,
                         int32_t epoch) {
  KVIDX_ASSERT(slot >= 0 && (uint64_t)slot <= v.cap_mask);
  KVIDX_ASSERT(entry != 0);
  uint32_t* p = v.pods + slot * v.pods_per_key;
  for (int j = 0; j < v.pods_per_key; ++j)
    if (p[j] == entry) return;
  for (int j = 0; j < v.pods_per_key; ++j) {
    uint32_t cur = p[j];
    if (cur == 0) {
      uint32_t prev = atomicCAS(&p[j], 0u, entry);
      if (prev == 0 || prev == entry) return;
    } else if (cur == entry) {
      return;
    }
  }
  atomicExch(&p[(uint32_t)epoch % v.pods_per_key], entry);  // full: overwrite
}

// Meta word of an engine-map slot whose key word is set, read past the L1
// (another CU may have published it since this one cached the line).  A
// writer that claimed the key word publishes the meta a store, a fence
// and an atomic later, waiting for nobody, so an unpublished word is
// polled: a bounded number of times, and the last word read is returned
// either way.
constexpr int EMAP_PUBLISH_POLLS = 1 << 12;
DEV uint32_t dev_emap_published_meta(const uint32_t* p) {
  uint32_t m = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int polls = 0; !(m & META_OCC) && polls < EMAP_PUBLISH_POLLS; ++polls) {
    __builtin_amdgcn_s_sleep(1);
    m = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return m;
}

// Engine map probe-or-insert, the device twin of cpu_ops.cpp's emap_put:
// a slot is this writer's only if it holds (h, model).  A live slot with
// the same key word under another model is somebody else's slot, like any
// other key's: probed past, and at most the window's ordinary victim.
// Free slots are claimed by atomicCAS on the key word, and racers of one
// (hash, model) walk the same slots in the same order, so they end on one
// slot.  A key word equal to h whose meta is not yet published belongs to
// a racer mid-insert whose model is unknown: the meta is polled until it
// is there (dev_emap_published_meta).  The claim publishes inside the
// loop body, ahead of that poll and with no exit of its own, so that a
// racer in the same wave has published before a lane of that wave polls.
// If the poll runs out the slot counts as another model's.
DEV void dev_emap_put(const Table& v, uint64_t h, uint32_t model,
                      uint64_t val) {
  h = remap_hash(h);
  const uint32_t want = META_OCC | (model & META_MODEL_MASK);
  uint64_t s = probe_start(h, v.cap_mask);
  int64_t first_tomb = -1;
  int64_t victim = -1;
  for (int t = 0; t < PROBE_MAX; ++t) {
    uint64_t i = (s + t) & v.cap_mask;
    uint64_t k = v.e_keys[i];
    int claimed = 0;
    if (k == 0) {
      k = atomicCAS((unsigned long long*)&v.e_keys[i], 0ull,
                    (unsigned long long)h);
      if (k == 0) {
        v.e_vals[i] = val;
        __threadfence();
        atomicExch(&v.e_meta[i], want);
        claimed = 1;
      }
    }
    // opaque to the optimizer: the publish above stays an if-then inside
    // the loop instead of moving to a loop exit, which a wave runs only
    // after its last lane has left the loop
    asm volatile("" : "+v"(claimed)::"memory");
    if (claimed) return;
    uint32_t m;
    if (k == h) {
      m = dev_emap_published_meta(&v.e_meta[i]);
      if ((m & META_OCC) && (m & META_TOMB)) {
        // our key, dead: whoever swings the meta word owns the slot
        if (atomicCAS(&v.e_meta[i], m, want) == m) {
          v.e_vals[i] = val;
          return;
        }
        m = __hip_atomic_load(&v.e_meta[i], __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
      }
      if ((m & META_OCC) && !(m & META_TOMB) &&
          (m & META_MODEL_MASK) == (model & META_MODEL_MASK)) {
        v.e_vals[i] = val;  // refresh value (idempotent for same chain)
        return;
      }
    } else {
      m = v.e_meta[i];
    }
    if (m & META_TOMB) {
      if (first_tomb < 0) first_tomb = (int64_t)i;
    } else if ((m & META_OCC) && victim < 0) {
      victim = (int64_t)i;
    }
  }
  int64_t i = first_tomb >= 0 ? first_tomb : victim;
  if (i < 0) i = (int64_t)s;
  atomicExch((unsigned long long*)&v.e_keys[i], (unsigned long long)h);
  v.e_vals[i] = val;
  __threadfence();
  atomicExch(&v.e_meta[i], META_OCC | (model & META_MODEL_MASK));
}

// Remove the n pod entries from the block an engine hash maps to and
// tombstone the block when its pod set empties.  The engine mapping is
// retained (replica determinism under sharding + chain continuity; see
// the cpu_evict note).  Entries outer, slots inner.
DEV void dev_remove_pods(const Table& v, uint64_t engine_hash, uint32_t model,
                         const uint32_t* __restrict__ entries, int n) {
  int64_t ei = dev_emap_find(v, engine_hash, model);
  if (ei < 0) return;
  uint64_t req = v.e_vals[ei];
  int64_t slot = dev_table_find(v, req, model);
  if (slot < 0) return;
  uint32_t* p = v.pods + slot * v.pods_per_key;
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < v.pods_per_key; ++k)
      atomicCAS(&p[k], entries[j], 0u);
  bool empty = true;
  for (int k = 0; k < v.pods_per_key; ++k)
    if (p[k] != 0) { empty = false; break; }
  if (empty) atomicOr(&v.meta[slot], META_TOMB);
}

// Store one block: publish engine hash -> request key (on every shard: the
// engine map is replicated), then, on the shard that owns the request
// key, insert it and add the n pod entries.
DEV void dev_store_block(const Table& v, uint64_t engine_hash, uint64_t req,
                         uint32_t model, const uint32_t* __restrict__ entries,
                         int n, int32_t epoch, int shard_id, int num_shards,
                         int emap_write) {
  if (emap_write) dev_emap_put(v, engine_hash, model, remap_hash(req));
  if (!owns_key(req, shard_id, num_shards)) return;
  int64_t slot = dev_table_put(v, req, model, epoch);
  for (int j = 0; j < n; ++j) dev_pod_set_add(v, slot, entries[j], epoch);
}

// Chunk count of BlockStored event e, or -1 when its engine-hash count
// differs from the token-derived chain length.  The reference Add() (and
// the CPU digest path) rejects such an event whole; every kernel that
// reads an event asks here, so CPU and GPU replicas stay convergent on
// malformed streams.
DEV int event_chain_len(const int32_t* __restrict__ tok_off,
                        const int32_t* __restrict__ eh_off, int64_t e,
                        int block_size) {
  KVIDX_ASSERT(eh_off[e + 1] >= eh_off[e] && tok_off[e + 1] >= tok_off[e]);
  const int n_chunks = (tok_off[e + 1] - tok_off[e]) / block_size;
  return n_chunks == eh_off[e + 1] - eh_off[e] ? n_chunks : -1;
}

// Chain parent of event e: the request key its parent engine hash maps to
// in the persistent engine map, else (no parent, or unknown) the root.
DEV uint64_t dev_event_parent(const Table& v,
                              const uint8_t* __restrict__ has_parent,
                              const uint64_t* __restrict__ parents,
                              const int32_t* __restrict__ model_of, int64_t e,
                              uint64_t init_hash) {
  if (!has_parent[e]) return init_hash;
  int64_t ei = dev_emap_find(v, parents[e], (uint32_t)model_of[e]);
  return ei >= 0 ? v.e_vals[ei] : init_hash;
}

// Probe one key and OR its visible pod entries into its per-tier mask
// words mk [n_tiers, W] (LDS or global).
// Returns: 0 absent, 1 present (raw pods nonzero), 2 present-but-empty.
DEV int dev_probe_collect(const Table& v, uint64_t h, uint32_t model,
                          const uint64_t* __restrict__ filter, int has_filter,
                          int num_pods, int W, int32_t epoch,
                          unsigned long long* mk, int n_tiers) {
  int64_t slot = dev_table_find(v, h, model);
  if (slot < 0) return 0;
  v.stamp[slot] = epoch;  // LRU touch on read (non-atomic ok)
  const uint32_t* p = v.pods + slot * v.pods_per_key;
  int any_raw = 0;
  for (int j = 0; j < v.pods_per_key; ++j) {
    uint32_t e = p[j];
    if (e == 0) continue;
    any_raw = 1;
    uint32_t pid = pod_entry_id(e);
    uint32_t tier = pod_entry_tier(e);
    if (pid >= (uint32_t)num_pods || tier >= MAX_TIERS) continue;
    if (has_filter && !((filter[pid / 64] >> (pid % 64)) & 1)) continue;
    if ((int)tier < n_tiers)  // interned => always true
      atomicOr(&mk[tier * W + pid / 64], 1ull << (pid % 64));
  }
  return any_raw ? 1 : 2;
}

// ---------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------

__global__ void k_insert(Table v, const uint64_t* __restrict__ eh,
                         const uint64_t* __restrict__ rh, int64_t n,
                         uint32_t model, const uint32_t* __restrict__ entries,
                         int n_entries, int32_t epoch, int shard_id,
                         int num_shards, int emap_write) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dev_store_block(v, eh[i], rh[i], model, entries, n_entries, epoch, shard_id,
                  num_shards, emap_write);
}

// Tombstone compaction (ROADMAP #9): thread per OLD slot rehashes live
// entries into a fresh bundle (lock-free via the usual CAS claims; old
// (key,model) pairs are unique so racers only contend on free slots).
__global__ void k_compact_main(Table ov, Table nv, int64_t cap) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  uint32_t m = ov.meta[i];
  if (!(m & META_OCC) || (m & META_TOMB)) return;
  int64_t s2 = dev_table_put(nv, ov.keys[i], m & META_MODEL_MASK,
                             ov.stamp[i]);
  uint32_t* dst = nv.pods + s2 * nv.pods_per_key;
  const uint32_t* src = ov.pods + i * ov.pods_per_key;
  for (int j = 0; j < nv.pods_per_key; ++j) dst[j] = src[j];
}

__global__ void k_compact_emap(Table ov, Table nv, int64_t cap) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  uint32_t m = ov.e_meta[i];
  if (!(m & META_OCC) || (m & META_TOMB)) return;
  dev_emap_put(nv, ov.e_keys[i], m & META_MODEL_MASK, ov.e_vals[i]);
}

__global__ void k_evict(Table v, const uint64_t* __restrict__ eh,
                        int64_t n, uint32_t model,
                        const uint32_t* __restrict__ entries, int n_entries) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dev_remove_pods(v, eh[i], model, entries, n_entries);
}

// ---- purge by pod ------------------------------------------------------
// One sweep over pods[C * P] read as the flat array it is.  A workgroup
// takes tiles of PURGE_ROWS whole table rows: PURGE_ROWS * P dwords start
// on a 1 KB boundary whatever P is, so a tile is read as 16-byte vectors,
// consecutive lanes taking consecutive vectors, and no row leaves its
// tile.  Inside the tile rows do straddle vectors and waves (P = 10: a row
// is 2.5 vectors), so the lane that holds a dword is not the lane that
// decides about its row: every lane reports what it saw of a row to that
// row's flag word in LDS (ROW_HIT: cleared an entry; ROW_LIVE: an entry
// remains), and after a barrier thread r reads row r's flags and
// tombstones the row if it was hit and nothing remains.  Nothing is read
// from global memory twice.  The tile's meta words (slot eligibility) and
// the purge bitmap (<= 512 B) sit in LDS as well: neighbouring lanes ask
// for the same or the next row (broadcast or distinct banks), and the
// bitmap test is one data-dependent ds_read_b32 for the few entries that
// are not empty.
constexpr int PURGE_THREADS = 256;
constexpr int PURGE_ROWS = 256;        // rows per tile: one per thread
constexpr int PURGE_VECS = 4;          // 16-byte loads in flight per thread
constexpr int PURGE_MAX_BLOCKS = 2048; // 8 workgroups on each of 256 CUs
constexpr uint32_t ROW_HIT = 1u, ROW_LIVE = 2u;

// One pod entry e read from *p, which lies in tile row `row`.
DEV void purge_entry(uint32_t e, uint32_t* p, int row,
                     const uint32_t* s_bits, uint32_t n_bits,
                     const uint32_t* s_meta, int model_id, uint32_t* s_flags,
                     uint32_t& n_cleared) {
  if (e == 0) return;
  const uint32_t pid = pod_entry_id(e);
  bool cleared = false;
  if (pid < n_bits && ((s_bits[pid >> 5] >> (pid & 31)) & 1) &&
      purge_slot_eligible(s_meta[row], model_id))
    // CAS, not a store: a concurrent dev_pod_set_add overwrite of this
    // slot must survive, and then the row stays live
    cleared = atomicCAS(p, e, 0u) == e;
  n_cleared += cleared ? 1u : 0u;
  atomicOr(&s_flags[row], cleared ? ROW_HIT : ROW_LIVE);
}

// bits: the purge bitmap as n_bit_words 32-bit words (pod id pid is bit
// pid % 32 of word pid / 32).  model_id -1: every model.  partials
// [gridDim.x][2]: each workgroup's {entries cleared, keys tombstoned},
// written once with plain stores - the op sums them after its one
// readback, so no counter has to be zeroed before the launch.
__global__ void __launch_bounds__(PURGE_THREADS) k_purge_pods(
    Table v, const uint32_t* __restrict__ bits, int n_bit_words, int model_id,
    int64_t n_tiles, uint32_t* __restrict__ partials) {
  __shared__ uint32_t s_bits[128];
  __shared__ uint32_t s_meta[PURGE_ROWS];
  __shared__ uint32_t s_flags[PURGE_ROWS];
  __shared__ uint32_t s_red[2 * (PURGE_THREADS / 64)];
  const int tid = threadIdx.x;
  const uint32_t P = (uint32_t)v.pods_per_key;
  const uint64_t cap = v.cap_mask + 1;
  const uint32_t n_bits = (uint32_t)n_bit_words * 32u;
  if (tid < n_bit_words) s_bits[tid] = bits[tid];
  uint32_t n_cleared = 0, n_tomb = 0;

  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = (uint64_t)tile * PURGE_ROWS;
    const uint64_t rows_left = cap - row0;
    const int rows = rows_left < PURGE_ROWS ? (int)rows_left : PURGE_ROWS;
    const uint32_t n_dw = (uint32_t)rows * P;
    const uint32_t n_vec = n_dw >> 2;
    uint32_t* tile_p = v.pods + row0 * P;
    const uint4* tile_v = reinterpret_cast<const uint4*>(tile_p);

    // the meta load goes out first and is the only one waited for before
    // the barrier; the first PURGE_VECS vector loads stay in flight
    const uint32_t m_mine = tid < rows ? v.meta[row0 + tid] : 0u;
    uint32_t base = 0;
    do {
      uint4 q[PURGE_VECS];
#pragma unroll
      for (int k = 0; k < PURGE_VECS; ++k) {
        const uint32_t vi = base + k * PURGE_THREADS + tid;
        q[k] = vi < n_vec ? tile_v[vi] : make_uint4(0, 0, 0, 0);
      }
      if (base == 0) {
        s_meta[tid] = m_mine;
        s_flags[tid] = 0;
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < PURGE_VECS; ++k) {
        const uint32_t vi = base + k * PURGE_THREADS + tid;
        if ((q[k].x | q[k].y | q[k].z | q[k].w) == 0) continue;
        const uint32_t i0 = vi * 4;
        uint32_t row = i0 / P;
        uint32_t col = i0 - row * P;
        const uint32_t e[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          purge_entry(e[j], tile_p + i0 + j, (int)row, s_bits, n_bits, s_meta,
                      model_id, s_flags, n_cleared);
          if (++col == P) { col = 0; ++row; }
        }
      }
      base += PURGE_THREADS * PURGE_VECS;
    } while (base < n_vec);
    // a tile whose dword count is no multiple of 4 (capacity 1 or 2 only)
    if ((uint32_t)tid < (n_dw & 3u)) {
      const uint32_t i = n_vec * 4 + tid;
      purge_entry(tile_p[i], tile_p + i, (int)(i / P), s_bits, n_bits, s_meta,
                  model_id, s_flags, n_cleared);
    }
    __syncthreads();
    // thread r owns row r: it wrote the row's meta and flag words and is
    // the one to rewrite them for the next tile, so no third barrier
    if (tid < rows && s_flags[tid] == ROW_HIT && !(s_meta[tid] & META_TOMB)) {
      const uint32_t old = atomicOr(&v.meta[row0 + tid], META_TOMB);
      n_tomb += (old & META_TOMB) ? 0u : 1u;
    }
  }

  // counters: wave, then workgroup, then one pair of stores
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_cleared += __shfl_down(n_cleared, off, 64);
    n_tomb += __shfl_down(n_tomb, off, 64);
  }
  if ((tid & 63) == 0) {
    s_red[2 * (tid >> 6)] = n_cleared;
    s_red[2 * (tid >> 6) + 1] = n_tomb;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t c = 0, t = 0;
    for (int w = 0; w < PURGE_THREADS / 64; ++w) {
      c += s_red[2 * w];
      t += s_red[2 * w + 1];
    }
    partials[2 * blockIdx.x] = c;
    partials[2 * blockIdx.x + 1] = t;
  }
}

// ---- remap pod ids -----------------------------------------------------
// The purge's sweep with a code table in place of the bitmap: the same
// tiles of PURGE_ROWS whole rows, the same 16-byte loads and per-row flag
// words.  The table (remap_entry's codes, 2 B per id, only the n given)
// is staged in LDS once per workgroup: 8 KB at n = 4096, 10 288 B static
// LDS in all, and the translation is one data-dependent ds_read_u16 per
// non-empty entry.  A moved entry reports ROW_LIVE, a dropped one ROW_HIT.
//
// The caller holds every other writer off (kvidx_ops.h), so entries and
// meta are written with plain stores: a 16-byte vector in which a dword
// changed goes back whole, once, by the lane that loaded it; one in which
// nothing changed, and any all-zero vector, is not written.

// One non-empty entry e of tile row `row`; returns what it becomes.
DEV uint32_t remap_one(uint32_t e, int row, const uint16_t* s_codes,
                       uint32_t n, const uint32_t* s_meta, uint32_t* s_flags,
                       uint32_t& n_moved, uint32_t& n_cleared) {
  // the map first: an entry that stays needs no look at its slot's meta
  uint32_t ne = remap_entry(e, s_codes, n);
  if (ne != e && !purge_slot_eligible(s_meta[row], -1)) ne = e;
  n_cleared += ne == 0 ? 1u : 0u;
  n_moved += (ne != 0 && ne != e) ? 1u : 0u;
  atomicOr(&s_flags[row], ne == 0 ? ROW_HIT : ROW_LIVE);
  return ne;
}

// remap: int32 [n], -1 = drop.  partials [gridDim.x][3]: each workgroup's
// {entries moved, entries cleared, keys tombstoned}, as in k_purge_pods.
__global__ void __launch_bounds__(PURGE_THREADS) k_remap_pods(
    Table v, const int32_t* __restrict__ remap, int n, int64_t n_tiles,
    uint32_t* __restrict__ partials) {
  __shared__ uint16_t s_codes[MAX_PODS];
  __shared__ uint32_t s_meta[PURGE_ROWS];
  __shared__ uint32_t s_flags[PURGE_ROWS];
  __shared__ uint32_t s_red[3 * (PURGE_THREADS / 64)];
  const int tid = threadIdx.x;
  const uint32_t P = (uint32_t)v.pods_per_key;
  const uint64_t cap = v.cap_mask + 1;
  const uint32_t un = (uint32_t)n;
  // two codes per lane and store; the first tile's barrier publishes them
  for (int i = 2 * tid; i < n; i += 2 * PURGE_THREADS) {
    const uint32_t lo = (uint32_t)(remap[i] + 1);
    const uint32_t hi = i + 1 < n ? (uint32_t)(remap[i + 1] + 1) : 0u;
    reinterpret_cast<uint32_t*>(s_codes)[i >> 1] = lo | (hi << 16);
  }
  uint32_t n_moved = 0, n_cleared = 0, n_tomb = 0;

  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = (uint64_t)tile * PURGE_ROWS;
    const uint64_t rows_left = cap - row0;
    const int rows = rows_left < PURGE_ROWS ? (int)rows_left : PURGE_ROWS;
    const uint32_t n_dw = (uint32_t)rows * P;
    const uint32_t n_vec = n_dw >> 2;
    uint32_t* tile_p = v.pods + row0 * P;
    uint4* tile_v = reinterpret_cast<uint4*>(tile_p);

    const uint32_t m_mine = tid < rows ? v.meta[row0 + tid] : 0u;
    uint32_t base = 0;
    do {
      uint4 q[PURGE_VECS];
#pragma unroll
      for (int k = 0; k < PURGE_VECS; ++k) {
        const uint32_t vi = base + k * PURGE_THREADS + tid;
        q[k] = vi < n_vec ? tile_v[vi] : make_uint4(0, 0, 0, 0);
      }
      if (base == 0) {
        s_meta[tid] = m_mine;
        s_flags[tid] = 0;
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < PURGE_VECS; ++k) {
        const uint32_t vi = base + k * PURGE_THREADS + tid;
        if ((q[k].x | q[k].y | q[k].z | q[k].w) == 0) continue;
        const uint32_t i0 = vi * 4;
        uint32_t row = i0 / P;
        uint32_t col = i0 - row * P;
        uint32_t e[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
        bool changed = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (e[j] != 0) {
            const uint32_t ne = remap_one(e[j], (int)row, s_codes, un, s_meta,
                                          s_flags, n_moved, n_cleared);
            changed |= ne != e[j];
            e[j] = ne;
          }
          if (++col == P) { col = 0; ++row; }
        }
        // vi < n_vec here: a vector past the tile was loaded as zeros
        if (changed) tile_v[vi] = make_uint4(e[0], e[1], e[2], e[3]);
      }
      base += PURGE_THREADS * PURGE_VECS;
    } while (base < n_vec);
    // a tile whose dword count is no multiple of 4 (capacity 1 or 2 only)
    if ((uint32_t)tid < (n_dw & 3u)) {
      const uint32_t i = n_vec * 4 + tid;
      const uint32_t e = tile_p[i];
      if (e != 0) {
        const uint32_t ne = remap_one(e, (int)(i / P), s_codes, un, s_meta,
                                      s_flags, n_moved, n_cleared);
        if (ne != e) tile_p[i] = ne;
      }
    }
    __syncthreads();
    // thread r owns row r, as in the purge
    if (tid < rows && s_flags[tid] == ROW_HIT && !(s_meta[tid] & META_TOMB)) {
      v.meta[row0 + tid] = s_meta[tid] | META_TOMB;
      ++n_tomb;
    }
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_moved += __shfl_down(n_moved, off, 64);
    n_cleared += __shfl_down(n_cleared, off, 64);
    n_tomb += __shfl_down(n_tomb, off, 64);
  }
  if ((tid & 63) == 0) {
    s_red[3 * (tid >> 6)] = n_moved;
    s_red[3 * (tid >> 6) + 1] = n_cleared;
    s_red[3 * (tid >> 6) + 2] = n_tomb;
  }
  __syncthreads();
  if (tid < 3) {
    uint32_t s = 0;
    for (int w = 0; w < PURGE_THREADS / 64; ++w) s += s_red[3 * w + tid];
    partials[3 * blockIdx.x + tid] = s;
  }
}

__global__ void k_get_request_keys(Table v,
                                   const uint64_t* __restrict__ eh, int64_t n,
                                   uint32_t model, uint8_t* __restrict__ found,
                                   uint64_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t ei = dev_emap_find(v, eh[i], model);
  if (ei >= 0) {
    found[i] = 1;
    out[i] = v.e_vals[ei];
  }
}

// Generic lookup producing global found[] + per-tier masks [K, T, W].
__global__ void k_lookup_masks(Table v, const uint64_t* __restrict__ rh,
                               int64_t K, uint32_t model,
                               const uint64_t* __restrict__ filter,
                               int has_filter, int num_pods, int W,
                               int32_t epoch, int shard_id, int num_shards,
                               int n_tiers,
                               uint8_t* __restrict__ found,
                               unsigned long long* __restrict__ masks) {
  int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  if (!owns_key(rh[k], shard_id, num_shards))
    return;  // unowned key: contributes zero masks on this shard
  found[k] = (uint8_t)dev_probe_collect(
      v, rh[k], model, filter, has_filter, num_pods, W, epoch,
      masks + (size_t)k * n_tiers * W, n_tiers);
}

// One (key, word) step of the longest-prefix walk, lane = pod bit.  mk is
// the key's tier-0 mask word for this 64-pod word (tier planes W apart).
// A pod stays active while every key so far lists it; an active pod earns
// the key's best tier weight.  Returns the lane's new active flag.
DEV int score_walk_step(const unsigned long long* mk, int W, int n_tiers,
                        const float* __restrict__ weights, int lane,
                        bool first, int& active, float& score) {
  int cur = 0;
  float wmax = 0.f;
  for (int t = 0; t < n_tiers; ++t) {
    if ((mk[t * W] >> lane) & 1) {
      cur = 1;
      wmax = fmaxf(wmax, weights[t]);
    }
  }
  int act = first ? cur : (active & cur);
  active = act;
  if (act) score += wmax;
  return act;
}

// Fused probe + longest-prefix score. One workgroup per prompt; dynamic
// LDS holds the per-key per-tier masks; the four waves then walk keys in
// order, a 64-pod word each, with the active pod set in registers.
//
// The body is shared by two entries that differ only in where prompt b's
// keys lie: k_fused_score takes flat hashes with offsets [B+1],
// k_fused_score_rows takes padded rows (h = hashes + b * stride, K =
// n_keys[b]) as the row-major chain kernel leaves them.
DEV void fused_score_body(
    Table v, const uint64_t* __restrict__ h, const int K,
    uint32_t model, const uint64_t* __restrict__ filter, int has_filter,
    const float* __restrict__ weights, int num_pods, int W, int32_t epoch,
    int n_tiers, float* __restrict__ scores) {
  // n_tiers = tiers actually registered (usually 1-2, <= MAX_TIERS):
  // sizing LDS by it instead of MAX_TIERS keeps 256-pod fleets (W=4)
  // at 16-32 KB/WG instead of 64 KB, preserving occupancy.
  extern __shared__ unsigned long long lds_masks[];  // [K, n_tiers, W]
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  // zero LDS
  for (int x = threadIdx.x; x < K * n_tiers * W; x += blockDim.x)
    lds_masks[x] = 0;
  __syncthreads();

  // phase 1: all probes in parallel (each is ~2 dependent HBM reads)
  for (int k = threadIdx.x; k < K; k += blockDim.x)
    dev_probe_collect(v, h[k], model, filter, has_filter, num_pods, W, epoch,
                      lds_masks + (size_t)k * n_tiers * W, n_tiers);
  __syncthreads();

  // phase 2: the walk. Words (64-pod groups) are independent prefix
  // walks, so they are distributed across the workgroup's 4 waves
  // (wave v takes words v, v+4, ...); lane l owns pod w*64+l. The
  // per-word early break is exact (a word stops when ITS active set
  // empties - the old all-words break was only an optimization).
  for (int w = wave; w < W; w += 4) {
    float score = 0.f;
    int active = 0;
    for (int k = 0; k < K; ++k) {
      const int act =
          score_walk_step(lds_masks + (size_t)k * n_tiers * W + w, W, n_tiers,
                          weights, lane, k == 0, active, score);
      if (!__any(act)) break;  // this word's active set is empty
    }
    int pid = w * 64 + lane;
    if (pid < num_pods) scores[(size_t)b * num_pods + pid] = score;
  }
}

__global__ void __launch_bounds__(256) k_fused_score(
    Table v, const uint64_t* __restrict__ hashes,
    const int32_t* __restrict__ offsets,  // [B+1]
    uint32_t model, const uint64_t* __restrict__ filter, int has_filter,
    const float* __restrict__ weights, int num_pods, int W, int32_t epoch,
    int n_tiers, float* __restrict__ scores) {
  const int b = blockIdx.x;
  fused_score_body(v, hashes + offsets[b], offsets[b + 1] - offsets[b], model,
                   filter, has_filter, weights, num_pods, W, epoch, n_tiers,
                   scores);
}

// Padded rows: prompt b's keys are hashes[b * stride .. + n_keys[b]).  The
// slots past n_keys[b] are never read (the chain kernel zeroes them, and
// remap_hash(0) is a legal key).
__global__ void __launch_bounds__(256) k_fused_score_rows(
    Table v, const uint64_t* __restrict__ hashes,  // [B, stride]
    const int32_t* __restrict__ n_keys,               // [B]
    int64_t stride, uint32_t model, const uint64_t* __restrict__ filter,
    int has_filter, const float* __restrict__ weights, int num_pods, int W,
    int32_t epoch, int n_tiers, float* __restrict__ scores) {
  const int b = blockIdx.x;
  fused_score_body(v, hashes + (int64_t)b * stride, n_keys[b], model, filter,
                   has_filter, weights, num_pods, W, epoch, n_tiers, scores);
}

// Walk precomputed masks (e.g. after an RCCL all-reduce merge of shard
// masks) -> scores.  Per-pod scoring is independent across 64-pod words
// (the all-empty break is only an optimization), so huge fleets split
// across blockIdx.y word-groups of up to 16 words each.
// Grid = (B, ceil(W/16)), one wave per block.
__global__ void __launch_bounds__(64) k_score_from_masks(
    const unsigned long long* __restrict__ masks,  // [Ktot, T, W]
    const int32_t* __restrict__ offsets,           // [B+1]
    const float* __restrict__ weights, int T, int num_pods, int W,
    float* __restrict__ scores) {
  const int b = blockIdx.x;
  const int w_lo = blockIdx.y * 16;
  const int w_hi = min(W, w_lo + 16);
  const int WG = w_hi - w_lo;
  const int K = offsets[b + 1] - offsets[b];
  const int lane = threadIdx.x & 63;
  float score[16];
  int active[16];
  for (int w = 0; w < WG; ++w) {
    score[w] = 0.f;
    active[w] = 0;
  }
  for (int k = 0; k < K; ++k) {
    const unsigned long long* mk =
        masks + (size_t)(offsets[b] + k) * T * W;
    bool any = false;
    for (int w = 0; w < WG; ++w) {
      const int act = score_walk_step(mk + w_lo + w, W, T, weights, lane,
                                      k == 0, active[w], score[w]);
      if (__any(act)) any = true;
    }
    if (!any) break;
  }
  for (int w = 0; w < WG; ++w) {
    int pid = (w_lo + w) * 64 + lane;
    if (pid < num_pods) scores[(size_t)b * num_pods + pid] = score[w];
  }
}

// Batched hash chains: one LANE per prompt (chains are serial per prompt,
// wave64-parallel across prompts; streaming CBOR->FNV keeps all state in
// registers).  ALGO is the chain-function policy (kvidx_common.h
// chain_link): 0 = fnv-64a, 1/2 = SHA-256 over the same payload.
template <int ALGO>
__global__ void k_hash_chain(const int64_t* __restrict__ tokens,
                             const int64_t* __restrict__ tok_off,  // [B+1]
                             const uint64_t* __restrict__ parents,
                             const int64_t* __restrict__ chunk_off,  // [B+1]
                             int64_t B, int block_size,
                             uint64_t* __restrict__ out) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  uint64_t h = parents[b];
  const int64_t* t0 = tokens + tok_off[b];
  int64_t n_chunks = chunk_off[b + 1] - chunk_off[b];
  uint64_t* o = out + chunk_off[b];
  for (int64_t c = 0; c < n_chunks; ++c) {
    h = chain_link<ALGO>(h, t0 + c * block_size, block_size);
    o[c] = h;
  }
}

// Transposed-layout hash chains (the read-path hot kernel): tokens are
// staged [token_pos][prompt] in int32, so at each chunk step all 64 lanes
// of a wave load one coalesced 256 B line per token position, and the
// next chunk's 16 independent loads prefetch under the current chunk's
// serial FNV ALU chain.  The row-major int64 variant (k_hash_chain)
// measured 2.5 ms per 512x512-chunk call on MI355X - pure HBM latency on
// strided per-lane loads; this layout removes that.
// out is [max_chunks][B] (transposed too; callers transpose back with a
// cheap torch op or consume the stride directly) or, row_major, [B]
// [max_chunks] as the fused-score kernel reads it.
// One chain per lane.  Several chains per lane (ILP) and an explicit
// double-buffer prefetch were both built and measured slower in every
// round: with one wave per SIMD the wave is instruction-ISSUE bound (one
// vector instruction per ~5 cycles, dependent or not), so x chains per
// lane take nearly x times the time (profiles/r01_chain_sweep.md,
// r04_fnv_chain.md, r05_score_walk.md, r07_native_refactor.md).  What
// makes a call faster is fewer instructions per chunk.
// The kernels write EVERY slot of out for their prompts, a zero where
// c >= n_chunks[b], so the caller need not clear the buffer first.
DEV int64_t chain_out_index(int row_major, int64_t b, int c, int max_chunks,
                            int64_t B) {
  return row_major ? b * max_chunks + c : (int64_t)c * B + b;
}

// SHA-256 chain (ALGO 1/2): not a re-skin of the FNV body.  FNV
// streams bytes through one 64-bit register; SHA-256 needs 16-word
// blocks and CBOR makes every byte position data-dependent per lane.
// Each lane therefore first packs its whole padded payload (1..6 blocks
// depending on BS and the token widths) into its own LDS column - layout
// [word][thread], so lanes at the same word index hit distinct banks and
// the data-dependent word index costs an LDS address, not scratch - and
// then the wave runs the fully unrolled 64-round compression together
// for the wave-maximum block count, a per-lane select discarding blocks
// a lane does not have (chunk_hash_sha256_wave).  The workgroup is
// SHA_TR_THREADS(BS) wide so the columns stay <= 48 KB per workgroup.
template <int NT>
struct ShaLdsCol {
  uint32_t* p;  // &words[0][threadIdx.x]
  DEV void st(int i, uint32_t v) { p[i * NT] = v; }
  DEV uint32_t ld(int i) const { return p[i * NT]; }
};
struct ShaWaveAny {
  DEV bool operator()(bool b) const { return __any(b); }
};
constexpr int sha_tr_threads(int bs) { return bs > 32 ? 128 : 256; }
constexpr int sha_tr_words(int bs) {
  return 16 * sha_blocks_for(sha_max_payload(bs));
}

template <int BS, int ALGO>
__global__ void k_sha_chain_tr(const int32_t* __restrict__ tokens_t,  // [T,B]
                               const uint64_t* __restrict__ parents,  // [B]
                               const int32_t* __restrict__ n_chunks,  // [B]
                               int64_t B, int max_chunks, int row_major,
                               uint64_t* __restrict__ out) {  // [maxC,B] or [B,maxC]
  constexpr int NT = sha_tr_threads(BS);
  __shared__ uint32_t sha_words[sha_tr_words(BS) * NT];
  const int64_t lane = (int64_t)blockIdx.x * NT + threadIdx.x;
  // no early return: idle lanes ride along (clamped loads, results
  // discarded) so every wave-wide vote below sees whole waves
  const bool live = lane < B;
  const int64_t bi = live ? lane : 0;
  uint64_t h = parents[bi];
  const int mc = live ? n_chunks[bi] : 0;
  ShaLdsCol<NT> col{sha_words + threadIdx.x};
  int c = 0;
  for (; c < max_chunks; ++c) {
    const bool active = c < mc;
    if (!__any(active)) break;  // wave-uniform: chains only get shorter
    uint32_t tok[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j)
      tok[j] = (uint32_t)tokens_t[(int64_t)(c * BS + j) * B + bi];
    const uint64_t h2 = chunk_hash_sha256_wave(
        h, tok, BS, sha_digest_word(ALGO), col, active, ShaWaveAny{});
    h = active ? h2 : h;
    if (live)
      out[chain_out_index(row_major, lane, c, max_chunks, B)] =
          active ? h : 0;
  }
  // the wave left early: its remaining slots are all unused
  if (live)
    for (; c < max_chunks; ++c)
      out[chain_out_index(row_major, lane, c, max_chunks, B)] = 0;
}

// Row-major staging of the FNV chain: chunks per flush, u64 per staged
// prompt row (one pad), dynamic LDS per workgroup.
constexpr int CHAIN_STAGE_CHUNKS = 16;
constexpr int CHAIN_STAGE_ROW = CHAIN_STAGE_CHUNKS + 1;
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
constexpr size_t chain_stage_bytes(int threads) {
  return (size_t)threads * CHAIN_STAGE_ROW * sizeof(uint64_t);
}

// Row-major output: a store of one chunk's hashes straight from the
// lanes is 64 separate 8-byte pieces, max_chunks * 8 bytes apart.  The
// wave parks each chunk's hashes in LDS instead and, every
// CHAIN_STAGE_CHUNKS chunks (and after the last), this writes each
// prompt's 128 bytes as eight 16-byte stores from eight neighbouring
// lanes: whole lines.
// Layout [prompt][17] u64 (16 chunks + 1 pad, 136 B rows), by the LDS
// bank model (ds_write_b64 and ds_read2_b64: bank = dword address mod
// 32, conflicts within groups of 16 consecutive lanes):
//  - write, lane p stores dwords 34p+2cc, +1: 34 = 2 mod 32, so 16
//    lanes cover all 32 banks once;
//  - read, lane l takes dwords 34(8g + l/8) + 4(l%8) + {0,1} and
//    {2,3}: per access the 8 lanes of a row hit banks 4i, 4i+1 off the
//    row's base, the group's other row is based 2 banks further on and
//    fills the gaps.
// Both are conflict-free.  One wave owns its region, and a wave's LDS
// operations execute in order, so wavefront-scope fences (no
// instructions, only compiler ordering) are all the synchronisation.
// stage: this wave's [64][CHAIN_STAGE_ROW]; lane: global lane = prompt;
// wl: lane within the wave; c: the chunk just staged.
DEV void chain_flush_rows(const uint64_t* stage, uint64_t* __restrict__ out,
                          int64_t lane, int wl, int c, int max_chunks,
                          int64_t B) {
  // flush chunks [c0, c0 + n): lane l writes chunks c0 + 2(l%8),
  // +1 of prompt 8g + l/8 of this wave, g = 0..7
  const int cc = c & (CHAIN_STAGE_CHUNKS - 1);
  const int c0 = c - cc;
  const int n = cc + 1;
  // rows start 16-byte aligned iff max_chunks is even; n is then
  // even too.  Odd max_chunks keeps 8-byte stores.
  const bool vec = (max_chunks & 1) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int part2 = 2 * (wl & 7);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const int r = g * 8 + (wl >> 3);
    const int64_t pb = lane - wl + r;  // prompt of row r
    const uint64_t* s = stage + r * CHAIN_STAGE_ROW + part2;
    const uint64_t v0 = s[0];
    const uint64_t v1 = s[1];
    if (pb < B && part2 < n) {
      uint64_t* o = out + pb * max_chunks + c0 + part2;
      if (vec) {
        *reinterpret_cast<u64x2*>(o) = u64x2{v0, v1};  // dwordx4
      } else {
        o[0] = v0;
        if (part2 + 1 < n) o[1] = v1;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int BS>
__global__ void k_fnv_chain_tr(const int32_t* __restrict__ tokens_t,  // [T,B]
                               const uint64_t* __restrict__ parents,  // [B]
                               const int32_t* __restrict__ n_chunks,  // [B]
                               int64_t B, int max_chunks, int row_major,
                               uint64_t* __restrict__ out) {  // [maxC,B] or [B,maxC]
  extern __shared__ uint64_t chain_stage[];  // [waves][64][CHAIN_STAGE_ROW]
  const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int wl = threadIdx.x & 63;
  uint64_t* stage =
      chain_stage + (size_t)(threadIdx.x >> 6) * (64 * CHAIN_STAGE_ROW);
  // no early return here either: the wide-parent vote below needs whole
  // waves, so lanes past B ride along as chains of no chunks
  const bool live = lane < B;
  const int64_t bi = live ? lane : 0;
  uint64_t h = parents[bi];
  const int mc = live ? n_chunks[bi] : 0;
  for (int c = 0; c < max_chunks; ++c) {
    // loads and the hash body are UNCONDITIONAL (clamped addresses, dead
    // chains compute garbage that a select discards)
    uint32_t tok[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j)
      tok[j] = (uint32_t)tokens_t[(int64_t)(c * BS + j) * B + bi];
    const bool active = c < mc;
    // Wave-uniform vote: every chain of the wave that still runs has a
    // parent above 0xFFFFFFFF (after chunk 0 it is a 64-bit hash), so
    // the parent item needs no selects.  A scalar branch, taken by the
    // whole wave.
    const bool wide = __all(!active || h > 0xFFFFFFFFull);
    const uint64_t h2 = chunk_hash_fast(h, tok, BS, wide);
    h = active ? h2 : h;
    // row_major writes the layout the fused-score kernel consumes,
    // which saves a 128 MB/call transpose pass downstream.  Unused
    // slots get their zero here: the caller hands in uninitialised
    // memory.
    const uint64_t val = active ? h : 0;
    const int cc = c & (CHAIN_STAGE_CHUNKS - 1);
    if (row_major)
      stage[wl * CHAIN_STAGE_ROW + cc] = val;
    else if (live)
      out[chain_out_index(row_major, lane, c, max_chunks, B)] = val;
    if (row_major && (cc == CHAIN_STAGE_CHUNKS - 1 || c == max_chunks - 1))
      chain_flush_rows(stage, out, lane, wl, c, max_chunks, B);
  }
}

// Apply a batch of KV events fully on-device: one WAVE per pod-group
// (events of one pod processed serially -> per-pod ordering preserved,
// kvevents/pool.go:132-144); within a BlockStored event lane 0 streams the
// request-key chain (token_processor.go:94-123, stitched from the parent
// engine key via the engine map like pool.go:279-296) and all 64 lanes
// fan out the per-block inserts.
template <int ALGO>
__global__ void k_apply_events(
    Table v, const int64_t* __restrict__ tokens,
    const int32_t* __restrict__ tok_off,     // [E+1]
    const uint64_t* __restrict__ ehashes,    // engine hashes, flat
    const int32_t* __restrict__ eh_off,      // [E+1]
    const uint64_t* __restrict__ parents,    // [E]
    const uint8_t* __restrict__ has_parent,  // [E]
    const uint8_t* __restrict__ ev_type,     // [E] 0=stored 1=removed
    const uint32_t* __restrict__ pod_entry,  // [E]
    const int32_t* __restrict__ grp_off,     // [G+1] event groups by pod
    const int32_t* __restrict__ model_of,    // [E] model id per event
    int64_t G, uint64_t init_hash, int block_size,
    int32_t epoch, int shard_id, int num_shards,
    uint64_t* __restrict__ req_scratch) {    // [total engine hashes]
  const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= G) return;
  const int e_begin = grp_off[g];
  const int e_end = grp_off[g + 1];

  for (int e = e_begin; e < e_end; ++e) {
    const int nh = eh_off[e + 1] - eh_off[e];
    const uint64_t* eh = ehashes + eh_off[e];
    const uint32_t model = (uint32_t)model_of[e];
    if (ev_type[e] == 1) {  // BlockRemoved
      for (int i = lane; i < nh; i += 64)
        dev_remove_pods(v, eh[i], model, &pod_entry[e], 1);
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    // BlockStored: lane 0 resolves parent + streams the request chain.
    // (The mismatch drop is uniform per wave: scalar per event.)
    const int n_chunks = event_chain_len(tok_off, eh_off, e, block_size);
    if (n_chunks < 0) continue;
    uint64_t* req = req_scratch + eh_off[e];
    if (lane == 0) {
      const int64_t* t0 = tokens + tok_off[e];
      uint64_t h =
          dev_event_parent(v, has_parent, parents, model_of, e, init_hash);
      for (int c = 0; c < n_chunks; ++c) {
        h = chain_link<ALGO>(h, t0 + (int64_t)c * block_size, block_size);
        req[c] = h;
      }
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < n_chunks; i += 64)
      dev_store_block(v, eh[i], req[i], model, &pod_entry[e], 1, epoch,
                      shard_id, num_shards, 1);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------------
// Phase-split event application (the serial wave-per-group kernel above
// left 63 lanes idle during each chain; here chains run one LANE per
// pod-group and the per-block inserts fan out thread-per-block).
// The host guards ordering: a batch where some engine hash is both
// stored and removed falls back to the serial kernel.
// ---------------------------------------------------------------------

// Batch map: (group, engine hash) -> global block index, for the blocks
// of the burst's KEPT BlockStored events only (open addressing, zeroed
// tensors per call; value = idx+1).  Removed blocks and the blocks of an
// event that event_chain_len drops never get a request key, so they are
// not in it: a parent that names one resolves through the persistent
// engine map like any other.  The group is part of the key word, so the
// 128 pods of a fleet that store one hash in one burst take 128 scattered
// slots, not one probe window.  Every block claims a slot of its own (no
// deduplication); two key words may also collide, so a finder checks the
// block an entry points to.  A block that finds no slot in its window is
// left out, and a parent naming it resolves through the engine map.
DEV uint64_t bmap_key(uint64_t h, int g) {
  // odd multiplier: for one hash, distinct groups give distinct words
  return remap_hash(h ^ ((uint64_t)(g + 1) * 0xD6E8FEB86659FD93ull));
}

// Group of event e: the g with grp_off[g] <= e < grp_off[g + 1].
DEV int dev_group_of_event(const int32_t* __restrict__ grp_off, int G, int e) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (grp_off[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void k_batch_bmap(const uint64_t* __restrict__ ehashes,
                             const int32_t* __restrict__ eh_off,
                             const int32_t* __restrict__ ev_of,
                             const uint8_t* __restrict__ ev_type,
                             const int32_t* __restrict__ tok_off,
                             const int32_t* __restrict__ grp_off, int G,
                             int block_size, int64_t n,
                             uint64_t* __restrict__ bkeys,
                             int32_t* __restrict__ bvals, int64_t bmask) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int e = ev_of[i];
  if (ev_type[e] == 1) return;  // BlockRemoved
  if (event_chain_len(tok_off, eh_off, e, block_size) < 0) return;
  const uint64_t key = bmap_key(ehashes[i], dev_group_of_event(grp_off, G, e));
  uint64_t s = probe_start(key, (uint64_t)bmask);
  for (int t = 0; t < PROBE_MAX; ++t) {
    uint64_t j = (s + t) & (uint64_t)bmask;
    uint64_t prev = atomicCAS((unsigned long long*)&bkeys[j], 0ull,
                              (unsigned long long)key);
    if (prev == 0) {
      bvals[j] = (int32_t)(i + 1);  // consumers run in a later kernel
      return;
    }
  }
}

// Latest block in [lo, hi) that group g's kept stores gave engine hash h,
// or -1.  [lo, hi) lies inside g's blocks: from its first block up to the
// asking event's own.
DEV int64_t dev_bmap_find(const uint64_t* __restrict__ bkeys,
                          const int32_t* __restrict__ bvals, int64_t bmask,
                          const uint64_t* __restrict__ ehashes, uint64_t h,
                          int g, int64_t lo, int64_t hi) {
  const uint64_t key = bmap_key(h, g);
  uint64_t s = probe_start(key, (uint64_t)bmask);
  int64_t best = -1;
  for (int t = 0; t < PROBE_MAX; ++t) {
    uint64_t j = (s + t) & (uint64_t)bmask;
    uint64_t k = bkeys[j];
    if (k == 0) break;
    if (k != key) continue;
    const int64_t bi = (int64_t)bvals[j] - 1;
    if (bi >= lo && bi < hi && bi > best && ehashes[bi] == h) best = bi;
  }
  return best;
}

// Phase A: one lane per pod-group walks its events in order computing
// request-key chains into req_scratch.  Parent resolution: the latest
// earlier block of the SAME group in this batch that a kept store gave
// the parent hash (bmap) first, then the persistent engine map
// (cross-batch), else the chain root.  What ANOTHER group of the batch
// stores is never a parent here: groups run concurrently.
template <int ALGO>
__global__ void k_event_chains(
    Table v, const int64_t* __restrict__ tokens,
    const int32_t* __restrict__ tok_off, const uint64_t* __restrict__ ehashes,
    const int32_t* __restrict__ eh_off, const uint64_t* __restrict__ parents,
    const uint8_t* __restrict__ has_parent, const uint8_t* __restrict__ ev_type,
    const int32_t* __restrict__ grp_off, const int32_t* __restrict__ model_of,
    int64_t G, uint64_t init_hash, int block_size,
    const uint64_t* __restrict__ bkeys, const int32_t* __restrict__ bvals,
    int64_t bmask, uint64_t* __restrict__ req_scratch) {
  int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int e_begin = grp_off[g];
  const int e_end = grp_off[g + 1];
  KVIDX_ASSERT(e_begin >= 0 && e_begin <= e_end);
  const int grp_first_block = eh_off[e_begin];
  for (int e = e_begin; e < e_end; ++e) {
    if (ev_type[e] == 1) continue;  // removals have no chain
    const int n_chunks = event_chain_len(tok_off, eh_off, e, block_size);
    if (n_chunks < 0) continue;
    const int64_t bi =
        has_parent[e] ? dev_bmap_find(bkeys, bvals, bmask, ehashes, parents[e],
                                      (int)g, grp_first_block, eh_off[e])
                      : -1;
    const int64_t* t0 = tokens + tok_off[e];
    uint64_t h = bi >= 0 ? req_scratch[bi]  // earlier event of this group
                         : dev_event_parent(v, has_parent, parents, model_of,
                                            e, init_hash);
    for (int c = 0; c < n_chunks; ++c) {
      h = chain_link<ALGO>(h, t0 + (int64_t)c * block_size, block_size);
      req_scratch[eh_off[e] + c] = h;
    }
  }
}

// Phase A variant for batches with NO batch-local parent references
// (the host checks parents against the batch's engine hashes): chains
// are then independent across EVENTS, not just pod groups, so one LANE
// per event runs them - 8x the parallelism of lane-per-group at the
// bench shape - and the tokens are staged TRANSPOSED [token_pos][event]
// in int32 like the read path's chain kernel, so each position is one
// coalesced 256 B line across the wave instead of 64 scattered 8 B
// reads (ROADMAP round-1 #2 follow-up; write path was 9.9M blocks/s
// with the serial chain phase dominating).
// Device-side staging for k_event_chains_ev: flat per-event int32
// tokens -> transposed [token_pos][event].  Host-side transpose of the
// ragged batch measured ~2-5 ms/batch in numpy (it briefly halved
// ingest); here it is one trivial bandwidth-bound kernel over ~2 MB.
__global__ void k_transpose_ev_tokens(const int32_t* __restrict__ flat,
                                      const int32_t* __restrict__ tok_off,
                                      int64_t E,
                                      int32_t* __restrict__ out) {  // [maxT,E]
  const int e = blockIdx.x;
  const int len = tok_off[e + 1] - tok_off[e];
  for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < len;
       i += gridDim.y * blockDim.x)
    out[(int64_t)i * E + e] = flat[tok_off[e] + i];
}

// Read-path staging for the chain kernels: flat ragged tokens (int64 or
// int32, narrowed to their low 32 bits as hash_chain_batch does) ->
// transposed int32 image [T = max_chunks * block_size][B].  A read batch
// is ~128 MB of image (4096 prompts x 8192 tokens), so unlike the event
// transpose above it goes through LDS: a workgroup moves one tile of 64
// prompts x 64 positions, reading 64 consecutive positions of a prompt
// per wave (one contiguous 512 B / 256 B piece) and writing one position
// of 64 consecutive prompts per wave (one 256 B line).
// LDS int32 [64][65].  ds_write_b32 / ds_read_b32: bank = dword address
// mod 32, conflicts within a 32-lane half.  The write of row r puts lane
// l at dword 65 r + l: consecutive.  The read of column r takes lane l
// from dword 65 l + r, and 65 = 1 mod 32: a half covers the 32 banks
// once.  Both are conflict-free.
// Every slot of the image is written, a zero at and past a prompt's last
// whole chunk and in the positions of short prompts, so the caller hands
// in uninitialised memory (the chain kernels load all T rows for every
// lane).  Grid = (ceil(T / 64), ceil(B / 64)).
constexpr int STAGE_TILE = 64;
template <typename TokT>
__global__ void __launch_bounds__(256) k_stage_ragged_tokens(
    const TokT* __restrict__ flat,          // [total]
    const int32_t* __restrict__ tok_off,    // [B+1]
    const int32_t* __restrict__ n_chunks,   // [B]
    int64_t B, int64_t T, int block_size,
    int32_t* __restrict__ out) {            // [T, B]
  __shared__ int32_t tile[STAGE_TILE][STAGE_TILE + 1];
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar, so that what depends on the prompt alone
  // (its offset and length) is loaded and computed once per wave
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t t0 = (int64_t)blockIdx.x * STAGE_TILE;
  const int64_t p0 = (int64_t)blockIdx.y * STAGE_TILE;
  constexpr int ROWS = STAGE_TILE / 4;  // tile rows per wave
  const int64_t pos = t0 + lane;
  // Unconditional loads from clamped addresses (token 0 exists: T > 0),
  // then selects: no branch, so the 16 loads of a lane are all in flight
  // before the first LDS write waits for its own.
  int32_t x[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = wave + 4 * i;
    const int64_t b = min(p0 + r, B - 1);
    const int64_t keep = (int64_t)n_chunks[b] * block_size;
    const int64_t first = tok_off[b];
    const bool ok = p0 + r < B && pos < keep;
    const int32_t v = (int32_t)flat[ok ? first + pos : 0];
    x[i] = ok ? v : 0;
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) tile[wave + 4 * i][lane] = x[i];
  __syncthreads();
  const int64_t b = p0 + lane;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = wave + 4 * i;
    if (t0 + r < T && b < B) out[(t0 + r) * B + b] = tile[lane][r];
  }
}

template <int ALGO>
__global__ void k_event_chains_ev(
    Table v, const int32_t* __restrict__ tokens_t,  // [maxT, E]
    const int32_t* __restrict__ tok_off, const uint64_t* __restrict__ ehashes,
    const int32_t* __restrict__ eh_off, const uint64_t* __restrict__ parents,
    const uint8_t* __restrict__ has_parent, const uint8_t* __restrict__ ev_type,
    const int32_t* __restrict__ model_of, int64_t E, uint64_t init_hash,
    int block_size, uint64_t* __restrict__ req_scratch) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  if (ev_type[e] == 1) return;  // removals have no chain
  const int n_chunks = event_chain_len(tok_off, eh_off, e, block_size);
  if (n_chunks < 0) return;
  uint64_t h = dev_event_parent(v, has_parent, parents, model_of, e, init_hash);
  uint32_t tok[64];  // block_size <= 64
  for (int c = 0; c < n_chunks; ++c) {
    for (int j = 0; j < block_size; ++j)
      tok[j] = (uint32_t)tokens_t[(int64_t)(c * block_size + j) * E + e];
    h = chain_link<ALGO>(h, tok, block_size);
    req_scratch[eh_off[e] + c] = h;
  }
}

// Phase B: one thread per block applies its insert/removal.
__global__ void k_event_inserts(
    Table v, const uint64_t* __restrict__ ehashes,
    const int32_t* __restrict__ eh_off, const int32_t* __restrict__ ev_of,
    const uint8_t* __restrict__ ev_type, const int32_t* __restrict__ tok_off,
    const uint32_t* __restrict__ pod_entry,
    const int32_t* __restrict__ model_of, int64_t n_blocks,
    int block_size, int32_t epoch, int shard_id, int num_shards,
    const uint64_t* __restrict__ req_scratch) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_blocks) return;
  const int e = ev_of[i];
  const uint32_t model = (uint32_t)model_of[e];
  if (ev_type[e] == 1) {  // BlockRemoved
    dev_remove_pods(v, ehashes[i], model, &pod_entry[e], 1);
    return;
  }
  // BlockStored: block i is one of the event's eh_off[e + 1] - eh_off[e]
  // engine hashes, which a kept event has one chunk each for
  if (event_chain_len(tok_off, eh_off, e, block_size) < 0) return;
  dev_store_block(v, ehashes[i], req_scratch[i], model, &pod_entry[e], 1,
                  epoch, shard_id, num_shards, 1);
}

// ---------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------

#define STREAM at::cuda::getCurrentCUDAStream().stream()

// kernel<<<ceil(n / 256), 256>>>(args...) on the current stream: the
// shape of every thread-per-item kernel here.
template <typename Kern, typename... Args>
static void launch_1d(Kern kernel, int64_t n, Args... args) {
  constexpr int threads = 256;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + threads - 1) / threads)),
                     dim3(threads), 0, STREAM, args...);
}

static const uint64_t* filter_ptr(const at::Tensor& filter_words) {
  return filter_words.numel() > 0 ? u64p(filter_words) : nullptr;
}

// The fused-score kernels hold a prompt's masks in LDS: up to 16 pod
// words, 64 KB.  gpu_score_hashes and gpu_score_flat_tokens ask
// fused_score_fits to choose their route; the launcher refuses what does
// not fit.
static size_t fused_score_lds_bytes(int64_t max_k, int64_t n_tiers,
                                    int64_t W) {
  return (size_t)max_k * n_tiers * W * sizeof(uint64_t);
}
static bool fused_score_fits(int64_t max_k, int64_t n_tiers, int64_t W) {
  return W <= 16 && fused_score_lds_bytes(max_k, n_tiers, W) <= 64 * 1024;
}

// One workgroup per prompt.  where...: the kernel arguments between the
// hashes and the model id, which say where prompt b's keys lie.
template <typename Kern, typename... Where>
static at::Tensor launch_fused_score(Kern kernel, const Table& v, int64_t B,
                                     const at::Tensor& hashes,
                                     int64_t model_id,
                                     const at::Tensor& filter_words,
                                     const at::Tensor& weights,
                                     int64_t num_pods, int64_t epoch,
                                     int64_t max_k, int64_t n_tiers,
                                     Where... where) {
  int64_t W = pod_words(num_pods);
  TORCH_CHECK(W <= 16, "fused score supports up to 1024 pods");
  n_tiers = clamp_tiers(n_tiers);
  TORCH_CHECK(fused_score_fits(max_k, n_tiers, W),
              "fused score LDS overflow: reduce keys per prompt or pods");
  auto scores = at::zeros({B, num_pods}, hashes.options().dtype(at::kFloat));
  if (B == 0) return scores;
  const uint64_t* filter = filter_ptr(filter_words);
  hipLaunchKernelGGL(kernel, dim3((int)B), dim3(256),
                     fused_score_lds_bytes(max_k, n_tiers, W), STREAM, v,
                     (const uint64_t*)u64p(hashes), where...,
                     (uint32_t)model_id, filter, filter ? 1 : 0,
                     weights.data_ptr<float>(), (int)num_pods, (int)W,
                     (int32_t)epoch, (int)n_tiers, scores.data_ptr<float>());
  return scores;
}

// Runs f(std::integral_constant<int, BS>) for a block size the transposed
// chain kernels are built for.
template <typename F>
static void dispatch_chain_block_size(int64_t block_size, F&& f) {
  switch (block_size) {
    case 4:  f(std::integral_constant<int, 4>{});  break;
    case 8:  f(std::integral_constant<int, 8>{});  break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    default:
      TORCH_CHECK(false, "hash_chain_tr supports block sizes 4/8/16/32/64; "
                         "use gpu_hash_chain for other sizes");
  }
}

// Host half of the ragged staging: what the offsets say about a batch.
// One int32 buffer [n_chunks (B) | token offsets (B+1)] so that both go
// up in one copy.
struct RaggedPlan {
  int64_t B = 0, max_k = 0, total_chunks = 0;
  at::Tensor host;  // int32 [2B+1]
};

static RaggedPlan plan_ragged(const at::Tensor& tokens,
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

// -> {tokens_t int32 [max_k * block_size, B], n_chunks int32 [B]} on dev.
// Host tokens go up once, unconverted; device tokens are read in place.
static std::vector<at::Tensor> stage_ragged(const RaggedPlan& p,
                                            at::Tensor tokens,
                                            int64_t block_size,
                                            at::Device dev) {
  auto up = p.host.to(dev);
  auto n_chunks = up.slice(0, 0, p.B);
  auto tok_off = up.slice(0, p.B, 2 * p.B + 1);
  int64_t T = p.max_k * block_size;
  auto out = at::empty({T, p.B}, up.options());
  if (p.B == 0 || T == 0) return {out, n_chunks};
  auto tok = tokens.is_cuda() ? tokens.contiguous()
                              : tokens.contiguous().to(dev);
  int64_t pt = (p.B + STAGE_TILE - 1) / STAGE_TILE;
  TORCH_CHECK(pt <= 65535, "too many prompts in one batch");
  dim3 grid((unsigned)((T + STAGE_TILE - 1) / STAGE_TILE), (unsigned)pt);
  auto launch = [&](auto* flat) {
    using TokT = std::remove_const_t<std::remove_pointer_t<decltype(flat)>>;
    hipLaunchKernelGGL(k_stage_ragged_tokens<TokT>, grid, dim3(256), 0, STREAM,
                       flat, i32p(tok_off), i32p(n_chunks), p.B, T,
                       (int)block_size, i32p(out));
  };
  if (tok.dtype() == at::kLong)
    launch(tok.data_ptr<int64_t>());
  else
    launch(tok.data_ptr<int32_t>());
  return {out, n_chunks};
}

// Phase B of both split routes: one thread per block.
static void launch_event_inserts(const Table& v, const at::Tensor& ehashes,
                                 const at::Tensor& eh_off,
                                 const at::Tensor& ev_of,
                                 const at::Tensor& ev_type,
                                 const at::Tensor& tok_off,
                                 const at::Tensor& pod_entry,
                                 const at::Tensor& model_of,
                                 int64_t block_size, int64_t epoch,
                                 int64_t shard_id, int64_t num_shards,
                                 const at::Tensor& req_scratch) {
  int64_t n = ehashes.numel();
  launch_1d(k_event_inserts, n, v, u64p(ehashes), i32p(eh_off), i32p(ev_of),
            u8p(ev_type), i32p(tok_off), u32p(pod_entry), i32p(model_of), n,
            (int)block_size, (int32_t)epoch, (int)shard_id, (int)num_shards,
            u64p(req_scratch));
}

}  // namespace kvidx

// ---------------------------------------------------------------------
// Ops: the definitions of what kvidx_ops.h declares.  The names are
// qualified, so a signature that drifts from its declaration does not
// compile (it would otherwise be a new overload, and the bound one an
// undefined symbol at import).
// ---------------------------------------------------------------------

void kvidx::gpu_insert(KVIDX_TABLE_PARAMS, at::Tensor engine_hashes,
                       at::Tensor request_hashes, int64_t model_id,
                       at::Tensor pod_entries, int64_t epoch, int64_t shard_id,
                       int64_t num_shards, int64_t emap_write) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  int64_t n = engine_hashes.numel();
  if (n == 0) return;
  launch_1d(k_insert, n, v, u64p(engine_hashes), u64p(request_hashes), n,
            (uint32_t)model_id, u32p(pod_entries), (int)pod_entries.numel(),
            (int32_t)epoch, (int)shard_id, (int)num_shards, (int)emap_write);
}

void kvidx::gpu_compact(KVIDX_TABLE_PARAMS, at::Tensor n_keys,
                        at::Tensor n_meta, at::Tensor n_stamp,
                        at::Tensor n_pods, at::Tensor n_e_keys,
                        at::Tensor n_e_meta, at::Tensor n_e_vals) {
  auto ov = make_table_view(KVIDX_TABLE_ARGS, true);
  auto nv = make_table_view(n_keys, n_meta, n_stamp, n_pods, n_e_keys,
                            n_e_meta, n_e_vals, pods_per_key, true);
  int64_t cap = keys.numel();
  launch_1d(k_compact_main, cap, ov, nv, cap);
  launch_1d(k_compact_emap, cap, ov, nv, cap);
}

void kvidx::gpu_evict(KVIDX_TABLE_PARAMS, at::Tensor engine_hashes,
                      int64_t model_id, at::Tensor pod_entries) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  int64_t n = engine_hashes.numel();
  if (n == 0) return;
  launch_1d(k_evict, n, v, u64p(engine_hashes), n, (uint32_t)model_id,
            u32p(pod_entries), (int)pod_entries.numel());
}

// One launch on the current stream, no fill before it; the only host wait
// is the readback of the per-workgroup counters.
std::vector<int64_t> kvidx::gpu_purge_pods(KVIDX_TABLE_PARAMS,
                                           at::Tensor purge_words,
                                           int64_t model_id) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  const int W = purge_words_checked(purge_words, model_id);
  TORCH_CHECK(purge_words.device() == keys.device(),
              "purge_words must live on the table's device");
  TORCH_CHECK(pods_per_key >= 1 && pods_per_key <= 4096,
              "pods_per_key out of range");
  TORCH_CHECK(pods.numel() == keys.numel() * pods_per_key,
              "pods must hold capacity * pods_per_key entries");
  // tiles are read as 16-byte vectors from the start of the array
  TORCH_CHECK(reinterpret_cast<uintptr_t>(v.pods) % 16 == 0,
              "pods storage must be 16-byte aligned");
  const int64_t cap = keys.numel();
  const int64_t n_tiles = (cap + PURGE_ROWS - 1) / PURGE_ROWS;
  const int64_t grid = std::min<int64_t>(n_tiles, PURGE_MAX_BLOCKS);
  auto partials = at::empty({grid, 2}, keys.options().dtype(at::kInt));
  hipLaunchKernelGGL(k_purge_pods, dim3((unsigned)grid), dim3(PURGE_THREADS),
                     0, STREAM, v,
                     reinterpret_cast<const uint32_t*>(u64p(purge_words)),
                     2 * W, (int)model_id, n_tiles, u32p(partials));
  auto host = partials.cpu();  // waits for the sweep
  const uint32_t* hp = u32p(host);
  int64_t entries = 0, tombs = 0;
  for (int64_t b = 0; b < grid; ++b) {
    entries += hp[2 * b];
    tombs += hp[2 * b + 1];
  }
  return {entries, tombs};
}

// The purge's launch shape; the map is validated on the host first (one
// small readback of remap), the counters come back after the sweep.
std::vector<int64_t> kvidx::gpu_remap_pods(KVIDX_TABLE_PARAMS,
                                           at::Tensor remap) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  TORCH_CHECK(remap.device() == keys.device(),
              "remap must live on the table's device");
  const int n = remap_checked(remap);
  TORCH_CHECK(pods_per_key >= 1 && pods_per_key <= 4096,
              "pods_per_key out of range");
  TORCH_CHECK(pods.numel() == keys.numel() * pods_per_key,
              "pods must hold capacity * pods_per_key entries");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(v.pods) % 16 == 0,
              "pods storage must be 16-byte aligned");
  const int64_t cap = keys.numel();
  const int64_t n_tiles = (cap + PURGE_ROWS - 1) / PURGE_ROWS;
  const int64_t grid = std::min<int64_t>(n_tiles, PURGE_MAX_BLOCKS);
  auto partials = at::empty({grid, 3}, keys.options().dtype(at::kInt));
  hipLaunchKernelGGL(k_remap_pods, dim3((unsigned)grid), dim3(PURGE_THREADS),
                     0, STREAM, v, i32p(remap), n, n_tiles, u32p(partials));
  auto host = partials.cpu();  // waits for the sweep
  const uint32_t* hp = u32p(host);
  int64_t moved = 0, cleared = 0, tombs = 0;
  for (int64_t b = 0; b < grid; ++b) {
    moved += hp[3 * b];
    cleared += hp[3 * b + 1];
    tombs += hp[3 * b + 2];
  }
  return {moved, cleared, tombs};
}

std::vector<at::Tensor> kvidx::gpu_get_request_keys(
    KVIDX_TABLE_PARAMS, at::Tensor engine_hashes, int64_t model_id) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  int64_t n = engine_hashes.numel();
  auto found = at::zeros({n}, engine_hashes.options().dtype(at::kByte));
  auto out = at::zeros({n}, engine_hashes.options());
  if (n == 0) return {found, out};
  launch_1d(k_get_request_keys, n, v, u64p(engine_hashes), n,
            (uint32_t)model_id, u8p(found), u64p(out));
  return {found, out};
}

std::vector<at::Tensor> kvidx::gpu_lookup(KVIDX_TABLE_PARAMS,
                                          at::Tensor request_hashes,
                                          int64_t model_id,
                                          at::Tensor filter_words,
                                          int64_t num_pods, int64_t epoch,
                                          int64_t shard_id, int64_t num_shards,
                                          int64_t n_tiers) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  int64_t K = request_hashes.numel();
  int64_t W = pod_words(num_pods);
  n_tiers = clamp_tiers(n_tiers);
  auto found = at::zeros({K}, request_hashes.options().dtype(at::kByte));
  // tier planes sized by the registered tier count (see cpu_lookup)
  auto masks = at::zeros({K, n_tiers, W}, request_hashes.options());
  if (K == 0) return {found, masks};
  const uint64_t* filter = filter_ptr(filter_words);
  launch_1d(k_lookup_masks, K, v, u64p(request_hashes), K, (uint32_t)model_id,
            filter, filter ? 1 : 0, (int)num_pods, (int)W, (int32_t)epoch,
            (int)shard_id, (int)num_shards, (int)n_tiers, u8p(found),
            reinterpret_cast<unsigned long long*>(u64p(masks)));
  return {found, masks};
}

at::Tensor kvidx::gpu_fused_score(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                  at::Tensor offsets, int64_t model_id,
                                  at::Tensor filter_words, at::Tensor weights,
                                  int64_t num_pods, int64_t epoch,
                                  int64_t max_k, int64_t n_tiers) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  return launch_fused_score(k_fused_score, v, offsets.numel() - 1, hashes,
                            model_id, filter_words, weights, num_pods, epoch,
                            max_k, n_tiers, (const int32_t*)i32p(offsets));
}

// gpu_fused_score over the padded rows that gpu_hash_chain_tr(row_major=1)
// returns: hashes int64 [B, stride], n_keys int32 [B] on the device.
at::Tensor kvidx::gpu_fused_score_rows(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                       at::Tensor n_keys, int64_t model_id,
                                       at::Tensor filter_words,
                                       at::Tensor weights, int64_t num_pods,
                                       int64_t epoch, int64_t max_k,
                                       int64_t n_tiers) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  TORCH_CHECK(hashes.is_cuda() && hashes.dtype() == at::kLong &&
                  hashes.dim() == 2 && hashes.is_contiguous(),
              "hashes must be a contiguous int64 [B, stride] device tensor");
  TORCH_CHECK(n_keys.is_cuda() && n_keys.dtype() == at::kInt &&
                  n_keys.is_contiguous(),
              "n_keys must be a contiguous int32 device tensor");
  int64_t B = hashes.size(0);
  int64_t stride = hashes.size(1);
  TORCH_CHECK(n_keys.numel() == B, "n_keys must have one entry per row");
  TORCH_CHECK(max_k <= stride, "max_k exceeds the row length");
  return launch_fused_score(k_fused_score_rows, v, B, hashes, model_id,
                            filter_words, weights, num_pods, epoch, max_k,
                            n_tiers, (const int32_t*)i32p(n_keys), stride);
}

at::Tensor kvidx::gpu_score_from_masks(at::Tensor masks, at::Tensor offsets,
                                       at::Tensor weights, int64_t num_pods) {
  int64_t B = offsets.numel() - 1;
  int64_t W = pod_words(num_pods);
  TORCH_CHECK(W <= 64, "score_from_masks supports up to 4096 pods");
  TORCH_CHECK(masks.dim() == 3, "masks must be [Ktot, T, W]");
  int64_t T = masks.size(1);  // tier planes, sized by the lookup
  auto scores = at::zeros({B, num_pods}, masks.options().dtype(at::kFloat));
  if (B == 0) return scores;
  int wgroups = (int)((W + 15) / 16);
  hipLaunchKernelGGL(
      k_score_from_masks, dim3((int)B, wgroups), dim3(64), 0, STREAM,
      reinterpret_cast<const unsigned long long*>(u64p(masks)),
      i32p(offsets), weights.data_ptr<float>(), (int)T, (int)num_pods, (int)W,
      scores.data_ptr<float>());
  return scores;
}

at::Tensor kvidx::gpu_score_hashes(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                   at::Tensor offsets, int64_t model_id,
                                   at::Tensor filter_words, at::Tensor weights,
                                   int64_t num_pods, int64_t epoch,
                                   int64_t max_k, int64_t n_tiers) {
  if (fused_score_fits(max_k, clamp_tiers(n_tiers), pod_words(num_pods)))
    return gpu_fused_score(KVIDX_TABLE_ARGS, hashes, offsets, model_id,
                           filter_words, weights, num_pods, epoch, max_k,
                           n_tiers);
  // The masks do not fit in LDS (huge fleet, or long prompts on a large
  // one; rare): masks in global memory, then the mask walk.
  auto fm = gpu_lookup(KVIDX_TABLE_ARGS, hashes, model_id, filter_words,
                       num_pods, epoch, 0, 1, n_tiers);
  return gpu_score_from_masks(fm[1].contiguous(), offsets, weights, num_pods);
}

std::vector<at::Tensor> kvidx::gpu_hash_chain(
    at::Tensor tokens, at::Tensor tok_off, at::Tensor parents,
    int64_t block_size, int64_t algo) {
  TORCH_CHECK(tokens.is_cuda());
  TORCH_CHECK(algo_valid(algo), "unknown chain hash algo id ", algo);
  int64_t B = parents.numel();
  auto chunk_off_cpu = at::zeros({B + 1}, at::kLong);
  {
    auto off_cpu = tok_off.to(at::kCPU);
    const int64_t* offp = off_cpu.data_ptr<int64_t>();
    int64_t* cop = chunk_off_cpu.data_ptr<int64_t>();
    for (int64_t b = 0; b < B; ++b)
      cop[b + 1] = cop[b] + (offp[b + 1] - offp[b]) / block_size;
  }
  auto chunk_off = chunk_off_cpu.to(tokens.device());
  int64_t total = chunk_off_cpu.data_ptr<int64_t>()[B];
  auto out = at::empty({total}, tokens.options());
  if (B == 0) return {out, chunk_off};
  dispatch_algo(algo, [&](auto A) {
    launch_1d(k_hash_chain<decltype(A)::value>, B, tokens.data_ptr<int64_t>(),
              tok_off.data_ptr<int64_t>(), u64p(parents),
              chunk_off.data_ptr<int64_t>(), B, (int)block_size, u64p(out));
  });
  return {out, chunk_off};
}

// tokens_t: int32 [T, B] (transposed); parents int64 [B]; n_chunks
// int32 [B].  Returns out int64 [max_chunks, B] (transposed hashes), or
// [B, max_chunks] with row_major.  ilp is a retired tuning knob (0 or 1).
at::Tensor kvidx::gpu_hash_chain_tr(at::Tensor tokens_t, at::Tensor parents,
                                    at::Tensor n_chunks, int64_t block_size,
                                    int64_t max_chunks, int64_t ilp,
                                    int64_t row_major, int64_t algo) {
  TORCH_CHECK(tokens_t.is_cuda() && tokens_t.dtype() == at::kInt);
  TORCH_CHECK(algo_valid(algo), "unknown chain hash algo id ", algo);
  TORCH_CHECK(ilp == 0 || ilp == 1,
              "gpu_hash_chain_tr runs one chain per lane: ilp must be 0 or 1 "
              "(the multi-chain and prefetch variants are gone), got ", ilp);
  TORCH_CHECK(tokens_t.dim() == 2, "tokens_t must be [T, B]");
  int64_t B = tokens_t.size(1);
  TORCH_CHECK(parents.numel() == B && n_chunks.numel() == B);
  // row_major=1: out is [B, max_chunks] (what the fused-score kernel
  // consumes directly - no transpose pass); default [max_chunks, B].
  // Not cleared: the kernels write every slot, a zero where
  // c >= n_chunks[b].  Keep it so.  A fill kernel in front of the chain
  // call costs only tens of µs, but with two kernels per call on the
  // read path's side stream the runtime keeps falling back to running
  // that stream and the score stream one after the other (call time
  // 1.2 -> 2.7 ms, flipping between and within processes; measured
  // with only this line changed, profiles/r04_fnv_chain.md).
  auto out = at::empty(row_major ? std::initializer_list<int64_t>{B, max_chunks}
                                 : std::initializer_list<int64_t>{max_chunks, B},
                       parents.options());
  if (B == 0 || max_chunks == 0) return out;
  TORCH_CHECK(tokens_t.size(0) >= max_chunks * block_size,
              "tokens_t has fewer rows than max_chunks * block_size");
  auto tokens_c = tokens_t.contiguous();
  auto launch = [&](auto kern, int threads, size_t lds) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((B + threads - 1) / threads)),
                       dim3(threads), lds, STREAM, i32p(tokens_c),
                       u64p(parents), i32p(n_chunks), B, (int)max_chunks,
                       (int)row_major, u64p(out));
  };
  // One prompt per lane either way.  SHA-256: workgroup width set by the
  // LDS payload columns.  FNV: one-wave workgroups, with row-major output
  // staged in LDS.  B / 64 waves spread over all CUs before any CU
  // gets a second one, where 256-thread workgroups put four waves on
  // each of a quarter as many CUs.  Measured (profiles/r04_fnv_chain.md):
  // alone, the row-major call is 8 % shorter and the transposed one the
  // same; beside the score kernel the chain gains what the score kernel
  // loses, and the chain is the longer stream, so the read call gets
  // shorter.  A raised wave priority (s_setprio 1 at kernel entry) was
  // tried with either shape and changed nothing measurable.  Measured
  // again with row-major output staged through LDS
  // (profiles/r05_score_walk.md): the two widths give the same call
  // time, 64 is 0.005..0.008 ms shorter alone; 64 stays.
  dispatch_algo(algo, [&](auto A) {
    dispatch_chain_block_size(block_size, [&](auto S) {
      constexpr int AL = decltype(A)::value;
      constexpr int BS = decltype(S)::value;
      if constexpr (AL == ALGO_FNV64A)
        launch(k_fnv_chain_tr<BS>, 64, row_major ? chain_stage_bytes(64) : 0);
      else
        launch(k_sha_chain_tr<BS, AL>, sha_tr_threads(BS), 0);
    });
  });
  return out;
}

std::vector<at::Tensor> kvidx::gpu_stage_ragged_tokens(
    at::Tensor tokens, at::Tensor offsets, int64_t block_size) {
  auto p = plan_ragged(tokens, offsets, block_size);
  at::Device dev = tokens.is_cuda()
                       ? tokens.device()
                       : at::Device(at::kCUDA, at::cuda::current_device());
  return stage_ragged(p, tokens, block_size, dev);
}

// The read path with the chain on the device: stage -> chain (row-major)
// -> fused score over the padded rows, all on the current stream with no
// host wait in between.  Returns float32 [B, num_pods] on the table's
// device.  Scores equal hash_chain_batch + gpu_fused_score bit for bit:
// same chain function, same walk.
at::Tensor kvidx::gpu_score_flat_tokens(KVIDX_TABLE_PARAMS,
                                        at::Tensor tokens_flat,
                                        at::Tensor offsets, int64_t model_id,
                                        at::Tensor filter_words,
                                        at::Tensor weights, int64_t num_pods,
                                        int64_t epoch, int64_t init_hash_bits,
                                        int64_t block_size, int64_t n_tiers,
                                        int64_t algo) {
  TORCH_CHECK(keys.is_cuda(), "table must live on the GPU");
  TORCH_CHECK(algo_valid(algo), "unknown chain hash algo id ", algo);
  auto p = plan_ragged(tokens_flat, offsets, block_size);
  auto dev = keys.device();
  auto fopt = at::TensorOptions().device(dev).dtype(at::kFloat);
  if (p.B == 0 || p.max_k == 0) return at::zeros({p.B, num_pods}, fopt);
  auto staged = stage_ragged(p, tokens_flat, block_size, dev);
  auto parents = at::full({p.B}, init_hash_bits, fopt.dtype(at::kLong));
  auto hashes = gpu_hash_chain_tr(staged[0], parents, staged[1], block_size,
                                  p.max_k, 0, 1, algo);
  if (fused_score_fits(p.max_k, clamp_tiers(n_tiers), pod_words(num_pods)))
    return gpu_fused_score_rows(KVIDX_TABLE_ARGS, hashes, staged[1], model_id,
                                filter_words, weights, num_pods, epoch,
                                p.max_k, n_tiers);
  // The masks do not fit in LDS: gather the live slots of the rows into
  // flat hashes for gpu_score_hashes.  It asks fused_score_fits the same
  // question again, so from here its fused branch is never taken: this
  // is the two-kernel path.  The gather index comes from the host's
  // n_chunks, no wait.
  auto idx_h = at::empty({p.total_chunks}, at::kLong);
  auto off_h = at::empty({p.B + 1}, at::kInt);
  {
    const int32_t* nc = p.host.data_ptr<int32_t>();
    int64_t* ip = idx_h.data_ptr<int64_t>();
    int32_t* op = off_h.data_ptr<int32_t>();
    TORCH_CHECK(p.total_chunks <= INT32_MAX, "too many chunks in one batch");
    int64_t n = 0;
    for (int64_t b = 0; b < p.B; ++b) {
      op[b] = (int32_t)n;
      for (int64_t k = 0; k < nc[b]; ++k) ip[n++] = b * p.max_k + k;
    }
    op[p.B] = (int32_t)n;
  }
  auto flat = hashes.view({-1}).index_select(0, idx_h.to(dev));
  return gpu_score_hashes(KVIDX_TABLE_ARGS, flat, off_h.to(dev), model_id,
                          filter_words, weights, num_pods, epoch, p.max_k,
                          n_tiers);
}

void kvidx::gpu_apply_events(KVIDX_TABLE_PARAMS, at::Tensor tokens,
                             at::Tensor tok_off, at::Tensor ehashes,
                             at::Tensor eh_off, at::Tensor parents,
                             at::Tensor has_parent, at::Tensor ev_type,
                             at::Tensor pod_entry, at::Tensor grp_off,
                             at::Tensor model_of, int64_t init_hash_bits,
                             int64_t block_size, int64_t epoch,
                             int64_t shard_id, int64_t num_shards,
                             int64_t algo) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  int64_t G = grp_off.numel() - 1;
  if (G == 0) return;
  TORCH_CHECK(model_of.numel() == ev_type.numel(),
              "model_of must have one id per event");
  auto req_scratch = at::empty({std::max<int64_t>(ehashes.numel(), 1)},
                               ehashes.options());
  const int waves_per_block = 4;
  int blocks = (int)((G + waves_per_block - 1) / waves_per_block);
  dispatch_algo(algo, [&](auto A) {
    hipLaunchKernelGGL(
        k_apply_events<decltype(A)::value>, dim3(blocks),
        dim3(waves_per_block * 64), 0, STREAM, v, tokens.data_ptr<int64_t>(),
        i32p(tok_off), u64p(ehashes), i32p(eh_off), u64p(parents),
        u8p(has_parent), u8p(ev_type), u32p(pod_entry), i32p(grp_off),
        i32p(model_of), G, (uint64_t)init_hash_bits, (int)block_size,
        (int32_t)epoch, (int)shard_id, (int)num_shards, u64p(req_scratch));
  });
}

// Transposed-chain phase-split apply: NO batch-local parents (host
// verified), so chains run one lane per EVENT from transposed int32
// tokens; inserts thread-per-block as usual.  No bmap is needed -
// parents resolve via the persistent engine map or the chain root.
void kvidx::gpu_apply_events_split_tr(KVIDX_TABLE_PARAMS,
                                      at::Tensor tokens_flat,
                                      at::Tensor tok_off, at::Tensor ehashes,
                                      at::Tensor eh_off, at::Tensor parents,
                                      at::Tensor has_parent,
                                      at::Tensor ev_type, at::Tensor pod_entry,
                                      at::Tensor ev_of, at::Tensor model_of,
                                      int64_t init_hash_bits,
                                      int64_t block_size, int64_t epoch,
                                      int64_t shard_id, int64_t num_shards,
                                      int64_t max_tokens, int64_t algo) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  TORCH_CHECK(tokens_flat.dtype() == at::kInt,
              "event tokens must be int32 (uint32 bit pattern)");
  TORCH_CHECK(block_size <= 64, "event chain kernel supports block_size<=64");
  int64_t E = ev_type.numel();
  int64_t n = ehashes.numel();
  if (E == 0 || n == 0) return;
  TORCH_CHECK(max_tokens > 0, "max_tokens must be positive");
  auto tokens_t = at::empty({max_tokens, E},
                            tokens_flat.options());
  auto req_scratch = at::zeros({n}, ehashes.options());
  int threads = 256;
  {
    int ygrid = (int)std::min<int64_t>((max_tokens + threads - 1) / threads,
                                       64);
    hipLaunchKernelGGL(k_transpose_ev_tokens, dim3((int)E, ygrid),
                       dim3(threads), 0, STREAM, i32p(tokens_flat),
                       i32p(tok_off), E, i32p(tokens_t));
  }
  TORCH_CHECK(model_of.numel() == E, "model_of must have one id per event");
  dispatch_algo(algo, [&](auto A) {
    launch_1d(k_event_chains_ev<decltype(A)::value>, E, v, i32p(tokens_t),
              i32p(tok_off), u64p(ehashes), i32p(eh_off), u64p(parents),
              u8p(has_parent), u8p(ev_type), i32p(model_of), E,
              (uint64_t)init_hash_bits, (int)block_size, u64p(req_scratch));
  });
  launch_event_inserts(v, ehashes, eh_off, ev_of, ev_type, tok_off, pod_entry,
                       model_of, block_size, epoch, shard_id, num_shards,
                       req_scratch);
}

// Phase-split apply: bmap build -> chains (lane per group) -> inserts
// (thread per block).  ev_of: int32 [total blocks] = owning event index.
void kvidx::gpu_apply_events_split(KVIDX_TABLE_PARAMS, at::Tensor tokens,
                                   at::Tensor tok_off, at::Tensor ehashes,
                                   at::Tensor eh_off, at::Tensor parents,
                                   at::Tensor has_parent, at::Tensor ev_type,
                                   at::Tensor pod_entry, at::Tensor grp_off,
                                   at::Tensor ev_of, at::Tensor model_of,
                                   int64_t init_hash_bits, int64_t block_size,
                                   int64_t epoch, int64_t shard_id,
                                   int64_t num_shards, int64_t algo) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  int64_t G = grp_off.numel() - 1;
  int64_t n = ehashes.numel();
  if (G == 0 || n == 0) return;
  int64_t bcap = 4;
  while (bcap < n * 2) bcap <<= 1;
  auto bkeys = at::zeros({bcap}, ehashes.options());
  auto bvals = at::zeros({bcap}, ehashes.options().dtype(at::kInt));
  auto req_scratch = at::zeros({n}, ehashes.options());

  TORCH_CHECK(model_of.numel() == ev_type.numel(),
              "model_of must have one id per event");
  TORCH_CHECK(ev_of.numel() == n, "ev_of must have one event per hash");
  launch_1d(k_batch_bmap, n, u64p(ehashes), i32p(eh_off), i32p(ev_of),
            u8p(ev_type), i32p(tok_off), i32p(grp_off), (int)G,
            (int)block_size, n, u64p(bkeys), i32p(bvals), bcap - 1);
  dispatch_algo(algo, [&](auto A) {
    launch_1d(k_event_chains<decltype(A)::value>, G, v,
              tokens.data_ptr<int64_t>(), i32p(tok_off), u64p(ehashes),
              i32p(eh_off), u64p(parents), u8p(has_parent), u8p(ev_type),
              i32p(grp_off), i32p(model_of), G, (uint64_t)init_hash_bits,
              (int)block_size, u64p(bkeys), i32p(bvals), bcap - 1,
              u64p(req_scratch));
  });
  launch_event_inserts(v, ehashes, eh_off, ev_of, ev_type, tok_off, pod_entry,
                       model_of, block_size, epoch, shard_id, num_shards,
                       req_scratch);
}
