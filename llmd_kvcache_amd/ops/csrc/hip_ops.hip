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

// dev_probe_collect for a key whose pods can no longer score: the find and
// the LRU touch, no pod row read, no mask.
DEV void dev_probe_touch(const Table& v, uint64_t h, uint32_t model,
                         int32_t epoch) {
  int64_t slot = dev_table_find(v, h, model);
  if (slot >= 0) v.stamp[slot] = epoch;
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

// ---- table sweeps ------------------------------------------------------
// One pass over pods[C * P] read as the flat array it is: the shape of the
// purge, the remap and the census.  sweep_table below walks it for the
// purge and the census; the remap has the same walk written out (see
// there).  A workgroup takes tiles of SWEEP_ROWS
// whole table rows (sweep_tile in kvidx_common.h): SWEEP_ROWS * P dwords
// start on a 1 KB boundary whatever P is, so a tile is read as 16-byte
// vectors, consecutive lanes taking consecutive vectors, SWEEP_VECS in
// flight per lane, and no row leaves its tile.  Inside the tile rows do
// straddle vectors and waves (P = 10: a row is 2.5 vectors), so the lane
// that holds a dword is not the lane that decides about its row: thread r
// publishes row r's state in LDS under a first barrier, every lane reports
// what it saw of a row to that state (sweep_vec_rows names the row), and
// after a second barrier thread r reads row r's state and acts on it.
// Nothing is read from global memory twice.
//
// What a kernel brings to the walk, as a struct K:
//   row_load(row)            a per-row load that goes out with the meta load
//   row_begin(r, m)          thread r: row r's LDS state from its meta word
//   vec(e, r, vi, tile_p)    one loaded vector: its four dwords, their tile
//                            rows, its index in the tile, the tile's dwords
//   dword(e, row, p)         one dword read from *p (tables under 4 rows)
//   row_end(r, row, x)       thread r after the second barrier; x is what
//                            row_load returned
// and its counters in K::c, which leave through wg_sum_store.

// dst[i] = the workgroup's sum of c[i]: wave shuffle, N words per wave in
// LDS, one barrier, N plain stores by threads 0..N-1.  Plain stores into a
// row of per-workgroup partials, which the op sums after its readback, in
// place of atomic adds: no counter has to be zeroed before the launch.
template <int N>
DEV void wg_sum_store(const uint32_t (&c)[N], uint32_t* dst) {
  __shared__ uint32_t s_red[N * (SWEEP_THREADS / 64)];
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    uint32_t x = c[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if ((tid & 63) == 0) s_red[N * (tid >> 6) + i] = x;
  }
  __syncthreads();
  if (tid < N) {
    uint32_t s = 0;
    for (int w = 0; w < SWEEP_THREADS / 64; ++w) s += s_red[N * w + tid];
    dst[tid] = s;
  }
}

// A table of fewer than 4 rows (capacity 1 or 2) can have fewer than 4
// dwords, or a dword count that is no multiple of 4: one workgroup walks
// it dword by dword.  Every larger table is whole vectors.
template <typename K>
DEV void sweep_tiny_table(const Table& v, K& k) {
  const uint32_t P = (uint32_t)v.pods_per_key;
  const uint32_t rows = (uint32_t)v.cap_mask + 1;
  const uint32_t tid = threadIdx.x;
  const uint32_t mine = tid < rows ? tid : 0u;
  const auto x = k.row_load(mine);
  k.row_begin((int)tid, tid < rows ? v.meta[mine] : 0u);
  __syncthreads();
  for (uint32_t i = tid; i < rows * P; i += SWEEP_THREADS)
    k.dword(v.pods[i], i / P, v.pods + i);
  __syncthreads();
  if (tid < rows) k.row_end((int)tid, tid, x);
}

template <bool CLAMPED, typename K>
DEV void sweep_table(const Table& v, int64_t n_tiles, K& k) {
  const int tid = threadIdx.x;
  const uint32_t P = (uint32_t)v.pods_per_key;
  const uint64_t cap = v.cap_mask + 1;
  if (cap < 4) {  // one tile, one workgroup (the op launches one)
    if (blockIdx.x == 0) sweep_tiny_table(v, k);
    return;
  }
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    // capacity >= 4: a tile is 4..256 rows, a whole number of vectors
    const SweepTile t = sweep_tile(cap, P, tile);
    uint32_t* tile_p = v.pods + t.row0 * P;
    const uint4* tile_v = reinterpret_cast<const uint4*>(tile_p);

    // CLAMPED: every load is unconditional, at a clamped index, so that
    // all of a round's loads go out back to back and each is waited for by
    // its own count: meta first (the only one needed ahead of the
    // barrier), the kernel's row load right behind it (not looked at until
    // the tile is done), then the vectors.  A lane past the end rereads
    // the last row or vector, a line its neighbours fetch anyway, and
    // drops it.  Otherwise a lane past the end loads nothing and walks a
    // zero vector.  Each kernel takes the form that measured faster for it
    // (profiles/r10_pod_census.md, r11_table_sweeps.md).
    const uint64_t my_row =
        t.row0 + (uint32_t)(tid < t.rows ? tid : t.rows - 1);
    const uint32_t m_mine =
        CLAMPED || tid < t.rows ? v.meta[my_row] : 0u;
    const auto x_mine = k.row_load(my_row);
    uint32_t base = 0;
    do {
      uint4 q[SWEEP_VECS];
#pragma unroll
      for (int i = 0; i < SWEEP_VECS; ++i) {
        const uint32_t vi = base + i * SWEEP_THREADS + tid;
        if (CLAMPED)
          q[i] = tile_v[vi < t.n_vec ? vi : t.n_vec - 1];
        else
          q[i] = vi < t.n_vec ? tile_v[vi] : make_uint4(0, 0, 0, 0);
      }
      if (base == 0) {
        k.row_begin(tid, tid < t.rows ? m_mine : 0u);
        __syncthreads();
      }
#pragma unroll
      for (int i = 0; i < SWEEP_VECS; ++i) {
        const uint32_t vi = base + i * SWEEP_THREADS + tid;
        // a vector past the tile is dropped, not walked a second time
        if ((CLAMPED && vi >= t.n_vec) || (q[i].x | q[i].y | q[i].z | q[i].w) == 0)
          continue;
        const uint32_t e[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
        uint32_t r[4];  // all inside the tile
        sweep_vec_rows(vi, P, r);
        k.vec(e, r, vi, tile_p);
      }
      base += SWEEP_THREADS * SWEEP_VECS;
    } while (base < t.n_vec);
    __syncthreads();
    // thread r owns row r: it wrote the row's LDS state and is the one to
    // rewrite it for the next tile, so no third barrier
    if (tid < t.rows) k.row_end(tid, t.row0 + tid, x_mine);
  }
}

// ---- purge by pod ------------------------------------------------------
// Row state: the row's meta word (slot eligibility) and a flag word to
// which every lane reports what it did to an entry of the row (ROW_HIT:
// cleared it; ROW_LIVE: it remains); thread r tombstones row r if it was
// hit and nothing remains.  Neighbouring lanes ask for the same or the
// next row: broadcast or distinct banks.  The purge bitmap (<= 512 B) sits
// in LDS as well; the bitmap test is one data-dependent ds_read_b32 for
// the few entries that are not empty.
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

struct PurgeSweep {
  const Table& v;
  const uint32_t* s_bits;
  uint32_t n_bits;
  int model_id;
  uint32_t* s_meta;   // [SWEEP_ROWS]
  uint32_t* s_flags;  // [SWEEP_ROWS]
  uint32_t c[2] = {0, 0};  // entries cleared, keys tombstoned
  DEV uint32_t row_load(uint64_t) const { return 0u; }
  DEV void row_begin(int r, uint32_t m) {
    s_meta[r] = m;
    s_flags[r] = 0;
  }
  DEV void dword(uint32_t e, uint32_t row, uint32_t* p) {
    purge_entry(e, p, (int)row, s_bits, n_bits, s_meta, model_id, s_flags,
                c[0]);
  }
  DEV void vec(const uint32_t (&e)[4], const uint32_t (&r)[4], uint32_t vi,
               uint32_t* tile_p) {
#pragma unroll
    for (int j = 0; j < 4; ++j) dword(e[j], r[j], tile_p + vi * 4 + j);
  }
  DEV void row_end(int r, uint64_t row, uint32_t) {
    if (s_flags[r] != ROW_HIT || (s_meta[r] & META_TOMB)) return;
    const uint32_t old = atomicOr(&v.meta[row], META_TOMB);
    c[1] += (old & META_TOMB) ? 0u : 1u;
  }
};

// bits: the purge bitmap as n_bit_words 32-bit words (pod id pid is bit
// pid % 32 of word pid / 32).  model_id -1: every model.  partials
// [gridDim.x][2]: each workgroup's {entries cleared, keys tombstoned}.
__global__ void __launch_bounds__(SWEEP_THREADS) k_purge_pods(
    Table v, const uint32_t* __restrict__ bits, int n_bit_words, int model_id,
    int64_t n_tiles, uint32_t* __restrict__ partials) {
  __shared__ uint32_t s_bits[128];
  __shared__ uint32_t s_meta[SWEEP_ROWS];
  __shared__ uint32_t s_flags[SWEEP_ROWS];
  // the walk's first barrier publishes the bitmap
  if ((int)threadIdx.x < n_bit_words) s_bits[threadIdx.x] = bits[threadIdx.x];
  PurgeSweep k{v, s_bits, (uint32_t)n_bit_words * 32u, model_id, s_meta,
               s_flags};
  sweep_table<false>(v, n_tiles, k);
  wg_sum_store(k.c, partials + 2 * blockIdx.x);
}

// ---- remap pod ids -----------------------------------------------------
// The purge with a code table in place of the bitmap, on a tile loop of
// its own: on sweep_table the identity remap measured 1..5 % slower than
// this loop under either load form (profiles/r11_table_sweeps.md), so the
// kernel stays as it was, tails for capacity 1 and 2 included.  The table
// (remap_entry's codes, 2 B per id, only the n given) is staged in LDS
// once per workgroup: 8 KB at n = 4096, 10 288 B static LDS in all, and
// the translation is one data-dependent ds_read_u16 per non-empty entry.
// A moved entry reports ROW_LIVE, a dropped one ROW_HIT.
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
__global__ void __launch_bounds__(SWEEP_THREADS) k_remap_pods(
    Table v, const int32_t* __restrict__ remap, int n, int64_t n_tiles,
    uint32_t* __restrict__ partials) {
  __shared__ uint16_t s_codes[MAX_PODS];
  __shared__ uint32_t s_meta[SWEEP_ROWS];
  __shared__ uint32_t s_flags[SWEEP_ROWS];
  __shared__ uint32_t s_red[3 * (SWEEP_THREADS / 64)];
  const int tid = threadIdx.x;
  const uint32_t P = (uint32_t)v.pods_per_key;
  const uint64_t cap = v.cap_mask + 1;
  const uint32_t un = (uint32_t)n;
  // two codes per lane and store; the first tile's barrier publishes them
  for (int i = 2 * tid; i < n; i += 2 * SWEEP_THREADS) {
    const uint32_t lo = (uint32_t)(remap[i] + 1);
    const uint32_t hi = i + 1 < n ? (uint32_t)(remap[i + 1] + 1) : 0u;
    reinterpret_cast<uint32_t*>(s_codes)[i >> 1] = lo | (hi << 16);
  }
  uint32_t n_moved = 0, n_cleared = 0, n_tomb = 0;

  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = (uint64_t)tile * SWEEP_ROWS;
    const uint64_t rows_left = cap - row0;
    const int rows = rows_left < SWEEP_ROWS ? (int)rows_left : SWEEP_ROWS;
    const uint32_t n_dw = (uint32_t)rows * P;
    const uint32_t n_vec = n_dw >> 2;
    uint32_t* tile_p = v.pods + row0 * P;
    uint4* tile_v = reinterpret_cast<uint4*>(tile_p);

    const uint32_t m_mine = tid < rows ? v.meta[row0 + tid] : 0u;
    uint32_t base = 0;
    do {
      uint4 q[SWEEP_VECS];
#pragma unroll
      for (int k = 0; k < SWEEP_VECS; ++k) {
        const uint32_t vi = base + k * SWEEP_THREADS + tid;
        q[k] = vi < n_vec ? tile_v[vi] : make_uint4(0, 0, 0, 0);
      }
      if (base == 0) {
        s_meta[tid] = m_mine;
        s_flags[tid] = 0;
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < SWEEP_VECS; ++k) {
        const uint32_t vi = base + k * SWEEP_THREADS + tid;
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
      base += SWEEP_THREADS * SWEEP_VECS;
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
    for (int w = 0; w < SWEEP_THREADS / 64; ++w) s += s_red[3 * w + tid];
    partials[3 * blockIdx.x + tid] = s;
  }
}

// ---- pod census --------------------------------------------------------
// The read-only sweep: nothing goes back to the table.  What it keeps:
//  - the pod x tier histogram, uint32 bins in dynamic LDS (num_pods *
//    n_tiers words: 512 B for 64 pods x 2 tiers, 64 KB at MAX_PODS x
//    MAX_TIERS), zeroed once per workgroup and carried across its
//    grid-stride loop; a non-empty entry of a live row is one ds_add_u32
//    with no return value;
//  - one LDS word per tile row: the row's meta bits (OCC, TOMB, model) with
//    a count of the row's non-zero entries in the free bits 16..29.  A lane
//    sums the non-zero entries it saw of a row over its vector and adds
//    them there once; after the barrier thread r classifies row r from
//    that one word (live / tombstoned / full) and looks at e_meta[row0 +
//    r], whose load went out with the meta load;
//  - unknown-bin hits and the six scalar counters in registers.
// Each workgroup leaves through plain stores into its row of partials
// [gridDim.x][bins + 6]; k_census_reduce sums the rows.  No fill pass and
// no global atomic.
constexpr uint32_t ROW_COUNT_SHIFT = 16;  // pods_per_key <= 4096: 13 bits
constexpr uint32_t ROW_META_BITS = META_OCC | META_TOMB | META_MODEL_MASK;
constexpr uint32_t ROW_COUNT_MASK = 0x3FFFu;
constexpr int64_t CENSUS_PARTIAL_BYTES = 32ll << 20;

// One entry e (possibly empty) of a tile row whose LDS word is rw.  The
// counters move by predicates; the one branch is around the LDS add.
DEV void census_entry(uint32_t e, uint32_t rw, int model_id,
                      uint32_t num_pods, uint32_t n_tiers, uint32_t* s_hist,
                      uint32_t& n_entries, uint32_t& n_unknown) {
  const bool counted = e != 0 && census_slot(rw, model_id) == CENSUS_LIVE;
  const int32_t b = census_bin(e, num_pods, n_tiers);
  n_entries += counted ? 1u : 0u;
  n_unknown += (counted && b < 0) ? 1u : 0u;
  if (counted && b >= 0)
    atomicAdd(&s_hist[b], 1u);  // result unused: no return value asked for
}

struct CensusSweep {
  const Table& v;
  int model_id;
  uint32_t num_pods, n_tiers;
  uint32_t* s_hist;  // [num_pods * n_tiers]
  uint32_t* s_row;   // [SWEEP_ROWS]
  // CensusSummary's order: live, tombstoned, full, entries, unknown, emap
  uint32_t c[CENSUS_SUMMARY_LEN] = {0, 0, 0, 0, 0, 0};
  DEV uint32_t row_load(uint64_t row) const { return v.e_meta[row]; }
  DEV void row_begin(int r, uint32_t m) { s_row[r] = m & ROW_META_BITS; }
  DEV void entry(uint32_t e, uint32_t rw) {
    census_entry(e, rw, model_id, num_pods, n_tiers, s_hist, c[3], c[4]);
  }
  DEV void dword(uint32_t e, uint32_t row, uint32_t*) {
    entry(e, s_row[row]);
    if (e != 0) atomicAdd(&s_row[row], 1u << ROW_COUNT_SHIFT);
  }
  DEV void vec(const uint32_t (&e)[4], const uint32_t (&r)[4], uint32_t,
               uint32_t*) {
    uint32_t rw[4];  // the four row words in one round of LDS reads
#pragma unroll
    for (int j = 0; j < 4; ++j) rw[j] = s_row[r[j]];
    uint32_t run = 0;  // non-zero entries of the current row so far
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      entry(e[j], rw[j]);
      run += e[j] != 0 ? 1u : 0u;
      if (j == 3 || r[j + 1 < 4 ? j + 1 : 3] != r[j]) {
        if (run) atomicAdd(&s_row[r[j]], run << ROW_COUNT_SHIFT);
        run = 0;
      }
    }
  }
  // em: the engine-map word of the same slot
  DEV void row_end(int r, uint64_t, uint32_t em) {
    const uint32_t rw = s_row[r];
    const CensusSlot s = census_slot(rw, model_id);
    c[0] += s == CENSUS_LIVE;
    c[1] += s == CENSUS_TOMB;
    c[2] += s == CENSUS_LIVE &&
            ((rw >> ROW_COUNT_SHIFT) & ROW_COUNT_MASK) ==
                (uint32_t)v.pods_per_key;
    c[5] += census_slot(em, model_id) == CENSUS_LIVE;
  }
};

__global__ void __launch_bounds__(SWEEP_THREADS) k_pod_census(
    Table v, int model_id, int num_pods, int n_tiers, int64_t n_tiles,
    uint32_t* __restrict__ partials) {
  extern __shared__ uint32_t s_hist[];  // [num_pods * n_tiers]
  __shared__ uint32_t s_row[SWEEP_ROWS];
  const uint32_t tid = threadIdx.x;
  const uint32_t bins = (uint32_t)num_pods * (uint32_t)n_tiers;
  // (the walk's first barrier publishes the zeros)
  for (uint32_t i = tid; i < bins; i += SWEEP_THREADS) s_hist[i] = 0;
  CensusSweep k{v, model_id, (uint32_t)num_pods, (uint32_t)n_tiers, s_hist,
                s_row};
  sweep_table<true>(v, n_tiles, k);
  // the barrier inside wg_sum_store also closes the histogram: no lane
  // copies a bin out while another wave may still add to it
  uint32_t* mine = partials + (size_t)blockIdx.x * (bins + CENSUS_SUMMARY_LEN);
  wg_sum_store(k.c, mine + bins);
  for (uint32_t i = tid; i < bins; i += SWEEP_THREADS) mine[i] = s_hist[i];
}

// out[c] = sum over the n_rows workgroup rows of partials[r][c].  A thread
// owns one column, so the 64 lanes of a wave read 64 neighbouring words of
// a row; with one thread per column and nothing else, 134 columns under
// 2048 rows were one workgroup walking 2048 dependent loads (0.46 ms
// measured), so a workgroup is 64 columns x 16 row slices: wave s sums rows
// s, s + 16, ... of its columns, eight loads in flight, and the slices meet
// in LDS.
constexpr int REDUCE_COLS = 64, REDUCE_SLICES = 16;
__global__ void __launch_bounds__(REDUCE_COLS * REDUCE_SLICES)
    k_census_reduce(const uint32_t* __restrict__ partials, int n_rows,
                    int n_cols, int64_t* __restrict__ out) {
  __shared__ unsigned long long s_part[REDUCE_SLICES][REDUCE_COLS];
  const int lane = threadIdx.x % REDUCE_COLS, slice = threadIdx.x / REDUCE_COLS;
  const int c = blockIdx.x * REDUCE_COLS + lane;
  unsigned long long s = 0;
  if (c < n_cols) {
#pragma unroll 8
    for (int r = slice; r < n_rows; r += REDUCE_SLICES)
      s += partials[(size_t)r * n_cols + c];
  }
  s_part[slice][lane] = s;
  __syncthreads();
  if (slice == 0 && c < n_cols) {
    for (int i = 1; i < REDUCE_SLICES; ++i) s += s_part[i][lane];
    out[c] = (int64_t)s;
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

// ---- score top-n: selection (the contract: kvidx_common.h rank_key) -----
// Two device functions under k_fused_topk[_rows] and k_topk_rows.

// Wave-wide unsigned 64-bit maximum, returned in scalar registers: every
// lane ends the butterfly with the same value, and saying so lets the
// rounds below compare against it and branch on it as scalars.
DEV uint64_t wave_max_u64(uint64_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t y = __shfl_xor(x, off, 64);
    x = y > x ? y : x;
  }
  // the builtin returns int: without the casts the low word sign-extends
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32));
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
  return ((uint64_t)hi << 32) | lo;
}

// Selection inside a wave, no removal.  A lane holds N rank keys in
// registers; round r takes the wave maximum over the keys strictly below
// round r - 1's winner.  Keys of different pods are never equal, so the
// bound stands in for removing the winner: key[] is only ever indexed by
// the unrolled i (a runtime index would put it behind gpr_idx moves or in
// scratch), and no lane diverges.  Returns round `lane`'s winner in lanes
// 0..top_n-1 and 0 (no candidate) everywhere else; the rounds stop at the
// first wave maximum that is no candidate.
template <int N>
DEV uint64_t wave_topk(const uint64_t (&key)[N], int top_n, int lane) {
  uint64_t bound = ~0ull;  // above every key: a finite score's bits
  uint64_t mine = 0;
  for (int r = 0; r < top_n; ++r) {
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
      m = (key[i] < bound && key[i] > m) ? key[i] : m;
    bound = wave_max_u64(m);
    if (bound < RANK_KEY_MIN) break;
    mine = lane == r ? bound : mine;
  }
  return mine;
}

// Merge across the workgroup's four waves and store one prompt's result
// rows.  mine: wave_topk's return.  xch: uint64 [4][MAX_TOPK] in LDS that
// nobody reads any more.  Each wave parks its MAX_TOPK slots (zeros past
// its winners, so nothing stale is ever read); after one barrier wave 0
// takes one parked key per lane, 4 x 16 = 64 exactly, runs the same rounds
// and lanes 0..top_n-1 store: ids and scores are one contiguous store of
// at most 64 B each, and every slot is written ((-1, 0.0f) where the
// candidates ran out).
DEV void wg_topk_store(uint64_t mine, uint64_t* xch, int top_n,
                       int32_t* __restrict__ ids_row,
                       float* __restrict__ scores_row) {
  static_assert(4 * MAX_TOPK == 64, "one parked key per lane of wave 0");
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (lane < MAX_TOPK) xch[wave * MAX_TOPK + lane] = mine;
  __syncthreads();
  if (wave != 0) return;
  const uint64_t parked[1] = {xch[lane]};
  const uint64_t win = wave_topk(parked, top_n, lane);
  if (lane < top_n) {
    ids_row[lane] = rank_key_id(win);
    scores_row[lane] = rank_key_score(win);
  }
}

// What a top-n kernel writes: ids int32 [B, top_n], scores float32
// [B, top_n].
struct TopkOut {
  int32_t* __restrict__ ids;
  float* __restrict__ scores;
  int top_n;
};

// Epilogue policies of fused_score_body.  word() is called by every lane
// once per 64-pod word its wave walked, with the pod's final score;
// finish() once by every thread after the walk, with the dynamic LDS.
//
// ScoreStore: the [B, num_pods] matrix (k_fused_score[_rows]).
struct ScoreStore {
  float* __restrict__ scores;
  DEV void word(int b, int pid, int num_pods, float score) {
    if (pid < num_pods) scores[(size_t)b * num_pods + pid] = score;
  }
  DEV void finish(int, unsigned long long*) {}
};

// ScoreTopk: nothing per pod leaves the registers.  A wave walks words
// wave, wave + 4, ...: at most four because W <= 16, so a lane ends with
// at most four keys.  They sit in a four-deep shift register, which takes
// the walk's runtime word loop without a runtime-indexed array; unused
// places stay 0.  The exchange area overlays the front of the mask area:
// the first barrier is the last wave's walk, after it nobody reads masks.
struct ScoreTopk {
  TopkOut out;
  uint64_t key[4] = {0, 0, 0, 0};
  DEV void word(int, int pid, int num_pods, float score) {
    key[3] = key[2];
    key[2] = key[1];
    key[1] = key[0];
    key[0] = pid < num_pods ? rank_key(score, (uint32_t)pid) : 0ull;
  }
  DEV void finish(int b, unsigned long long* lds) {
    const uint64_t mine = wave_topk(key, out.top_n, threadIdx.x & 63);
    __syncthreads();
    wg_topk_store(mine, reinterpret_cast<uint64_t*>(lds), out.top_n,
                  out.ids + (size_t)b * out.top_n,
                  out.scores + (size_t)b * out.top_n);
  }
};

// Fused probe + longest-prefix score. One workgroup per prompt; dynamic
// LDS holds the per-key per-tier masks; the four waves then walk keys in
// order, a 64-pod word each, with the active pod set in registers.
//
// The body is shared by four entries.  They differ in where prompt b's
// keys lie: k_fused_score and k_fused_topk take flat hashes with offsets
// [B+1], k_fused_score_rows and k_fused_topk_rows take padded rows (h =
// hashes + b * stride, K = n_keys[b]) as the row-major chain kernel
// leaves them; and in the epilogue policy, the score matrix or top-n.
template <typename Epilogue>
DEV void fused_score_body(
    Table v, const uint64_t* __restrict__ h, const int K,
    uint32_t model, const uint64_t* __restrict__ filter, int has_filter,
    const float* __restrict__ weights, int num_pods, int W, int32_t epoch,
    int n_tiers, Epilogue epi) {
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
    epi.word(b, w * 64 + lane, num_pods, score);
  }
  epi.finish(b, lds_masks);
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
                   ScoreStore{scores});
}

// k_fused_score with the pick inside: ids / scores [B, top_n] in place of
// the matrix.  At least 512 B of dynamic LDS (the exchange area).
__global__ void __launch_bounds__(256) k_fused_topk(
    Table v, const uint64_t* __restrict__ hashes,
    const int32_t* __restrict__ offsets,  // [B+1]
    uint32_t model, const uint64_t* __restrict__ filter, int has_filter,
    const float* __restrict__ weights, int num_pods, int W, int32_t epoch,
    int n_tiers, TopkOut out) {
  const int b = blockIdx.x;
  fused_score_body(v, hashes + offsets[b], offsets[b + 1] - offsets[b], model,
                   filter, has_filter, weights, num_pods, W, epoch, n_tiers,
                   ScoreTopk{out});
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
                   has_filter, weights, num_pods, W, epoch, n_tiers,
                   ScoreStore{scores});
}

__global__ void __launch_bounds__(256) k_fused_topk_rows(
    Table v, const uint64_t* __restrict__ hashes,  // [B, stride]
    const int32_t* __restrict__ n_keys,               // [B]
    int64_t stride, uint32_t model, const uint64_t* __restrict__ filter,
    int has_filter, const float* __restrict__ weights, int num_pods, int W,
    int32_t epoch, int n_tiers, TopkOut out) {
  const int b = blockIdx.x;
  fused_score_body(v, hashes + (int64_t)b * stride, n_keys[b], model, filter,
                   has_filter, weights, num_pods, W, epoch, n_tiers,
                   ScoreTopk{out});
}

// ---- tiled fused score: any K, any W <= 64, one launch -----------------
// fused_score_body keeps all K keys' masks in LDS, which bounds K and W.
// Nothing in the scoring needs that: the walk is sequential in k and
// carries an active bit and a score per pod.  Here that state stays in
// registers for the whole prompt and the keys pass through LDS KT at a
// time, in two tile buffers [KT, n_tiers, W] (KT: tiled_score_tile_keys on
// the host), followed by two vote words.
//
// Work split: one workgroup of 256 per prompt; wave v owns words v, v + 4,
// ..., WPW = ceil(W / 4) of them at most, a compile-time bound picked on
// the host so that score[] / active[] are only indexed by unrolled
// constants; a word past W is skipped wave-uniformly.  Lane l owns pod
// bit l.
//
// Step i = -1 .. n_tiles - 1, two barriers each:
//   A  zero the buffer of tile i + 1 (all threads) | barrier
//   B  probe tile i + 1 into it: key j of the tile by lane j / 4 of wave
//      j % 4, so every wave has probes in flight; then walk tile i from
//      the other buffer, which step i - 1 probed | barrier
// A wave that is through with its probes walks while the others' probes
// are still in flight, and a wave without a live word only probes.
//
// After the break: a word whose active set emptied is never walked again
// (live, a wave-uniform bit per word).  Each wave that still has a live
// word after tile i says so in vote word i & 1 before barrier B; if none
// did, nothing can score any more and the workgroup leaves the loop.  Tile
// i + 1 is probed by then; the keys from (i + 2) * KT on are found and
// stamped by dev_probe_touch, 256 at a time, no LDS, no barrier - stamp
// ends as the split route leaves it.
//
// Scores are bit-identical to fused_score_body's and cpu_fused_score's:
// the same dev_probe_collect and score_walk_step, per pod in key order.

// Epilogues over a lane's WPW final scores; both run behind the loop's
// last barrier, after which nobody reads masks.
template <int WPW>
DEV void tiled_finish(ScoreStore out, int b, const float (&score)[WPW], int W,
                      int num_pods, unsigned long long*) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < WPW; ++j) {
    const int w = wave + 4 * j;
    if (w < W) out.word(b, w * 64 + lane, num_pods, score[j]);
  }
}

// One rank key per word, straight into wave_topk<WPW>; the exchange area
// overlays the front of tile buffer 0.
template <int WPW>
DEV void tiled_finish(TopkOut out, int b, const float (&score)[WPW], int W,
                      int num_pods, unsigned long long* lds) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  uint64_t key[WPW];
#pragma unroll
  for (int j = 0; j < WPW; ++j) {
    const int pid = (wave + 4 * j) * 64 + lane;
    key[j] = (wave + 4 * j < W && pid < num_pods)
                 ? rank_key(score[j], (uint32_t)pid)
                 : 0ull;
  }
  const uint64_t mine = wave_topk(key, out.top_n, lane);
  wg_topk_store(mine, reinterpret_cast<uint64_t*>(lds), out.top_n,
                out.ids + (size_t)b * out.top_n,
                out.scores + (size_t)b * out.top_n);
}

template <int WPW, typename Out>
DEV void tiled_score_body(
    Table v, const uint64_t* __restrict__ h, const int K, uint32_t model,
    const uint64_t* __restrict__ filter, int has_filter,
    const float* __restrict__ weights, int num_pods, int W, int32_t epoch,
    int n_tiers, int KT, Out out) {
  extern __shared__ unsigned long long lds_masks[];  // 2 x [KT, n_tiers, W]
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  // scalar, so that word indices and the live bits are wave-uniform to
  // the compiler as well
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int TW = n_tiers * W;
  const int tile_words = KT * TW;
  int* vote = reinterpret_cast<int*>(lds_masks + 2 * tile_words);  // [2]
  const int n_tiles = (K + KT - 1) / KT;

  float score[WPW];
  int active[WPW];
  unsigned live = 0;  // bit j: word wave + 4 j can still score
#pragma unroll
  for (int j = 0; j < WPW; ++j) {
    score[j] = 0.f;
    active[j] = 0;
    if (wave + 4 * j < W) live |= 1u << j;
  }

  int k_touch = K;  // first key of the touch-only tail
  for (int i = -1; i < n_tiles; ++i) {
    // A: the next tile's buffer, and this step's vote word
    const int nk0 = (i + 1) * KT;
    const int nlen = min(KT, K - nk0);  // <= 0: there is no next tile
    unsigned long long* nbuf = lds_masks + ((i + 1) & 1) * tile_words;
    for (int x = threadIdx.x; x < nlen * TW; x += blockDim.x) nbuf[x] = 0;
    if (threadIdx.x == 0) vote[i & 1] = 0;
    __syncthreads();

    // B: the next tile's probes, then this tile's walk
    const int j = lane * 4 + wave;
    if (j < nlen)
      dev_probe_collect(v, h[nk0 + j], model, filter, has_filter, num_pods, W,
                        epoch, nbuf + (size_t)j * TW, n_tiers);
    if (i >= 0) {
      const int k0 = i * KT;
      const int len = min(KT, K - k0);
      const unsigned long long* cbuf = lds_masks + (i & 1) * tile_words;
#pragma unroll
      for (int jw = 0; jw < WPW; ++jw) {
        if (!((live >> jw) & 1)) continue;  // past W, or its set is empty
        const int w = wave + 4 * jw;
        for (int kk = 0; kk < len; ++kk) {
          const int act =
              score_walk_step(cbuf + (size_t)kk * TW + w, W, n_tiers, weights,
                              lane, k0 + kk == 0, active[jw], score[jw]);
          if (!__any(act)) {
            live &= ~(1u << jw);
            break;
          }
        }
      }
      if (live && lane == 0) vote[i & 1] = 1;
    }
    __syncthreads();
    if (i >= 0 && !vote[i & 1]) {
      k_touch = (i + 2) * KT;
      break;
    }
  }
  for (int64_t k = (int64_t)k_touch + threadIdx.x; k < K; k += blockDim.x)
    dev_probe_touch(v, h[k], model, epoch);

  tiled_finish<WPW>(out, b, score, W, num_pods, lds_masks);
}

// The four entries: where prompt b's keys lie (flat hashes with offsets, or
// padded rows) x what leaves (the matrix, or top-n), as the resident fused
// kernels above.  Dynamic LDS: tiled_score_lds_bytes on the host.
template <int WPW>
__global__ void __launch_bounds__(256) k_tiled_score(
    Table v, const uint64_t* __restrict__ hashes,
    const int32_t* __restrict__ offsets,  // [B+1]
    uint32_t model, const uint64_t* __restrict__ filter, int has_filter,
    const float* __restrict__ weights, int num_pods, int W, int32_t epoch,
    int n_tiers, int KT, float* __restrict__ scores) {
  const int b = blockIdx.x;
  tiled_score_body<WPW>(v, hashes + offsets[b], offsets[b + 1] - offsets[b],
                        model, filter, has_filter, weights, num_pods, W, epoch,
                        n_tiers, KT, ScoreStore{scores});
}

template <int WPW>
__global__ void __launch_bounds__(256) k_tiled_topk(
    Table v, const uint64_t* __restrict__ hashes,
    const int32_t* __restrict__ offsets,  // [B+1]
    uint32_t model, const uint64_t* __restrict__ filter, int has_filter,
    const float* __restrict__ weights, int num_pods, int W, int32_t epoch,
    int n_tiers, int KT, TopkOut out) {
  const int b = blockIdx.x;
  tiled_score_body<WPW>(v, hashes + offsets[b], offsets[b + 1] - offsets[b],
                        model, filter, has_filter, weights, num_pods, W, epoch,
                        n_tiers, KT, out);
}

template <int WPW>
__global__ void __launch_bounds__(256) k_tiled_score_rows(
    Table v, const uint64_t* __restrict__ hashes,  // [B, stride]
    const int32_t* __restrict__ n_keys,               // [B]
    int64_t stride, uint32_t model, const uint64_t* __restrict__ filter,
    int has_filter, const float* __restrict__ weights, int num_pods, int W,
    int32_t epoch, int n_tiers, int KT, float* __restrict__ scores) {
  const int b = blockIdx.x;
  tiled_score_body<WPW>(v, hashes + (int64_t)b * stride, n_keys[b], model,
                        filter, has_filter, weights, num_pods, W, epoch,
                        n_tiers, KT, ScoreStore{scores});
}

template <int WPW>
__global__ void __launch_bounds__(256) k_tiled_topk_rows(
    Table v, const uint64_t* __restrict__ hashes,  // [B, stride]
    const int32_t* __restrict__ n_keys,               // [B]
    int64_t stride, uint32_t model, const uint64_t* __restrict__ filter,
    int has_filter, const float* __restrict__ weights, int num_pods, int W,
    int32_t epoch, int n_tiers, int KT, TopkOut out) {
  const int b = blockIdx.x;
  tiled_score_body<WPW>(v, hashes + (int64_t)b * stride, n_keys[b], model,
                        filter, has_filter, weights, num_pods, W, epoch,
                        n_tiers, KT, out);
}

// Top-n of any score matrix [B, P], 1 <= P <= MAX_PODS, values finite and
// >= 0: the route for what the fused kernel refuses.  One workgroup of 256
// per row; thread t loads columns t, t + 256, ... (a wave reads 256
// contiguous bytes per round), PER of them at most, PER a compile-time
// bound picked on the host so that the keys stay in registers.  A column
// past P contributes key 0.
constexpr int TOPK_ROWS_THREADS = 256;
template <int PER>
__global__ void __launch_bounds__(TOPK_ROWS_THREADS) k_topk_rows(
    const float* __restrict__ scores, int P, TopkOut out) {
  static_assert(PER * TOPK_ROWS_THREADS <= MAX_PODS, "PER is sized by P");
  __shared__ uint64_t xch[4 * MAX_TOPK];
  const int64_t b = blockIdx.x;
  const float* row = scores + b * P;
  uint64_t key[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = i * TOPK_ROWS_THREADS + (int)threadIdx.x;
    key[i] = c < P ? rank_key(row[c], (uint32_t)c) : 0ull;
  }
  const uint64_t mine = wave_topk(key, out.top_n, threadIdx.x & 63);
  wg_topk_store(mine, xch, out.top_n, out.ids + b * out.top_n,
                out.scores + b * out.top_n);
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

// ---- merged masks -> top-n, one launch ----------------------------------
// k_score_from_masks with tiled_score_body's work split and the pick
// inside: one workgroup of 256 per prompt, wave v owns words v, v + 4, ...
// (WPW of them at most, skipped wave-uniformly past W), lane l is pod bit
// l, score[] / active[] in registers for the whole prompt.  The [B,
// num_pods] matrix never exists.
//
// A prompt's masks are one contiguous span of K * T * W words.  It passes
// through LDS in tiles of KT keys (tiled_score_tile_keys), two buffers
// [KT, T, W], software-pipelined with ONE barrier per tile:
//   issue tile i + 1's global loads into registers (thread t takes vectors
//   t, t + 256, ..., NV at most) | walk tile i out of buffer i & 1 | write
//   the registers to buffer (i + 1) & 1, which was last read before the
//   previous barrier | barrier.
// The loads are in flight for the length of the walk.  V16: 16-byte
// vectors, chosen on the host where T * W is even and the base is 16-byte
// aligned (every span then starts and ends on a 16-byte boundary); else
// 8-byte vectors, twice as many.
//
// Early exit: a word whose active set emptied is never walked again.  A
// wave that still holds a live word after tile i stores i + 1 into the
// vote word before the barrier; a thread that then reads less than i + 1
// knows that nobody can score any more and leaves - walk and loads end
// together (one tile was loaded ahead).  The word only ever grows and live
// words only ever die, so a wave already in step i + 1 can only have
// written what keeps a slower thread in the loop, and nothing is reset.
//
// The walk takes a tile 64 keys at a time per word: one LDS read per tier
// with a key in every lane, then 64 steps fed through readlane
// (score_walk_lane).  A step per LDS round trip, which is what
// score_walk_step over LDS costs, measured slower than k_score_from_masks'
// scalar loads (profiles/r15_masks_topk.md).
//
// Scores are bit-identical to cpu_score_from_masks': score_walk_step's
// arithmetic per pod in key order.  Epilogue: tiled_finish<WPW>(TopkOut), the exchange
// area over buffer 0 behind the last barrier.
// score_walk_step for key j of a chunk whose tier words sit one key per
// lane in m[]: the same cur / wmax / score arithmetic in the same tier
// order, the words taken from lane j (wave-uniform) instead of from memory.
DEV int score_walk_lane(const unsigned long long (&m)[MAX_TIERS], int j,
                        int n_tiers, const float (&wt)[MAX_TIERS], int lane,
                        bool first, int& active, float& score) {
  int cur = 0;
  float wmax = 0.f;
#pragma unroll
  for (int t = 0; t < MAX_TIERS; ++t) {
    if (t < n_tiers) {
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)m[t], j);
      const uint32_t hi =
          (uint32_t)__builtin_amdgcn_readlane((int)(m[t] >> 32), j);
      if (((((uint64_t)hi << 32) | lo) >> lane) & 1) {
        cur = 1;
        wmax = fmaxf(wmax, wt[t]);
      }
    }
  }
  const int act = first ? cur : (active & cur);
  active = act;
  if (act) score += wmax;
  return act;
}

template <bool V16>
struct MaskVec {
  using type = unsigned long long;
  static constexpr int NV = 16, WORDS = 1;
};
// a native vector, not ulonglong2: the struct wrapper keeps stage[] out of
// registers (the array went to scratch with it)
typedef unsigned long long mask_u64x2 __attribute__((ext_vector_type(2)));
template <>
struct MaskVec<true> {
  using type = mask_u64x2;
  static constexpr int NV = 8, WORDS = 2;
};
// Host and device agree on what a thread can stage: NV vectors.
template <bool V16>
constexpr int mask_tile_max_words() {
  return MaskVec<V16>::NV * MaskVec<V16>::WORDS * 256;
}

template <int WPW, bool V16>
__global__ void __launch_bounds__(256) k_topk_from_masks(
    const unsigned long long* __restrict__ masks,  // [Ktot, T, W]
    const int32_t* __restrict__ offsets,           // [B+1]
    int Ktot, const float* __restrict__ weights, int T, int num_pods, int W,
    int KT, TopkOut out) {
  using Vec = typename MaskVec<V16>::type;
  constexpr int NV = MaskVec<V16>::NV;
  // 2 x [KT, T, W], vote; aligned for the 16-byte tile stores
  extern __shared__ __attribute__((aligned(16))) unsigned long long
      lds_mask_tiles[];
  unsigned long long* const lds_masks = lds_mask_tiles;
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int TW = T * W;
  const int tile_words = KT * TW;
  volatile int* vote = reinterpret_cast<int*>(lds_masks + 2 * tile_words);
  // offsets the caller got wrong shorten the span; they never leave masks
  const int k_lo = min(max(offsets[b], 0), Ktot);
  const int K = max(min(offsets[b + 1], Ktot) - k_lo, 0);
  const int n_tiles = (K + KT - 1) / KT;
  const unsigned long long* span = masks + (size_t)k_lo * TW;

  float score[WPW];
  int active[WPW];
  unsigned live = 0;  // bit j: word wave + 4 j can still score
#pragma unroll
  for (int j = 0; j < WPW; ++j) {
    score[j] = 0.f;
    active[j] = 0;
    if (wave + 4 * j < W) live |= 1u << j;
  }

  float wt[MAX_TIERS];
#pragma unroll
  for (int t = 0; t < MAX_TIERS; ++t) wt[t] = t < T ? weights[t] : 0.f;

  Vec stage[NV];
  // vectors of tile i: whole, because a tile is whole keys of TW words
  auto tile_vecs = [&](int i) {
    return min(KT, K - i * KT) * TW / MaskVec<V16>::WORDS;
  };
  auto fetch = [&](int i) {  // global -> registers
    const Vec* src =
        reinterpret_cast<const Vec*>(span + (size_t)i * tile_words);
    const int n = tile_vecs(i);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int x = j * 256 + (int)threadIdx.x;
      if (x < n) stage[j] = src[x];
    }
  };
  auto park = [&](int i) {  // registers -> buffer i & 1
    Vec* dst = reinterpret_cast<Vec*>(lds_masks + (i & 1) * tile_words);
    const int n = tile_vecs(i);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int x = j * 256 + (int)threadIdx.x;
      if (x < n) dst[x] = stage[j];
    }
  };

  if (threadIdx.x == 0) *vote = 0;
  if (n_tiles > 0) {
    fetch(0);
    park(0);
  }
  __syncthreads();
  for (int i = 0; i < n_tiles; ++i) {
    const bool more = i + 1 < n_tiles;
    if (more) fetch(i + 1);
    const int k0 = i * KT;
    const int len = min(KT, K - k0);
    const unsigned long long* cbuf = lds_masks + (i & 1) * tile_words;
#pragma unroll
    for (int jw = 0; jw < WPW; ++jw) {
      if (!((live >> jw) & 1)) continue;  // past W, or its set is empty
      const unsigned long long* col = cbuf + wave + 4 * jw;
      // 64 keys at a time: lane j reads key c0 + j's tier words, one LDS
      // round trip for the chunk; step j then takes them from lane j
      // through scalar registers, so no memory latency sits between two
      // steps of the walk
      for (int c0 = 0; c0 < len && ((live >> jw) & 1); c0 += 64) {
        const int n = min(64, len - c0);
        unsigned long long mine[MAX_TIERS];
#pragma unroll
        for (int t = 0; t < MAX_TIERS; ++t)
          mine[t] = (t < T && lane < n)
                        ? col[(size_t)(c0 + lane) * TW + t * W]
                        : 0ull;
        for (int j = 0; j < n; ++j) {
          const int act = score_walk_lane(mine, j, T, wt, lane,
                                          k0 + c0 + j == 0, active[jw],
                                          score[jw]);
          if (!__any(act)) {
            live &= ~(1u << jw);
            break;
          }
        }
      }
    }
    if (live && lane == 0) *vote = i + 1;
    if (more) park(i + 1);
    __syncthreads();
    if (*vote < i + 1) break;
  }

  tiled_finish<WPW>(out, b, score, W, num_pods, lds_masks);
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

// ---------------------------------------------------------------------
// The ragged (wave-tiled) device chain: stage and chain over one token
// image PER WAVE of 64 prompts (kvidx_ops.h plan_ragged_waves), hashes out
// in CSR form.  The prompts are sorted by length, so the 64 of a wave are
// neighbours in length: wave g's image int32 [wave_k[g] * BS][64] is only
// as tall as its own longest prompt, its chain loop runs wave_k[g] times,
// and memory is ~4 B per token + 8 B per chunk whatever the batch's length
// distribution.  The padded kernels above pay max_k of the whole batch for
// every wave.
// ---------------------------------------------------------------------

// Wave of staging tile `tile`: the g with tile_start[g] <= tile <
// tile_start[g + 1].  tile is uniform over the workgroup, so the steps are
// scalar loads and branches (as dev_group_of_event for one event).
DEV int dev_wave_of_tile(const int32_t* __restrict__ tile_start, int G,
                         int tile) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_start[mid] <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// k_stage_ragged_tokens' tile transposition (same LDS tile, same
// unconditional clamped loads) over the per-wave images.  1-D grid, one
// workgroup per 64-position tile of one wave: tile rows are the wave's 64
// prompts perm[64 g ..], -1 a row of zeros; output row t of wave g is the
// one 256 B line at img + img_off[g] + 64 t.  Every slot of every image is
// written, a zero at and past a prompt's last whole chunk.
template <typename TokT>
__global__ void __launch_bounds__(256) k_stage_ragged_waves(
    const TokT* __restrict__ flat,            // [total]
    const int32_t* __restrict__ tok_off,      // [B+1]
    const int32_t* __restrict__ n_chunks,     // [B]
    const int32_t* __restrict__ perm,         // [64 G]
    const int32_t* __restrict__ wave_k,       // [G]
    const int64_t* __restrict__ img_off,      // [G+1]
    const int32_t* __restrict__ tile_start,   // [G+1]
    int G, int block_size,
    int32_t* __restrict__ img) {
  __shared__ int32_t tile[STAGE_TILE][STAGE_TILE + 1];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = dev_wave_of_tile(tile_start, G, (int)blockIdx.x);
  const int64_t t0 = (int64_t)((int)blockIdx.x - tile_start[g]) * STAGE_TILE;
  const int64_t T = (int64_t)wave_k[g] * block_size;  // rows of this image
  const int32_t* rows = perm + (int64_t)g * 64;
  constexpr int ROWS = STAGE_TILE / 4;  // tile rows per wave
  const int64_t pos = t0 + lane;
  int32_t x[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int p = rows[wave + 4 * i];  // scalar: one prompt per wave and step
    const int pc = max(p, 0);
    const int64_t keep = (int64_t)n_chunks[pc] * block_size;
    const int64_t first = tok_off[pc];
    const bool ok = p >= 0 && pos < keep;
    // token 0 exists: a planned wave has a prompt with a whole chunk
    const int32_t v = (int32_t)flat[ok ? first + pos : 0];
    x[i] = ok ? v : 0;
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) tile[wave + 4 * i][lane] = x[i];
  __syncthreads();
  int32_t* out = img + img_off[g];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = wave + 4 * i;
    if (t0 + r < T) out[(t0 + r) * 64 + lane] = tile[lane][r];
  }
}

// chain_flush_rows for CSR output: row r of the wave is prompt perm[..+r],
// whose chunks go to out[h_off + c], c < its n_chunks.  The flushing lane
// gets both from lane r by shuffle.  CSR has no padding - the slot after a
// prompt's last chunk is the next prompt's first - so only chunks below
// n_chunks are stored, and a 16-byte store is taken only for a whole pair
// whose destination is 16-byte aligned (an even row start; odd rows keep
// 8-byte stores).  ho / mc: this lane's own h_off and n_chunks (0 chunks
// for a lane without a prompt).
DEV void chain_flush_csr(const uint64_t* stage, uint64_t* __restrict__ out,
                         int ho, int mc, int wl, int c) {
  const int cc = c & (CHAIN_STAGE_CHUNKS - 1);
  const int c0 = c - cc;
  const bool base16 = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const int part2 = 2 * (wl & 7);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const int r = g * 8 + (wl >> 3);
    const int ho_r = __shfl(ho, r, 64);
    const int mc_r = __shfl(mc, r, 64);
    const uint64_t* s = stage + r * CHAIN_STAGE_ROW + part2;
    const uint64_t v0 = s[0];
    const uint64_t v1 = s[1];
    // chunks c0 + part2, + 1 of row r; what is staged ends at c <= its
    // wave's last chunk, so "below mc_r" implies "staged"
    const int n = min(mc_r - (c0 + part2), 2);
    if (n > 0) {
      uint64_t* o = out + (int64_t)ho_r + c0 + part2;
      if (n == 2 && base16 && (ho_r & 1) == 0) {
        *reinterpret_cast<u64x2*>(o) = u64x2{v0, v1};  // dwordx4
      } else {
        o[0] = v0;
        if (n == 2) o[1] = v1;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Chain root policies of the four wave chain kernels: where lane l's chain
// starts.  Each kernel is one body under two __global__ entries, as
// fused_score_body is under its epilogues.  root(p, mc) is called once per
// lane in the prologue, with the lane's row p of the plan (-1: none) and
// its chunk count, and is over before the chunk loop, so the loop is the
// same convergent one under either policy.
//
// RootInit: one constant for the whole batch - the read path, where every
// prompt hashes from the chain root.
struct RootInit {
  uint64_t init;
  DEV uint64_t operator()(int, int) const { return init; }
};

// RootEvents: the rows are events, and event e starts from the request key
// its parent engine hash maps to in the engine map (dev_event_parent), else
// from init.  One divergent probe per chain: no launch and no roots buffer
// of its own.  Lanes without a chunk do not probe.  An engine-map value may
// be below 2^32; the FNV bodies' `wide` vote sees it from chunk 0 on, since
// it votes on h before every chunk.
struct RootEvents {
  Table v;
  const uint64_t* __restrict__ parents;    // [E]
  const uint8_t* __restrict__ has_parent;  // [E]
  const int32_t* __restrict__ model_of;    // [E]
  uint64_t init;
  DEV uint64_t operator()(int e, int mc) const {
    if (mc <= 0) return init;
    return dev_event_parent(v, has_parent, parents, model_of, e, init);
  }
};

// RootLinked: RootEvents for bursts whose events chain from each other.
// The host (plan_event_links) has resolved every batch-local parent to
// link[e], the index in req_scratch of the parent block's request key, and
// ordered the launches by level, so a linked lane's root is one load and no
// lane waits for another workgroup.  link[e] < 0: the engine map, as
// RootEvents.  A lane without chunks loads nothing.
// scratch is the kernels' own `out` (req_scratch).  The slot a lane reads
// here belongs to an event one level below: an EARLIER launch on the same
// stream wrote it, and this launch, which holds one level's waves only,
// never writes it.  So nothing reachable through `out` is both written and
// read in one launch, and the __restrict__ on `out` still holds.
// A linked root, like an engine-map value, may be below 2^32; the `wide`
// vote covers it in the same way.
struct RootLinked {
  RootEvents ev;
  const int32_t* __restrict__ link;  // [E]
  const uint64_t* scratch;           // [n_hashes]
  DEV uint64_t operator()(int e, int mc) const {
    if (mc <= 0) return ev.init;
    const int bi = link[e];
    return bi >= 0 ? scratch[bi] : ev(e, mc);
  }
};

// k_fnv_chain_tr's chunk body over wave g's own image, wave_k[g] trips.
// One-wave workgroups, block g = wave wave0 + g (wave0: 0 except under the
// per-level launches of the _lk entries): the longest waves are dispatched
// first.  Lane l is prompt perm[64 g + l]; -1 is a chain of no chunks.
// out: CSR, chunk c of prompt p at out[h_off[p] + c]; nothing outside
// [0, total_chunks) is written.
template <int BS, typename Root>
DEV void fnv_chain_waves_body(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    int wave0, Root root, uint64_t* __restrict__ out) {
  __shared__ uint64_t stage[64 * CHAIN_STAGE_ROW];
  const int g = wave0 + (int)blockIdx.x;
  const int wl = threadIdx.x;
  const int p = perm[(int64_t)g * 64 + wl];
  const int pc = max(p, 0);
  const int mc = p >= 0 ? n_chunks[pc] : 0;
  const int ho = h_off[pc];
  const int K = __builtin_amdgcn_readfirstlane(wave_k[g]);
  const int32_t* tokens_t = img + img_off[g] + wl;
  uint64_t h = root(p, mc);
  for (int c = 0; c < K; ++c) {
    uint32_t tok[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j)
      tok[j] = (uint32_t)tokens_t[(int64_t)(c * BS + j) * 64];
    const bool active = c < mc;
    const bool wide = __all(!active || h > 0xFFFFFFFFull);
    const uint64_t h2 = chunk_hash_fast(h, tok, BS, wide);
    h = active ? h2 : h;
    const int cc = c & (CHAIN_STAGE_CHUNKS - 1);
    stage[wl * CHAIN_STAGE_ROW + cc] = h;  // read back only where c < mc
    if (cc == CHAIN_STAGE_CHUNKS - 1 || c == K - 1)
      chain_flush_csr(stage, out, ho, mc, wl, c);
  }
}

template <int BS>
__global__ void __launch_bounds__(64) k_fnv_chain_waves(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    uint64_t init, uint64_t* __restrict__ out) {
  fnv_chain_waves_body<BS>(img, img_off, perm, wave_k, n_chunks, h_off, 0,
                           RootInit{init}, out);
}

// The ingest entry: rows are events, h_off is the events' eh_off and out
// is req_scratch, of which only the chunks of kept stores are written.
template <int BS>
__global__ void __launch_bounds__(64) k_fnv_chain_waves_ev(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    RootEvents roots, uint64_t* __restrict__ out) {
  fnv_chain_waves_body<BS>(img, img_off, perm, wave_k, n_chunks, h_off, 0,
                           roots, out);
}

// The linked ingest entry: one level's waves [wave0, wave1) of a linked
// plan, launched level by level (launch_wave_chain).  Grid: wave1 - wave0.
template <int BS>
__global__ void __launch_bounds__(64) k_fnv_chain_waves_lk(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    int wave0, int wave1, RootLinked roots, uint64_t* __restrict__ out) {
  if (wave0 + (int)blockIdx.x >= wave1) return;  // the whole one-wave group
  fnv_chain_waves_body<BS>(img, img_off, perm, wave_k, n_chunks, h_off, wave0,
                           roots, out);
}

// k_sha_chain_tr over the per-wave images: wave_k[g] as the loop bound,
// CSR stores of active chunks only, no zero-fill tail.  The waves of a
// workgroup have different trip counts, which is safe: nothing in
// chunk_hash_sha256_wave is a workgroup barrier (each lane packs into its
// own LDS column, the votes are wave-wide), and neither is anything here.
template <int BS, int ALGO, typename Root>
DEV void sha_chain_waves_body(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    int wave0, int G, Root root, uint64_t* __restrict__ out) {
  constexpr int NT = sha_tr_threads(BS);
  __shared__ uint32_t sha_words[sha_tr_words(BS) * NT];
  const int wl = threadIdx.x & 63;
  // the launch's waves are [wave0, G), NT / 64 of them per workgroup
  const int g = __builtin_amdgcn_readfirstlane(
      wave0 + (int)blockIdx.x * (NT / 64) + (int)(threadIdx.x >> 6));
  if (g >= G) return;  // a whole wave, and no barrier follows
  const int p = perm[(int64_t)g * 64 + wl];
  const int pc = max(p, 0);
  const int mc = p >= 0 ? n_chunks[pc] : 0;
  uint64_t* o = out + h_off[pc];
  const int K = __builtin_amdgcn_readfirstlane(wave_k[g]);
  const int32_t* tokens_t = img + img_off[g] + wl;
  ShaLdsCol<NT> col{sha_words + threadIdx.x};
  uint64_t h = root(p, mc);
  for (int c = 0; c < K; ++c) {
    const bool active = c < mc;
    uint32_t tok[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j)
      tok[j] = (uint32_t)tokens_t[(int64_t)(c * BS + j) * 64];
    const uint64_t h2 = chunk_hash_sha256_wave(
        h, tok, BS, sha_digest_word(ALGO), col, active, ShaWaveAny{});
    h = active ? h2 : h;
    if (active) o[c] = h;
  }
}

template <int BS, int ALGO>
__global__ void k_sha_chain_waves(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    int G, uint64_t init, uint64_t* __restrict__ out) {
  sha_chain_waves_body<BS, ALGO>(img, img_off, perm, wave_k, n_chunks, h_off,
                                 0, G, RootInit{init}, out);
}

template <int BS, int ALGO>
__global__ void k_sha_chain_waves_ev(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    int G, RootEvents roots, uint64_t* __restrict__ out) {
  sha_chain_waves_body<BS, ALGO>(img, img_off, perm, wave_k, n_chunks, h_off,
                                 0, G, roots, out);
}

// One level's waves [wave0, wave1): wave1 is the bound G is above.  Grid:
// ceil((wave1 - wave0) / (NT / 64)).
template <int BS, int ALGO>
__global__ void k_sha_chain_waves_lk(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    int wave0, int wave1, RootLinked roots, uint64_t* __restrict__ out) {
  sha_chain_waves_body<BS, ALGO>(img, img_off, perm, wave_k, n_chunks, h_off,
                                 wave0, wave1, roots, out);
}

// ---------------------------------------------------------------------
// The stream chain kernels: the ragged chain for ANY block size 1..65535.
// The templated kernels above hold a chunk's tokens in tok[BS], so their
// registers (FNV) and LDS columns (SHA) grow with the block size and stop
// at 64.  These take block_size at run time and pass the tokens through a
// fixed window: same work split (lane = prompt perm[64 g + l], wave_k[g]
// trips over wave g's own image), same CSR output, footprint independent
// of the block size.  block_size is a kernel argument, uniform over the
// grid: everything derived from it is scalar, every branch on it a scalar
// branch.
// ---------------------------------------------------------------------

// FNV-64a.  A chunk is chunk_hash_begin, block_size / 16 trips of a rolled
// loop over groups of CHAIN_GROUP positions - 16 unconditional loads of one
// 256 B line each into a statically indexed tok[16], then 16 unrolled
// steps - one group of block_size % 16, chunk_hash_end.  The image is
// position-major, so the walk over a wave's rows is one running pointer
// from the first chunk to the last.
template <typename Root>
DEV void fnv_chain_stream_body(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    int wave0, Root root, int block_size, uint64_t* __restrict__ out) {
  __shared__ uint64_t stage[64 * CHAIN_STAGE_ROW];
  const int g = wave0 + (int)blockIdx.x;
  const int wl = threadIdx.x;
  const int p = perm[(int64_t)g * 64 + wl];
  const int pc = max(p, 0);
  const int mc = p >= 0 ? n_chunks[pc] : 0;
  const int ho = h_off[pc];
  const int K = __builtin_amdgcn_readfirstlane(wave_k[g]);
  const ChainShape s = chain_shape(block_size);
  const int32_t* t = img + img_off[g] + wl;  // rows [0, K * block_size)
  uint64_t h = root(p, mc);
  for (int c = 0; c < K; ++c) {
    const bool active = c < mc;
    const bool wide = __all(!active || h > 0xFFFFFFFFull);
    uint64_t h2 = chunk_hash_begin(h, wide, s);
#pragma unroll 1
    for (int gi = 0; gi < s.groups; ++gi, t += CHAIN_GROUP * 64) {
      uint32_t tok[CHAIN_GROUP];
#pragma unroll
      for (int j = 0; j < CHAIN_GROUP; ++j) tok[j] = (uint32_t)t[j * 64];
      h2 = chunk_hash_group(h2, tok);
    }
    if (s.tail) {
      uint32_t tok[CHAIN_GROUP];
#pragma unroll
      for (int j = 0; j < CHAIN_GROUP; ++j)  // rows past the chunk: not read
        tok[j] = j < s.tail ? (uint32_t)t[j * 64] : 0u;
      t += s.tail * 64;
      h2 = chunk_hash_group(h2, tok, s.tail);
    }
    h2 = chunk_hash_end(h2);
    h = active ? h2 : h;
    const int cc = c & (CHAIN_STAGE_CHUNKS - 1);
    stage[wl * CHAIN_STAGE_ROW + cc] = h;  // read back only where c < mc
    if (cc == CHAIN_STAGE_CHUNKS - 1 || c == K - 1)
      chain_flush_csr(stage, out, ho, mc, wl, c);
  }
}

__global__ void __launch_bounds__(64) k_fnv_chain_stream(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    uint64_t init, int block_size, uint64_t* __restrict__ out) {
  fnv_chain_stream_body(img, img_off, perm, wave_k, n_chunks, h_off, 0,
                        RootInit{init}, block_size, out);
}

__global__ void __launch_bounds__(64) k_fnv_chain_stream_ev(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    RootEvents roots, int block_size, uint64_t* __restrict__ out) {
  fnv_chain_stream_body(img, img_off, perm, wave_k, n_chunks, h_off, 0, roots,
                        block_size, out);
}

__global__ void __launch_bounds__(64) k_fnv_chain_stream_lk(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    int wave0, int wave1, RootLinked roots, int block_size,
    uint64_t* __restrict__ out) {
  if (wave0 + (int)blockIdx.x >= wave1) return;  // the whole one-wave group
  fnv_chain_stream_body(img, img_off, perm, wave_k, n_chunks, h_off, wave0,
                        roots, block_size, out);
}

// SHA-256 over the same payload: chunk_hash_sha256_seg, SHA_SEG_TOKENS
// tokens at a time through a column of sha_seg_words() words per lane
// (28 KB for the wave, whatever the block size).  A segment's tokens are
// loaded in one go - unconditionally for a whole segment, under scalar
// branches for the last one - so one memory latency is paid per segment,
// under which sit up to five compressions.  One-wave workgroups as the FNV
// kernel: there is no workgroup barrier here or in the driver, and a wave
// with fewer trips holds no other wave's LDS.
template <int ALGO, typename Root>
DEV void sha_chain_stream_body(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    int wave0, Root root, int block_size, uint64_t* __restrict__ out) {
  constexpr int SEG = SHA_SEG_TOKENS;
  __shared__ uint32_t sha_words[sha_seg_words(SEG) * 64];
  const int g = wave0 + (int)blockIdx.x;
  const int wl = threadIdx.x;
  const int p = perm[(int64_t)g * 64 + wl];
  const int pc = max(p, 0);
  const int mc = p >= 0 ? n_chunks[pc] : 0;
  uint64_t* o = out + h_off[pc];
  const int K = __builtin_amdgcn_readfirstlane(wave_k[g]);
  const int32_t* chunk = img + img_off[g] + wl;  // rows [0, K * block_size)
  ShaLdsCol<64> col{sha_words + wl};
  uint64_t h = root(p, mc);
  for (int c = 0; c < K; ++c, chunk += (int64_t)block_size * 64) {
    const bool active = c < mc;
    auto load = [chunk](int first, int cnt, uint32_t (&tok)[SEG])
                    __attribute__((always_inline)) {
      const int32_t* t = chunk + (int64_t)first * 64;
      if (cnt == SEG) {
#pragma unroll
        for (int j = 0; j < SEG; ++j) tok[j] = (uint32_t)t[j * 64];
      } else {
#pragma unroll
        for (int j = 0; j < SEG; ++j)  // rows past the chunk: not read
          tok[j] = j < cnt ? (uint32_t)t[j * 64] : 0u;
      }
    };
    const uint64_t h2 = chunk_hash_sha256_seg<SEG>(
        h, block_size, load, sha_digest_word(ALGO), col, active, ShaWaveAny{});
    h = active ? h2 : h;
    if (active) o[c] = h;
  }
}

template <int ALGO>
__global__ void __launch_bounds__(64) k_sha_chain_stream(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    uint64_t init, int block_size, uint64_t* __restrict__ out) {
  sha_chain_stream_body<ALGO>(img, img_off, perm, wave_k, n_chunks, h_off, 0,
                              RootInit{init}, block_size, out);
}

template <int ALGO>
__global__ void __launch_bounds__(64) k_sha_chain_stream_ev(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    RootEvents roots, int block_size, uint64_t* __restrict__ out) {
  sha_chain_stream_body<ALGO>(img, img_off, perm, wave_k, n_chunks, h_off, 0,
                              roots, block_size, out);
}

template <int ALGO>
__global__ void __launch_bounds__(64) k_sha_chain_stream_lk(
    const int32_t* __restrict__ img, const int64_t* __restrict__ img_off,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ wave_k,
    const int32_t* __restrict__ n_chunks, const int32_t* __restrict__ h_off,
    int wave0, int wave1, RootLinked roots, int block_size,
    uint64_t* __restrict__ out) {
  if (wave0 + (int)blockIdx.x >= wave1) return;  // the whole one-wave group
  sha_chain_stream_body<ALGO>(img, img_off, perm, wave_k, n_chunks, h_off,
                              wave0, roots, block_size, out);
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

// What the three table sweeps launch with, after the checks they share:
// min(tiles, SWEEP_MAX_BLOCKS, max_grid) workgroups, at least one, and an
// unfilled int32 partials [grid, cols] for their counters.
struct SweepLaunch {
  int64_t n_tiles, grid;
  at::Tensor partials;
};
static SweepLaunch plan_sweep(KVIDX_TABLE_PARAMS, const Table& v, int64_t cols,
                              int64_t max_grid = SWEEP_MAX_BLOCKS) {
  TORCH_CHECK(pods_per_key >= 1 && pods_per_key <= 4096,
              "pods_per_key out of range");
  TORCH_CHECK(pods.numel() == keys.numel() * pods_per_key,
              "pods must hold capacity * pods_per_key entries");
  TORCH_CHECK(meta.device() == keys.device() &&
                  pods.device() == keys.device() &&
                  e_meta.device() == keys.device(),
              "table tensors must share one device");
  // tiles are read as 16-byte vectors from the start of the array
  TORCH_CHECK(reinterpret_cast<uintptr_t>(v.pods) % 16 == 0,
              "pods storage must be 16-byte aligned");
  const int64_t n_tiles = (keys.numel() + SWEEP_ROWS - 1) / SWEEP_ROWS;
  const int64_t grid = std::max<int64_t>(
      1, std::min<int64_t>({n_tiles, (int64_t)SWEEP_MAX_BLOCKS, max_grid}));
  return {n_tiles, grid,
          at::empty({grid, cols}, keys.options().dtype(at::kInt))};
}

// The column sums of partials [grid, N], read back: the sweep's host wait.
template <int N>
static std::vector<int64_t> sum_partials(const at::Tensor& partials) {
  auto host = partials.cpu();
  const uint32_t* hp = u32p(host);
  std::vector<int64_t> sums(N, 0);
  for (int64_t b = 0; b < host.size(0); ++b)
    for (int i = 0; i < N; ++i) sums[i] += hp[N * b + i];
  return sums;
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

// What a fused launch is shaped by, after the checks every fused op shares.
struct FusedGeom {
  int64_t W, n_tiers;
  size_t lds;  // the masks
};
static FusedGeom fused_geom_checked(int64_t num_pods, int64_t max_k,
                                    int64_t n_tiers) {
  int64_t W = pod_words(num_pods);
  TORCH_CHECK(W <= 16, "fused score supports up to 1024 pods");
  n_tiers = clamp_tiers(n_tiers);
  TORCH_CHECK(fused_score_fits(max_k, n_tiers, W),
              "fused score LDS overflow: reduce keys per prompt or pods");
  return {W, n_tiers, fused_score_lds_bytes(max_k, n_tiers, W)};
}

// One workgroup per prompt, B >= 1.  out: the kernel's last argument;
// where...: the kernel arguments between the hashes and the model id,
// which say where prompt b's keys lie.
template <typename Kern, typename Out, typename... Where>
static void launch_fused(Kern kernel, const Table& v, int64_t B,
                         const FusedGeom& g, size_t lds_bytes,
                         const at::Tensor& hashes, int64_t model_id,
                         const at::Tensor& filter_words,
                         const at::Tensor& weights, int64_t num_pods,
                         int64_t epoch, Out out, Where... where) {
  const uint64_t* filter = filter_ptr(filter_words);
  hipLaunchKernelGGL(kernel, dim3((int)B), dim3(256), lds_bytes, STREAM, v,
                     (const uint64_t*)u64p(hashes), where...,
                     (uint32_t)model_id, filter, filter ? 1 : 0,
                     weights.data_ptr<float>(), (int)num_pods, (int)g.W,
                     (int32_t)epoch, (int)g.n_tiers, out);
}

template <typename Kern, typename... Where>
static at::Tensor launch_fused_score(Kern kernel, const Table& v, int64_t B,
                                     const at::Tensor& hashes,
                                     int64_t model_id,
                                     const at::Tensor& filter_words,
                                     const at::Tensor& weights,
                                     int64_t num_pods, int64_t epoch,
                                     int64_t max_k, int64_t n_tiers,
                                     Where... where) {
  const FusedGeom g = fused_geom_checked(num_pods, max_k, n_tiers);
  auto scores = at::zeros({B, num_pods}, hashes.options().dtype(at::kFloat));
  if (B == 0) return scores;
  launch_fused(kernel, v, B, g, g.lds, hashes, model_id, filter_words, weights,
               num_pods, epoch, scores.data_ptr<float>(), where...);
  return scores;
}

// {ids int32 [B, top_n], scores float32 [B, top_n]} beside `like`, not
// filled: the top-n kernels write every slot.
static constexpr size_t TOPK_XCH_BYTES = 4 * MAX_TOPK * sizeof(uint64_t);
static std::vector<at::Tensor> topk_alloc(const at::Tensor& like, int64_t B,
                                          int64_t top_n) {
  return {at::empty({B, top_n}, like.options().dtype(at::kInt)),
          at::empty({B, top_n}, like.options().dtype(at::kFloat))};
}
static TopkOut topk_out(const std::vector<at::Tensor>& r, int64_t top_n) {
  return {r[0].data_ptr<int32_t>(), r[1].data_ptr<float>(), (int)top_n};
}

// launch_fused_score for the top-n entries: the same checks, no fill, and
// dynamic LDS of at least the exchange area (one key, one tier, 64 pods
// are 8 bytes of masks).
template <typename Kern, typename... Where>
static std::vector<at::Tensor> launch_fused_topk(
    Kern kernel, const Table& v, int64_t B, const at::Tensor& hashes,
    int64_t model_id, const at::Tensor& filter_words,
    const at::Tensor& weights, int64_t num_pods, int64_t epoch, int64_t max_k,
    int64_t n_tiers, int64_t top_n, Where... where) {
  TORCH_CHECK(top_n >= 1 && top_n <= MAX_TOPK, "top_n must be 1..", MAX_TOPK);
  const FusedGeom g = fused_geom_checked(num_pods, max_k, n_tiers);
  auto r = topk_alloc(hashes, B, top_n);
  if (B == 0) return r;
  launch_fused(kernel, v, B, g, std::max(g.lds, TOPK_XCH_BYTES), hashes,
               model_id, filter_words, weights, num_pods, epoch,
               topk_out(r, top_n), where...);
  return r;
}

// ---- tiled fused score: the launch ---------------------------------------
// Keys per tile for (n_tiers, W): two buffers of KT keys and the two vote
// words stay within the 64 KB of dynamic LDS a launch gets without a
// function attribute.  Up to 256 keys (one probe per thread and tile);
// past 32 KB a workgroup gives LDS back for residency (four workgroups per
// CU keep more probes in flight than two with longer tiles), down to 16
// keys, below which a tile is mostly barriers.
static constexpr int64_t TILED_VOTE_BYTES = 2 * sizeof(int);
int64_t tiled_score_tile_keys(int64_t n_tiers, int64_t W) {
  const int64_t key_bytes = clamp_tiers(n_tiers) * W * sizeof(uint64_t);
  TORCH_CHECK(W >= 1 && W <= MAX_PODS / 64, "W must be 1..", MAX_PODS / 64);
  const int64_t fit = (64 * 1024 - TILED_VOTE_BYTES) / (2 * key_bytes);
  const int64_t kt = std::max<int64_t>(16, 32 * 1024 / (2 * key_bytes));
  return std::min<int64_t>({256, kt, fit});
}

// What a tiled launch is shaped by, after the checks every tiled op shares.
struct TiledGeom {
  int64_t W, n_tiers, KT;
  size_t lds;  // both buffers and the vote words
};
static TiledGeom tiled_geom_checked(int64_t num_pods, int64_t max_k,
                                    int64_t n_tiers) {
  TORCH_CHECK(num_pods >= 1 && num_pods <= MAX_PODS, "num_pods must be 1..",
              MAX_PODS);
  TORCH_CHECK(max_k >= 0, "max_k must not be negative");
  const int64_t W = pod_words(num_pods);
  n_tiers = clamp_tiers(n_tiers);
  const int64_t KT = tiled_score_tile_keys(n_tiers, W);
  const size_t buf = (size_t)KT * n_tiers * W * sizeof(uint64_t);
  // the top-n exchange area overlays one buffer
  TORCH_CHECK(buf >= TOPK_XCH_BYTES &&
                  2 * buf + TILED_VOTE_BYTES <= (size_t)64 * 1024,
              "tiled score tile out of range");
  return {W, n_tiers, KT, 2 * buf + TILED_VOTE_BYTES};
}

// Runs f(std::integral_constant<int, WPW>) for the smallest instantiated
// words-per-wave bound that covers W <= 64.
template <typename F>
static void dispatch_tiled_wpw(int64_t W, F&& f) {
  const int64_t wpw = (W + 3) / 4;
  if (wpw <= 1) f(std::integral_constant<int, 1>{});
  else if (wpw <= 2) f(std::integral_constant<int, 2>{});
  else if (wpw <= 4) f(std::integral_constant<int, 4>{});
  else if (wpw <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

// One workgroup per prompt, B >= 1: launch_fused with the tile length in
// front of `out`.
template <typename Kern, typename Out, typename... Where>
static void launch_tiled(Kern kernel, const Table& v, int64_t B,
                         const TiledGeom& g, const at::Tensor& hashes,
                         int64_t model_id, const at::Tensor& filter_words,
                         const at::Tensor& weights, int64_t num_pods,
                         int64_t epoch, Out out, Where... where) {
  const uint64_t* filter = filter_ptr(filter_words);
  hipLaunchKernelGGL(kernel, dim3((int)B), dim3(256), g.lds, STREAM, v,
                     (const uint64_t*)u64p(hashes), where...,
                     (uint32_t)model_id, filter, filter ? 1 : 0,
                     weights.data_ptr<float>(), (int)num_pods, (int)g.W,
                     (int32_t)epoch, (int)g.n_tiers, (int)g.KT, out);
}

// The two tiled ops of each output kind.  Entry: a generic lambda from WPW
// to the __global__ instantiation (flat or rows).
template <typename Entry, typename... Where>
static at::Tensor launch_tiled_score(Entry entry, const Table& v, int64_t B,
                                     const at::Tensor& hashes,
                                     int64_t model_id,
                                     const at::Tensor& filter_words,
                                     const at::Tensor& weights,
                                     int64_t num_pods, int64_t epoch,
                                     int64_t max_k, int64_t n_tiers,
                                     Where... where) {
  const TiledGeom g = tiled_geom_checked(num_pods, max_k, n_tiers);
  // the kernel writes every column of every row
  auto scores = at::empty({B, num_pods}, hashes.options().dtype(at::kFloat));
  if (B == 0) return scores;
  dispatch_tiled_wpw(g.W, [&](auto N) {
    launch_tiled(entry(N), v, B, g, hashes, model_id, filter_words, weights,
                 num_pods, epoch, scores.data_ptr<float>(), where...);
  });
  return scores;
}

template <typename Entry, typename... Where>
static std::vector<at::Tensor> launch_tiled_topk(
    Entry entry, const Table& v, int64_t B, const at::Tensor& hashes,
    int64_t model_id, const at::Tensor& filter_words,
    const at::Tensor& weights, int64_t num_pods, int64_t epoch, int64_t max_k,
    int64_t n_tiers, int64_t top_n, Where... where) {
  TORCH_CHECK(top_n >= 1 && top_n <= MAX_TOPK, "top_n must be 1..", MAX_TOPK);
  const TiledGeom g = tiled_geom_checked(num_pods, max_k, n_tiers);
  auto r = topk_alloc(hashes, B, top_n);
  if (B == 0) return r;
  dispatch_tiled_wpw(g.W, [&](auto N) {
    launch_tiled(entry(N), v, B, g, hashes, model_id, filter_words, weights,
                 num_pods, epoch, topk_out(r, top_n), where...);
  });
  return r;
}

// The padded rows of the *_rows ops: hashes int64 [B, stride], n_keys
// int32 [B], both on the device.
static void check_padded_rows(const at::Tensor& hashes,
                              const at::Tensor& n_keys, int64_t max_k) {
  TORCH_CHECK(hashes.is_cuda() && hashes.dtype() == at::kLong &&
                  hashes.dim() == 2 && hashes.is_contiguous(),
              "hashes must be a contiguous int64 [B, stride] device tensor");
  TORCH_CHECK(n_keys.is_cuda() && n_keys.dtype() == at::kInt &&
                  n_keys.is_contiguous(),
              "n_keys must be a contiguous int32 device tensor");
  TORCH_CHECK(n_keys.numel() == hashes.size(0),
              "n_keys must have one entry per row");
  TORCH_CHECK(max_k <= hashes.size(1), "max_k exceeds the row length");
}

// The block sizes the templated chain kernels are built for.
static bool chain_block_size_templated(int64_t block_size) {
  return block_size == 4 || block_size == 8 || block_size == 16 ||
         block_size == 32 || block_size == 64;
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
  const SweepLaunch s = plan_sweep(KVIDX_TABLE_ARGS, v, 2);
  hipLaunchKernelGGL(k_purge_pods, dim3((unsigned)s.grid), dim3(SWEEP_THREADS),
                     0, STREAM, v,
                     reinterpret_cast<const uint32_t*>(u64p(purge_words)),
                     2 * W, (int)model_id, s.n_tiles, u32p(s.partials));
  return sum_partials<2>(s.partials);  // {entries cleared, keys tombstoned}
}

// The purge's launch shape; the map is validated on the host first (one
// small readback of remap), the counters come back after the sweep.
std::vector<int64_t> kvidx::gpu_remap_pods(KVIDX_TABLE_PARAMS,
                                           at::Tensor remap) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  TORCH_CHECK(remap.device() == keys.device(),
              "remap must live on the table's device");
  const int n = remap_checked(remap);
  const SweepLaunch s = plan_sweep(KVIDX_TABLE_ARGS, v, 3);
  hipLaunchKernelGGL(k_remap_pods, dim3((unsigned)s.grid), dim3(SWEEP_THREADS),
                     0, STREAM, v, i32p(remap), n, s.n_tiles,
                     u32p(s.partials));
  return sum_partials<3>(s.partials);  // {moved, cleared, keys tombstoned}
}

// The sweep, the reduce and one readback of bins + 6 int64 words, on the
// current stream.  The grid is capped so that the partials stay within
// CENSUS_PARTIAL_BYTES: 511 workgroups at 16384 bins, which is also what 2
// workgroups of 64 KB LDS per CU come to.
std::vector<at::Tensor> kvidx::gpu_pod_census(KVIDX_TABLE_PARAMS,
                                              int64_t model_id,
                                              int64_t num_pods,
                                              int64_t n_tiers) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  const int64_t bins =
      census_bins_checked(KVIDX_TABLE_ARGS, model_id, num_pods, n_tiers);
  const int64_t cols = bins + CENSUS_SUMMARY_LEN;
  const SweepLaunch s =
      plan_sweep(KVIDX_TABLE_ARGS, v, cols, CENSUS_PARTIAL_BYTES / (4 * cols));
  // a workgroup's uint32 bins and counters cannot wrap
  const int64_t tiles_per_wg = (s.n_tiles + s.grid - 1) / s.grid;
  TORCH_CHECK(tiles_per_wg * SWEEP_ROWS * pods_per_key < (1ll << 32),
              "table too large for 32-bit per-workgroup census counters");
  auto sums = at::empty({cols}, keys.options().dtype(at::kLong));
  hipLaunchKernelGGL(k_pod_census, dim3((unsigned)s.grid), dim3(SWEEP_THREADS),
                     (size_t)bins * sizeof(uint32_t), STREAM, v, (int)model_id,
                     (int)num_pods, (int)n_tiers, s.n_tiles,
                     u32p(s.partials));
  hipLaunchKernelGGL(k_census_reduce,
                     dim3((unsigned)((cols + REDUCE_COLS - 1) / REDUCE_COLS)),
                     dim3(REDUCE_COLS * REDUCE_SLICES), 0, STREAM,
                     u32p(s.partials), (int)s.grid, (int)cols,
                     sums.data_ptr<int64_t>());
  auto err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "pod census launch failed: ",
              hipGetErrorString(err));
  auto host = sums.cpu();  // waits for both kernels
  return {host.narrow(0, 0, bins).view({num_pods, n_tiers}),
          host.narrow(0, bins, CENSUS_SUMMARY_LEN)};
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
  check_padded_rows(hashes, n_keys, max_k);
  return launch_fused_score(k_fused_score_rows, v, hashes.size(0), hashes,
                            model_id, filter_words, weights, num_pods, epoch,
                            max_k, n_tiers, (const int32_t*)i32p(n_keys),
                            hashes.size(1));
}

std::vector<at::Tensor> kvidx::gpu_fused_topk(
    KVIDX_TABLE_PARAMS, at::Tensor hashes, at::Tensor offsets,
    int64_t model_id, at::Tensor filter_words, at::Tensor weights,
    int64_t num_pods, int64_t epoch, int64_t max_k, int64_t n_tiers,
    int64_t top_n) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  return launch_fused_topk(k_fused_topk, v, offsets.numel() - 1, hashes,
                           model_id, filter_words, weights, num_pods, epoch,
                           max_k, n_tiers, top_n,
                           (const int32_t*)i32p(offsets));
}

std::vector<at::Tensor> kvidx::gpu_fused_topk_rows(
    KVIDX_TABLE_PARAMS, at::Tensor hashes, at::Tensor n_keys, int64_t model_id,
    at::Tensor filter_words, at::Tensor weights, int64_t num_pods,
    int64_t epoch, int64_t max_k, int64_t n_tiers, int64_t top_n) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  check_padded_rows(hashes, n_keys, max_k);
  return launch_fused_topk(k_fused_topk_rows, v, hashes.size(0), hashes,
                           model_id, filter_words, weights, num_pods, epoch,
                           max_k, n_tiers, top_n,
                           (const int32_t*)i32p(n_keys), hashes.size(1));
}

// The tiled twins of the four fused ops: the same arguments, any max_k >= 0
// and any fleet up to MAX_PODS, one launch each.
at::Tensor kvidx::gpu_tiled_score(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                  at::Tensor offsets, int64_t model_id,
                                  at::Tensor filter_words, at::Tensor weights,
                                  int64_t num_pods, int64_t epoch,
                                  int64_t max_k, int64_t n_tiers) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  return launch_tiled_score(
      [](auto N) { return k_tiled_score<decltype(N)::value>; }, v,
      offsets.numel() - 1, hashes, model_id, filter_words, weights, num_pods,
      epoch, max_k, n_tiers, (const int32_t*)i32p(offsets));
}

at::Tensor kvidx::gpu_tiled_score_rows(KVIDX_TABLE_PARAMS, at::Tensor hashes,
                                       at::Tensor n_keys, int64_t model_id,
                                       at::Tensor filter_words,
                                       at::Tensor weights, int64_t num_pods,
                                       int64_t epoch, int64_t max_k,
                                       int64_t n_tiers) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  check_padded_rows(hashes, n_keys, max_k);
  return launch_tiled_score(
      [](auto N) { return k_tiled_score_rows<decltype(N)::value>; }, v,
      hashes.size(0), hashes, model_id, filter_words, weights, num_pods, epoch,
      max_k, n_tiers, (const int32_t*)i32p(n_keys), hashes.size(1));
}

std::vector<at::Tensor> kvidx::gpu_tiled_topk(
    KVIDX_TABLE_PARAMS, at::Tensor hashes, at::Tensor offsets,
    int64_t model_id, at::Tensor filter_words, at::Tensor weights,
    int64_t num_pods, int64_t epoch, int64_t max_k, int64_t n_tiers,
    int64_t top_n) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  return launch_tiled_topk(
      [](auto N) { return k_tiled_topk<decltype(N)::value>; }, v,
      offsets.numel() - 1, hashes, model_id, filter_words, weights, num_pods,
      epoch, max_k, n_tiers, top_n, (const int32_t*)i32p(offsets));
}

std::vector<at::Tensor> kvidx::gpu_tiled_topk_rows(
    KVIDX_TABLE_PARAMS, at::Tensor hashes, at::Tensor n_keys, int64_t model_id,
    at::Tensor filter_words, at::Tensor weights, int64_t num_pods,
    int64_t epoch, int64_t max_k, int64_t n_tiers, int64_t top_n) {
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  check_padded_rows(hashes, n_keys, max_k);
  return launch_tiled_topk(
      [](auto N) { return k_tiled_topk_rows<decltype(N)::value>; }, v,
      hashes.size(0), hashes, model_id, filter_words, weights, num_pods, epoch,
      max_k, n_tiers, top_n, (const int32_t*)i32p(n_keys), hashes.size(1));
}

std::vector<at::Tensor> kvidx::gpu_topk_rows(at::Tensor scores,
                                             int64_t top_n) {
  TORCH_CHECK(scores.is_cuda(), "scores must live on the GPU");
  const int64_t P = topk_rows_checked(scores, top_n);
  const int64_t B = scores.size(0);
  TORCH_CHECK(B <= INT32_MAX, "too many rows in one batch");
  auto r = topk_alloc(scores, B, top_n);
  if (B == 0) return r;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(TOPK_ROWS_THREADS), 0,
                       STREAM, (const float*)scores.data_ptr<float>(), (int)P,
                       topk_out(r, top_n));
  };
  // columns per thread: the power of two that covers P
  const int64_t per = (P + TOPK_ROWS_THREADS - 1) / TOPK_ROWS_THREADS;
  if (per <= 1) launch(k_topk_rows<1>);
  else if (per <= 2) launch(k_topk_rows<2>);
  else if (per <= 4) launch(k_topk_rows<4>);
  else if (per <= 8) launch(k_topk_rows<8>);
  else launch(k_topk_rows<16>);
  return r;
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

// One k_topk_from_masks launch on the current stream, which has to be a
// stream of the tensors' device.  The tile geometry is the tiled ops'
// (tiled_geom_checked); the vector form is decided here, once per call.
std::vector<at::Tensor> kvidx::gpu_topk_from_masks(at::Tensor masks,
                                                   at::Tensor offsets,
                                                   at::Tensor weights,
                                                   int64_t num_pods,
                                                   int64_t top_n) {
  TORCH_CHECK(masks.is_cuda() && masks.dtype() == at::kLong &&
                  masks.dim() == 3 && masks.is_contiguous(),
              "masks must be a contiguous int64 [Ktot, n_tiers, W] device "
              "tensor");
  TORCH_CHECK(offsets.is_cuda() && offsets.dtype() == at::kInt &&
                  offsets.dim() == 1 && offsets.numel() >= 1 &&
                  offsets.is_contiguous(),
              "offsets must be a contiguous int32 [B+1] device tensor");
  const int64_t T = masks.size(1);
  TORCH_CHECK(T >= 1 && T <= MAX_TIERS, "n_tiers must be 1..", MAX_TIERS);
  TORCH_CHECK(weights.is_cuda() && weights.dtype() == at::kFloat &&
                  weights.is_contiguous() && weights.numel() >= T,
              "weights must be a contiguous float32 device tensor with one "
              "entry per tier");
  TORCH_CHECK(offsets.device() == masks.device() &&
                  weights.device() == masks.device(),
              "masks, offsets and weights must share one device");
  TORCH_CHECK(masks.get_device() == at::cuda::current_device(),
              "the current stream belongs to another device than masks");
  TORCH_CHECK(top_n >= 1 && top_n <= MAX_TOPK, "top_n must be 1..", MAX_TOPK);
  const TiledGeom g = tiled_geom_checked(num_pods, 0, T);
  TORCH_CHECK(masks.size(2) == g.W, "masks must hold pod_words(num_pods) = ",
              g.W, " words per tier");
  const int64_t B = offsets.numel() - 1;
  TORCH_CHECK(B <= INT32_MAX, "too many prompts in one batch");
  auto r = topk_alloc(masks, B, top_n);
  if (B == 0) return r;
  const int64_t TW = T * g.W;
  const bool v16 = TW % 2 == 0 &&
                   reinterpret_cast<uintptr_t>(masks.data_ptr()) % 16 == 0;
  // a thread stages one tile in NV registers
  TORCH_CHECK(g.KT * TW <= (v16 ? mask_tile_max_words<true>()
                                : mask_tile_max_words<false>()),
              "mask tile out of range");
  TORCH_CHECK(masks.size(0) <= INT32_MAX, "too many keys in one batch");
  dispatch_tiled_wpw(g.W, [&](auto N) {
    constexpr int WPW = decltype(N)::value;
    auto kern = v16 ? k_topk_from_masks<WPW, true>
                    : k_topk_from_masks<WPW, false>;
    hipLaunchKernelGGL(
        kern, dim3((unsigned)B), dim3(256), g.lds, STREAM,
        reinterpret_cast<const unsigned long long*>(u64p(masks)),
        (const int32_t*)i32p(offsets), (int)masks.size(0),
        (const float*)weights.data_ptr<float>(), (int)T, (int)num_pods,
        (int)g.W, (int)g.KT, topk_out(r, top_n));
  });
  return r;
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
  // The masks do not fit in LDS (a fleet past 1024 pods, or long prompts
  // on a large one): the keys go through LDS a tile at a time.
  return gpu_tiled_score(KVIDX_TABLE_ARGS, hashes, offsets, model_id,
                         filter_words, weights, num_pods, epoch, max_k,
                         n_tiers);
}

// gpu_score_hashes' decision with the pick on the device: the matrix
// never exists.
std::vector<at::Tensor> kvidx::gpu_topk_hashes(
    KVIDX_TABLE_PARAMS, at::Tensor hashes, at::Tensor offsets,
    int64_t model_id, at::Tensor filter_words, at::Tensor weights,
    int64_t num_pods, int64_t epoch, int64_t max_k, int64_t n_tiers,
    int64_t top_n) {
  if (fused_score_fits(max_k, clamp_tiers(n_tiers), pod_words(num_pods)))
    return gpu_fused_topk(KVIDX_TABLE_ARGS, hashes, offsets, model_id,
                          filter_words, weights, num_pods, epoch, max_k,
                          n_tiers, top_n);
  return gpu_tiled_topk(KVIDX_TABLE_ARGS, hashes, offsets, model_id,
                        filter_words, weights, num_pods, epoch, max_k, n_tiers,
                        top_n);
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
//
// Both ops over flat tokens are these two steps and a last call.
// chain_flat_tokens: stage -> chain; rows int64 [B, max_k] and n_keys int32
// [B] on the table's device (undefined where B or max_k is 0).
namespace kvidx {
struct ChainedRows {
  RaggedPlan p;
  at::Tensor rows, n_keys;
};
static ChainedRows chain_flat_tokens(const at::Tensor& keys,
                                     const at::Tensor& tokens_flat,
                                     const at::Tensor& offsets,
                                     int64_t init_hash_bits,
                                     int64_t block_size, int64_t algo) {
  TORCH_CHECK(keys.is_cuda(), "table must live on the GPU");
  TORCH_CHECK(algo_valid(algo), "unknown chain hash algo id ", algo);
  ChainedRows c;
  c.p = plan_ragged(tokens_flat, offsets, block_size);
  if (c.p.B == 0 || c.p.max_k == 0) return c;
  auto dev = keys.device();
  auto staged = stage_ragged(c.p, tokens_flat, block_size, dev);
  auto parents = at::full({c.p.B}, init_hash_bits,
                          at::TensorOptions().device(dev).dtype(at::kLong));
  c.n_keys = staged[1];
  c.rows = kvidx::gpu_hash_chain_tr(staged[0], parents, staged[1], block_size,
                                    c.p.max_k, 0, 1, algo);
  return c;
}
}  // namespace kvidx

at::Tensor kvidx::gpu_score_flat_tokens(KVIDX_TABLE_PARAMS,
                                        at::Tensor tokens_flat,
                                        at::Tensor offsets, int64_t model_id,
                                        at::Tensor filter_words,
                                        at::Tensor weights, int64_t num_pods,
                                        int64_t epoch, int64_t init_hash_bits,
                                        int64_t block_size, int64_t n_tiers,
                                        int64_t algo) {
  auto c = chain_flat_tokens(keys, tokens_flat, offsets, init_hash_bits,
                             block_size, algo);
  const RaggedPlan& p = c.p;
  if (p.B == 0 || p.max_k == 0)
    return at::zeros({p.B, num_pods}, keys.options().dtype(at::kFloat));
  if (fused_score_fits(p.max_k, clamp_tiers(n_tiers), pod_words(num_pods)))
    return gpu_fused_score_rows(KVIDX_TABLE_ARGS, c.rows, c.n_keys, model_id,
                                filter_words, weights, num_pods, epoch,
                                p.max_k, n_tiers);
  return gpu_tiled_score_rows(KVIDX_TABLE_ARGS, c.rows, c.n_keys, model_id,
                              filter_words, weights, num_pods, epoch, p.max_k,
                              n_tiers);
}

// gpu_score_flat_tokens with top-n as the last call.  A batch without a
// whole chunk has no candidates: (-1, 0.0f) everywhere, no launch.
std::vector<at::Tensor> kvidx::gpu_topk_flat_tokens(
    KVIDX_TABLE_PARAMS, at::Tensor tokens_flat, at::Tensor offsets,
    int64_t model_id, at::Tensor filter_words, at::Tensor weights,
    int64_t num_pods, int64_t epoch, int64_t init_hash_bits,
    int64_t block_size, int64_t n_tiers, int64_t algo, int64_t top_n) {
  TORCH_CHECK(top_n >= 1 && top_n <= MAX_TOPK, "top_n must be 1..", MAX_TOPK);
  auto c = chain_flat_tokens(keys, tokens_flat, offsets, init_hash_bits,
                             block_size, algo);
  const RaggedPlan& p = c.p;
  if (p.B == 0 || p.max_k == 0)
    return {at::full({p.B, top_n}, -1, keys.options().dtype(at::kInt)),
            at::zeros({p.B, top_n}, keys.options().dtype(at::kFloat))};
  if (fused_score_fits(p.max_k, clamp_tiers(n_tiers), pod_words(num_pods)))
    return gpu_fused_topk_rows(KVIDX_TABLE_ARGS, c.rows, c.n_keys, model_id,
                               filter_words, weights, num_pods, epoch, p.max_k,
                               n_tiers, top_n);
  return gpu_tiled_topk_rows(KVIDX_TABLE_ARGS, c.rows, c.n_keys, model_id,
                             filter_words, weights, num_pods, epoch, p.max_k,
                             n_tiers, top_n);
}

// Stage and chain over an uploaded wave plan, for the read path's prompts
// (roots: the batch's one init, uint64_t) and the write path's events
// (roots: RootEvents, or RootLinked over a linked plan): one
// k_stage_ragged_waves, then the templated chain kernel at block sizes
// 4/8/16/32/64 and the stream kernel at every other, under the entry the
// roots select.  Under RootLinked the chain entry is launched once per
// level, with that level's wave range [level_wave[l], level_wave[l + 1]),
// in level order: the stream orders the launches, the host waits for none,
// and all levels' images come from the one stage launch.  up: p.host on the
// device; tok: flat tokens on the device, int64 or int32; out: int64, chunk
// c of row r at h_off[r] + c.  p.G > 0.  Everything on the current stream.
namespace kvidx {
template <typename Roots>
static void launch_wave_chain(const WavePlan& p, const at::Tensor& up,
                              const at::Tensor& tok, int64_t block_size,
                              int64_t algo, Roots roots,
                              const at::Tensor& out) {
  constexpr bool EV = std::is_same_v<Roots, RootEvents>;
  constexpr bool LK = std::is_same_v<Roots, RootLinked>;
  const at::Tensor img_off = p.img_off(up);
  const int32_t* w = i32p(up);
  const int32_t* n_chunks = w + p.at_n_chunks();
  const int32_t* perm = w + p.at_perm();
  const int32_t* wave_k = w + p.at_wave_k();
  const int32_t* h_off = w + p.at_h_off();
  auto img = at::empty({p.image_elems}, up.options());
  const int G = (int)p.G;
  auto stage = [&](auto* flat) {
    using TokT = std::remove_const_t<std::remove_pointer_t<decltype(flat)>>;
    hipLaunchKernelGGL(k_stage_ragged_waves<TokT>, dim3((unsigned)p.tiles),
                       dim3(256), 0, STREAM, flat, w + p.at_tok_off(),
                       n_chunks, perm, wave_k, img_off.data_ptr<int64_t>(),
                       w + p.at_tile_start(), G, (int)block_size, i32p(img));
  };
  if (tok.dtype() == at::kLong)
    stage(tok.data_ptr<int64_t>());
  else
    stage(tok.data_ptr<int32_t>());
  // kern over waves [w0, w1), wpg waves per workgroup; with_bound: the
  // entry takes the range's end behind h_off (the SHA waves kernels); rest:
  // what follows the roots.  The _lk entries take both ends of the range.
  auto run = [&](auto kern, auto with_bound, int wpg, auto... rest) {
    auto launch = [&](int w0, int w1) {
      const dim3 grid((unsigned)((w1 - w0 + wpg - 1) / wpg)), block(64 * wpg);
      if constexpr (LK)
        hipLaunchKernelGGL(kern, grid, block, 0, STREAM, i32p(img),
                           img_off.data_ptr<int64_t>(), perm, wave_k, n_chunks,
                           h_off, w0, w1, roots, rest...);
      else if constexpr (decltype(with_bound)::value)
        hipLaunchKernelGGL(kern, grid, block, 0, STREAM, i32p(img),
                           img_off.data_ptr<int64_t>(), perm, wave_k, n_chunks,
                           h_off, w1, roots, rest...);
      else
        hipLaunchKernelGGL(kern, grid, block, 0, STREAM, i32p(img),
                           img_off.data_ptr<int64_t>(), perm, wave_k, n_chunks,
                           h_off, roots, rest...);
    };
    if constexpr (LK) {
      const int32_t* level_wave = p.host.data_ptr<int32_t>() + p.at_level_wave;
      for (int64_t l = 0; l < p.n_levels; ++l)
        if (level_wave[l + 1] > level_wave[l])  // a level may have no chain
          launch(level_wave[l], level_wave[l + 1]);
    } else {
      launch(0, G);
    }
  };
  if (!chain_block_size_templated(block_size)) {
    // one-wave workgroups, block g = wave g, for either hash
    dispatch_algo(algo, [&](auto A) {
      constexpr int AL = decltype(A)::value;
      if constexpr (AL == ALGO_FNV64A)
        run([] {
          if constexpr (LK) return k_fnv_chain_stream_lk;
          else if constexpr (EV) return k_fnv_chain_stream_ev;
          else return k_fnv_chain_stream;
        }(), std::false_type{}, 1, (int)block_size, u64p(out));
      else
        run([] {
          if constexpr (LK) return k_sha_chain_stream_lk<AL>;
          else if constexpr (EV) return k_sha_chain_stream_ev<AL>;
          else return k_sha_chain_stream<AL>;
        }(), std::false_type{}, 1, (int)block_size, u64p(out));
    });
    return;
  }
  dispatch_algo(algo, [&](auto A) {
    dispatch_chain_block_size(block_size, [&](auto S) {
      constexpr int AL = decltype(A)::value;
      constexpr int BS = decltype(S)::value;
      if constexpr (AL == ALGO_FNV64A)
        run([] {
          if constexpr (LK) return k_fnv_chain_waves_lk<BS>;
          else if constexpr (EV) return k_fnv_chain_waves_ev<BS>;
          else return k_fnv_chain_waves<BS>;
        }(), std::false_type{}, 1, u64p(out));
      else
        run([] {
          if constexpr (LK) return k_sha_chain_waves_lk<BS, AL>;
          else if constexpr (EV) return k_sha_chain_waves_ev<BS, AL>;
          else return k_sha_chain_waves<BS, AL>;
        }(), std::true_type{}, sha_tr_threads(BS) / 64, u64p(out));
    });
  });
}

// The ragged device chain: plan (host) -> one upload -> launch_wave_chain,
// on the current stream.  hashes int64 [total_chunks] and h_off int32
// [B+1] on `dev`; both undefined where the batch has no whole chunk
// (nothing is uploaded or launched then).
struct ChainedCsr {
  WavePlan p;
  at::Tensor hashes, h_off;
};
static ChainedCsr chain_ragged_waves(const at::Tensor& tokens_flat,
                                     const at::Tensor& offsets,
                                     int64_t init_hash_bits,
                                     int64_t block_size, int64_t algo,
                                     at::Device dev) {
  TORCH_CHECK(algo_valid(algo), "unknown chain hash algo id ", algo);
  // the five block sizes of the templated kernels keep them; every other
  // one the stream kernels take goes to those.  Refused before anything
  // is uploaded or launched.
  TORCH_CHECK(chain_block_size_templated(block_size) ||
                  stream_chain_block_size_ok(block_size),
              "the ragged device chain takes block sizes 1..65535");
  ChainedCsr c;
  c.p = plan_ragged_waves(tokens_flat, offsets, block_size);
  const WavePlan& p = c.p;
  if (p.G == 0) return c;
  const at::Tensor up = p.host.to(dev);
  c.h_off = p.i32(up, p.at_h_off(), p.B + 1);
  c.hashes = at::empty({p.total_chunks}, up.options().dtype(at::kLong));
  auto tok = tokens_flat.is_cuda() ? tokens_flat.contiguous()
                                   : tokens_flat.contiguous().to(dev);
  launch_wave_chain(p, up, tok, block_size, algo, (uint64_t)init_hash_bits,
                    c.hashes);
  return c;
}
}  // namespace kvidx

std::vector<at::Tensor> kvidx::gpu_hash_chain_ragged(at::Tensor tokens_flat,
                                                     at::Tensor offsets,
                                                     int64_t init_hash_bits,
                                                     int64_t block_size,
                                                     int64_t algo) {
  at::Device dev = tokens_flat.is_cuda()
                       ? tokens_flat.device()
                       : at::Device(at::kCUDA, at::cuda::current_device());
  auto c = chain_ragged_waves(tokens_flat, offsets, init_hash_bits, block_size,
                              algo, dev);
  if (c.p.G > 0) return {c.hashes, c.h_off};
  auto opt = at::TensorOptions().device(dev);
  return {at::empty({0}, opt.dtype(at::kLong)),
          at::zeros({c.p.B + 1}, opt.dtype(at::kInt))};
}

at::Tensor kvidx::gpu_score_flat_tokens_ragged(
    KVIDX_TABLE_PARAMS, at::Tensor tokens_flat, at::Tensor offsets,
    int64_t model_id, at::Tensor filter_words, at::Tensor weights,
    int64_t num_pods, int64_t epoch, int64_t init_hash_bits,
    int64_t block_size, int64_t n_tiers, int64_t algo) {
  TORCH_CHECK(keys.is_cuda(), "table must live on the GPU");
  auto c = chain_ragged_waves(tokens_flat, offsets, init_hash_bits, block_size,
                              algo, keys.device());
  if (c.p.G == 0)
    return at::zeros({c.p.B, num_pods}, keys.options().dtype(at::kFloat));
  return gpu_score_hashes(KVIDX_TABLE_ARGS, c.hashes, c.h_off, model_id,
                          filter_words, weights, num_pods, epoch, c.p.max_k,
                          n_tiers);
}

std::vector<at::Tensor> kvidx::gpu_topk_flat_tokens_ragged(
    KVIDX_TABLE_PARAMS, at::Tensor tokens_flat, at::Tensor offsets,
    int64_t model_id, at::Tensor filter_words, at::Tensor weights,
    int64_t num_pods, int64_t epoch, int64_t init_hash_bits,
    int64_t block_size, int64_t n_tiers, int64_t algo, int64_t top_n) {
  TORCH_CHECK(keys.is_cuda(), "table must live on the GPU");
  TORCH_CHECK(top_n >= 1 && top_n <= MAX_TOPK, "top_n must be 1..", MAX_TOPK);
  auto c = chain_ragged_waves(tokens_flat, offsets, init_hash_bits, block_size,
                              algo, keys.device());
  if (c.p.G == 0)
    return {at::full({c.p.B, top_n}, -1, keys.options().dtype(at::kInt)),
            at::zeros({c.p.B, top_n}, keys.options().dtype(at::kFloat))};
  return gpu_topk_hashes(KVIDX_TABLE_ARGS, c.hashes, c.h_off, model_id,
                         filter_words, weights, num_pods, epoch, c.p.max_k,
                         n_tiers, top_n);
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

// Wave-tiled phase-split apply: the _tr route's bursts (no batch-local
// parent, no store+remove conflict; host verified) over per-wave token
// images, at any block size.  Events sorted by chain length share waves, a
// wave's image is as tall as its own longest event, and each lane resolves
// its parent in the chain kernel's prologue (RootEvents).  The chain
// kernels write only the chunks of kept stores, which are all that
// k_event_inserts reads of req_scratch, so it is not cleared.
void kvidx::gpu_apply_events_split_waves(
    KVIDX_TABLE_PARAMS, at::Tensor tokens_flat, at::Tensor tok_off,
    at::Tensor ehashes, at::Tensor eh_off, at::Tensor parents,
    at::Tensor has_parent, at::Tensor ev_type, at::Tensor pod_entry,
    at::Tensor ev_of, at::Tensor model_of, int64_t init_hash_bits,
    int64_t block_size, int64_t epoch, int64_t shard_id, int64_t num_shards,
    int64_t algo) {
  // refused before anything is uploaded or launched
  TORCH_CHECK(stream_chain_block_size_ok(block_size),
              "the wave-tiled ingest chain takes block sizes 1..65535");
  TORCH_CHECK(algo_valid(algo), "unknown chain hash algo id ", algo);
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  const at::Device dev = keys.device();
  const auto on_dev = [&](const at::Tensor& t, at::ScalarType ty, int64_t n) {
    return t.device() == dev && t.dtype() == ty && t.is_contiguous() &&
           t.numel() == n;
  };
  const int64_t E = ev_type.numel();
  const int64_t n = ehashes.numel();
  TORCH_CHECK(on_dev(tokens_flat, at::kInt, tokens_flat.numel()),
              "event tokens must be int32 (uint32 bit pattern) on the "
              "table's device");
  TORCH_CHECK(on_dev(ehashes, at::kLong, n) && on_dev(ev_of, at::kInt, n),
              "ehashes int64 and ev_of int32 must hold one entry per hash "
              "on the table's device");
  TORCH_CHECK(on_dev(parents, at::kLong, E) &&
                  on_dev(has_parent, at::kByte, E) &&
                  on_dev(pod_entry, at::kInt, E) &&
                  on_dev(model_of, at::kInt, E),
              "parents, has_parent, pod_entry and model_of must hold one "
              "entry per event on the table's device");
  const WavePlan p = plan_event_waves(tok_off, eh_off, ev_type,
                                      tokens_flat.numel(), n, block_size);
  if (E == 0 || n == 0) return;
  const at::Tensor up = p.host.to(dev);  // the one upload
  const at::Tensor d_tok_off = p.i32(up, p.at_tok_off(), E + 1);
  const at::Tensor d_eh_off = p.i32(up, p.at_h_off(), E + 1);
  const at::Tensor d_ev_type =
      p.i32(up, p.at_tail(), p.tail).view(at::kByte).slice(0, 0, E);
  auto req_scratch = at::empty({n}, ehashes.options());
  if (p.G > 0)  // else only removals and dropped stores: the inserts alone
    launch_wave_chain(p, up, tokens_flat, block_size, algo,
                      RootEvents{v, u64p(parents), u8p(has_parent),
                                 i32p(model_of), (uint64_t)init_hash_bits},
                      req_scratch);
  launch_event_inserts(v, ehashes, d_eh_off, ev_of, d_ev_type, d_tok_off,
                       pod_entry, model_of, block_size, epoch, shard_id,
                       num_shards, req_scratch);
}

// Linked wave-tiled phase-split apply: the waves route for bursts WITH
// batch-local parents (no store+remove conflict; host verified).  link /
// level: plan_event_links' result, on the host.  plan_linked_event_waves ->
// the one upload -> stage -> the chain entries level by level (RootLinked)
// -> k_event_inserts.  No batch map and no k_event_chains: the host plan
// has done dev_bmap_find's work, and the launch order the waiting.
void kvidx::gpu_apply_events_split_linked(
    KVIDX_TABLE_PARAMS, at::Tensor tokens_flat, at::Tensor tok_off,
    at::Tensor ehashes, at::Tensor eh_off, at::Tensor parents,
    at::Tensor has_parent, at::Tensor ev_type, at::Tensor pod_entry,
    at::Tensor ev_of, at::Tensor model_of, at::Tensor link, at::Tensor level,
    int64_t init_hash_bits, int64_t block_size, int64_t epoch,
    int64_t shard_id, int64_t num_shards, int64_t algo) {
  // refused before anything is uploaded or launched
  TORCH_CHECK(stream_chain_block_size_ok(block_size),
              "the wave-tiled ingest chain takes block sizes 1..65535");
  TORCH_CHECK(algo_valid(algo), "unknown chain hash algo id ", algo);
  auto v = make_table_view(KVIDX_TABLE_ARGS, true);
  const at::Device dev = keys.device();
  const auto on_dev = [&](const at::Tensor& t, at::ScalarType ty, int64_t n) {
    return t.device() == dev && t.dtype() == ty && t.is_contiguous() &&
           t.numel() == n;
  };
  const int64_t E = ev_type.numel();
  const int64_t n = ehashes.numel();
  TORCH_CHECK(on_dev(tokens_flat, at::kInt, tokens_flat.numel()),
              "event tokens must be int32 (uint32 bit pattern) on the "
              "table's device");
  TORCH_CHECK(on_dev(ehashes, at::kLong, n) && on_dev(ev_of, at::kInt, n),
              "ehashes int64 and ev_of int32 must hold one entry per hash "
              "on the table's device");
  TORCH_CHECK(on_dev(parents, at::kLong, E) &&
                  on_dev(has_parent, at::kByte, E) &&
                  on_dev(pod_entry, at::kInt, E) &&
                  on_dev(model_of, at::kInt, E),
              "parents, has_parent, pod_entry and model_of must hold one "
              "entry per event on the table's device");
  TORCH_CHECK(level.device().is_cpu() && level.dtype() == at::kInt &&
                  level.dim() == 1 && level.numel() == E,
              "level must be an int32 [E] host tensor");
  const EventLinks links{E ? level.max().item<int64_t>() + 1 : 0, link, level};
  const WavePlan p = plan_linked_event_waves(
      tok_off, eh_off, ev_type, links, tokens_flat.numel(), n, block_size);
  if (E == 0 || n == 0) return;
  const at::Tensor up = p.host.to(dev);  // the one upload
  const at::Tensor d_tok_off = p.i32(up, p.at_tok_off(), E + 1);
  const at::Tensor d_eh_off = p.i32(up, p.at_h_off(), E + 1);
  const at::Tensor d_ev_type =
      p.i32(up, p.at_tail(), (E + 3) / 4).view(at::kByte).slice(0, 0, E);
  auto req_scratch = at::empty({n}, ehashes.options());
  if (p.G > 0)  // else only removals and dropped stores: the inserts alone
    launch_wave_chain(
        p, up, tokens_flat, block_size, algo,
        RootLinked{RootEvents{v, u64p(parents), u8p(has_parent),
                              i32p(model_of), (uint64_t)init_hash_bits},
                   i32p(up) + p.at_link, u64p(req_scratch)},
        req_scratch);
  launch_event_inserts(v, ehashes, d_eh_off, ev_of, d_ev_type, d_tok_off,
                       pod_entry, model_of, block_size, epoch, shard_id,
                       num_shards, req_scratch);
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
