"""Table-backed index: HBM3E-resident on GPU, same layout on CPU.

This is the MI355X-native replacement for the reference's Go-map/LRU
in-memory index (pkg/kvcache/kvblock/in_memory.go): an open-addressing
hash table (ops/csrc/kvidx_common.h) probed by wave-cooperative HIP
kernels on gfx950, or by the bit-identical C++ reference on CPU.

Two concrete backends:
 - ``NativeIndex``  - the table on CPU tensors (fast CPU mode; also the
   golden reference for GPU differential tests);
 - ``GpuIndex``     - the table in HBM on ``cuda:N``; inserts/evicts/
   lookups are batched kernel launches; the read path can bypass the
   generic ``lookup`` entirely via ``fused_scores`` (one kernel does
   probe + longest-prefix scoring).

String identities (pod, model, tier) are interned host-side into dense
ids (Registry); the table stores only ids.
"""

from __future__ import annotations

import heapq
import os
import threading
from collections import namedtuple
from contextlib import nullcontext
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from ..scorer import default_kv_cache_backend_configs
from ..utils import hashing
from ..utils.idgate import IdGate
from .event_batch import (FIELDS, FlatEvents, flatten_event_batches,
                          plan_write_route)
from .index import Index
from .keys import Key, PodEntry

MAX_TIERS = 4
DEFAULT_CAPACITY = 1 << 21  # 2M slots; ~1M keys at 0.5 load factor
DEFAULT_PODS_PER_KEY = 10  # in_memory.go:34
MAX_PODS = 4096


def _to_i64(h: int) -> int:
    """uint64 -> int64 bit reinterpretation for torch tensors."""
    return h - (1 << 64) if h >= (1 << 63) else h


def _to_u64(v: int) -> int:
    return v & 0xFFFFFFFFFFFFFFFF


class Registry:
    """Interns pod/model/tier strings to dense ids (thread-safe).

    Pod ids can be given back (``release_pods``): a released id holds the
    empty string in ``id_to_pod`` and is absent from ``pod_to_id``.
    ``pod_id`` reuses the LOWEST free id before growing - a deterministic
    policy, so replicated ranks fed the same stream agree - and trailing
    free ids are trimmed, so ``num_pods`` shrinks again.

    Ids of LIVE pods change only in ``apply_pod_compaction``.  Whoever
    carries a pod id across calls - from name to launch, or from an
    id-ordered result back to names - does so inside ``ids_shared()``;
    the compaction runs inside ``ids_exclusive()``.  ``pod_generation``
    counts the compactions applied: a caller who keeps an id-ordered
    tensor (``fused_scores``) outside any such span compares it before
    and after, and discards the tensor if it moved."""

    def __init__(self, tier_names: Optional[Sequence[str]] = None):
        self._lock = threading.Lock()
        self._id_gate = IdGate()
        self.pod_generation = 0
        self.pod_to_id: Dict[str, int] = {}
        self.id_to_pod: List[str] = []
        self._free_pod_ids: List[int] = []  # min-heap of holes in id_to_pod
        self.model_to_id: Dict[str, int] = {}
        self.id_to_model: List[str] = []
        tiers = list(tier_names or [b.name for b in default_kv_cache_backend_configs()])
        self.tier_to_id: Dict[str, int] = {}
        self.id_to_tier: List[str] = []
        for t in tiers:
            self._intern_tier(t)

    def _intern_tier(self, tier: str) -> int:
        tid = self.tier_to_id.get(tier)
        if tid is None:
            if len(self.id_to_tier) >= MAX_TIERS:
                # Silently sharing a slot would mis-weight scores for
                # every tier folded onto it; fail loudly instead (event
                # paths catch this and drop the offending event).
                raise ValueError(
                    f"tier registry full ({MAX_TIERS}): cannot intern "
                    f"{tier!r}; registered tiers: {self.id_to_tier}"
                )
            tid = len(self.id_to_tier)
            self.tier_to_id[tier] = tid
            self.id_to_tier.append(tier)
        return tid

    def pod_id(self, pod: str) -> int:
        if not pod:
            raise ValueError("pod identifier must not be empty")
        with self._lock:
            pid = self.pod_to_id.get(pod)
            if pid is None:
                if self._free_pod_ids:
                    pid = heapq.heappop(self._free_pod_ids)
                    self.id_to_pod[pid] = pod
                else:
                    if len(self.id_to_pod) >= MAX_PODS:
                        raise ValueError(f"pod registry full ({MAX_PODS})")
                    pid = len(self.id_to_pod)
                    self.id_to_pod.append(pod)
                self.pod_to_id[pod] = pid
            return pid

    def release_pods(self, pods: Sequence[str]) -> List[int]:
        """Give back the ids of these pods (unknown names are ignored);
        returns the released ids.  The caller has already purged them
        from every table that shares this registry."""
        with self._lock:
            released = []
            for pod in pods:
                pid = self.pod_to_id.pop(pod, None)
                if pid is None:
                    continue
                self.id_to_pod[pid] = ""
                heapq.heappush(self._free_pod_ids, pid)
                released.append(pid)
            if released:
                self._trim_free_tail()
            return released

    def _trim_free_tail(self) -> None:
        n = len(self.id_to_pod)
        while n and not self.id_to_pod[n - 1]:
            n -= 1
        if n != len(self.id_to_pod):
            del self.id_to_pod[n:]
            self._free_pod_ids = [i for i in self._free_pod_ids if i < n]
            heapq.heapify(self._free_pod_ids)

    def _set_pods(self, names: Sequence[str]) -> None:
        """Replace the pod id space (checkpoint load); empty names are
        free ids.  Caller holds the lock."""
        self.id_to_pod = list(names)
        self.pod_to_id = {p: i for i, p in enumerate(self.id_to_pod) if p}
        self._free_pod_ids = [i for i, p in enumerate(self.id_to_pod)
                              if not p]
        heapq.heapify(self._free_pod_ids)
        self._trim_free_tail()

    # -- renumbering ----------------------------------------------------
    def ids_shared(self):
        """Context manager: pod ids do not change inside (re-entrant)."""
        return self._id_gate.shared

    def ids_exclusive(self):
        """Context manager: no ids_shared() span is open inside."""
        return self._id_gate.exclusive

    def plan_pod_compaction(self, dropping: Sequence[str] = ()
                            ) -> Optional[List[int]]:
        """The order-preserving map that closes every hole: remap[old] is
        the new id of a live pod (the live ids in ascending order become
        0, 1, 2, ...) and -1 for a free id.  A pure function of the
        registry, so replicas fed the same stream plan the same map.
        None if no hole lies below the highest live id.  Pods named in
        `dropping` count as free already (retire and compact at once)."""
        with self._lock:
            drop = {self.pod_to_id[p] for p in dropping if p in self.pod_to_id}
            remap, nxt, holes = [], 0, False
            for pid, name in enumerate(self.id_to_pod):
                if name and pid not in drop:
                    remap.append(nxt)
                    holes |= nxt != pid
                    nxt += 1
                else:
                    remap.append(-1)
            return remap if holes else None

    def apply_pod_compaction(self, remap: Sequence[int]) -> None:
        """Renumber by a plan_pod_compaction map (ids mapped to -1 are
        forgotten) and bump pod_generation.  The caller holds
        ids_exclusive() and has rewritten every table that shares this
        registry."""
        with self._lock:
            if len(remap) != len(self.id_to_pod):
                raise ValueError("remap does not match the pod id space")
            live = [(new, self.id_to_pod[old])
                    for old, new in enumerate(remap) if new >= 0]
            names = [""] * (max((n for n, _ in live), default=-1) + 1)
            for new, name in live:
                if not name or names[new]:
                    raise ValueError("remap is not a renumbering of live pods")
                names[new] = name
            self._set_pods(names)
            self.pod_generation += 1

    def model_id(self, model: str) -> int:
        with self._lock:
            mid = self.model_to_id.get(model)
            if mid is None:
                if len(self.id_to_model) >= 0xFFFF:
                    raise ValueError("model registry full")
                mid = len(self.id_to_model)
                self.model_to_id[model] = mid
                self.id_to_model.append(model)
            return mid

    def tier_id(self, tier: str) -> int:
        with self._lock:
            return self._intern_tier(tier)

    @property
    def num_pods(self) -> int:
        with self._lock:
            return len(self.id_to_pod)


@dataclass
class TableIndexConfig:
    capacity: int = DEFAULT_CAPACITY
    pods_per_key: int = DEFAULT_PODS_PER_KEY
    device: str = "cpu"
    # sharding: the main table stores only keys with
    # chunk_hash % num_shards == shard_id; the engine map is replicated
    # (parallel/sharded.py merges per-shard masks over RCCL)
    shard_id: int = 0
    num_shards: int = 1
    tier_names: List[str] = field(
        default_factory=lambda: [b.name for b in default_kv_cache_backend_configs()]
    )


@dataclass
class GpuIndexConfig(TableIndexConfig):
    device: str = "cuda:0"


class KvTable:
    """Tensor bundle + op dispatch for one table instance."""

    def __init__(self, cfg: TableIndexConfig):
        cap = cfg.capacity
        if cap & (cap - 1):
            raise ValueError("capacity must be a power of two")
        self.cfg = cfg
        self.device = torch.device(cfg.device)
        self.is_cuda = self.device.type == "cuda"
        from ..ops import cpu_ext

        self.ops = cpu_ext.require()
        if self.is_cuda and not self.ops.HAS_HIP:
            raise RuntimeError(
                "native extension built without HIP support but a GPU table "
                "was requested - rebuild with ROCm torch"
            )
        opts = dict(device=self.device)
        self.keys = torch.zeros(cap, dtype=torch.int64, **opts)
        self.meta = torch.zeros(cap, dtype=torch.int32, **opts)
        self.stamp = torch.zeros(cap, dtype=torch.int32, **opts)
        self.pods = torch.zeros(cap * cfg.pods_per_key, dtype=torch.int32, **opts)
        self.e_keys = torch.zeros(cap, dtype=torch.int64, **opts)
        self.e_meta = torch.zeros(cap, dtype=torch.int32, **opts)
        self.e_vals = torch.zeros(cap, dtype=torch.int64, **opts)
        self._epoch = 0
        self._epoch_lock = threading.Lock()

    def next_epoch(self) -> int:
        with self._epoch_lock:
            self._epoch = (self._epoch + 1) & 0x7FFFFFFF
            return self._epoch

    def _t(self):
        return (
            self.keys,
            self.meta,
            self.stamp,
            self.pods,
            self.e_keys,
            self.e_meta,
            self.e_vals,
            self.cfg.pods_per_key,
        )

    # -- raw ops (tensors in the table's device) -----------------------
    def insert(self, engine_hashes, request_hashes, model_id, pod_entries,
               emap_write: bool = True):
        """emap_write=False skips the engine-map write - the tier-
        promotion path reuses request hashes as engine hashes and a
        self-mapping there would corrupt get_request_key()."""
        fn = self.ops.gpu_insert if self.is_cuda else self.ops.cpu_insert
        fn(*self._t(), engine_hashes, request_hashes, model_id, pod_entries,
           self.next_epoch(), self.cfg.shard_id, self.cfg.num_shards,
           1 if emap_write else 0)

    def evict(self, engine_hashes, model_id, pod_entries):
        fn = self.ops.gpu_evict if self.is_cuda else self.ops.cpu_evict
        fn(*self._t(), engine_hashes, model_id, pod_entries)

    def purge_pods(self, purge_words, model_id: int = -1) -> Tuple[int, int]:
        """Strip a set of pods from every pod set of the table (model_id
        -1: of every model) and tombstone the keys that become empty.
        purge_words: int64 [W], bit pid % 64 of word pid // 64 selects
        pod id pid.  Returns (entries_cleared, keys_tombstoned); on a GPU
        table the sweep has completed when this returns."""
        words = purge_words.to(device=self.device, dtype=torch.int64)
        fn = (self.ops.gpu_purge_pods if self.is_cuda
              else self.ops.cpu_purge_pods)
        entries, keys = fn(*self._t(), words.contiguous(), model_id)
        return int(entries), int(keys)

    def remap_pods(self, remap: Sequence[int]) -> Tuple[int, int, int]:
        """Rewrite pod ids in every pod set of the table: remap[old] is
        the new id, -1 drops the entry, ids >= len(remap) stay; keys that
        lose their last entry are tombstoned.  Returns (entries_moved,
        entries_cleared, keys_tombstoned).  The caller keeps every other
        writer off the table for the duration (the sweep uses plain
        stores); on a GPU table it has completed when this returns."""
        t = torch.as_tensor(remap, dtype=torch.int32).to(self.device)
        fn = (self.ops.gpu_remap_pods if self.is_cuda
              else self.ops.cpu_remap_pods)
        moved, cleared, keys = fn(*self._t(), t.contiguous())
        return int(moved), int(cleared), int(keys)

    def lookup(self, request_hashes, model_id, filter_words, num_pods,
               sharded=True, n_tiers=MAX_TIERS):
        fn = self.ops.gpu_lookup if self.is_cuda else self.ops.cpu_lookup
        cfg = self.cfg
        shard_id = cfg.shard_id if sharded else 0
        num_shards = cfg.num_shards if sharded else 1
        return fn(*self._t(), request_hashes, model_id, filter_words,
                  num_pods, self.next_epoch(), shard_id, num_shards,
                  n_tiers)

    def score_hashes(self, hashes, counts_or_offsets, model_id, filter_words,
                     weights, num_pods, max_k=None, n_tiers=MAX_TIERS):
        if self.is_cuda:
            # fused kernel, or lookup + mask walk where its LDS is too
            # small.  n_tiers (tiers registered) sizes that LDS: 1-2 tiers
            # keep 256-pod fleets at 16-32 KB/WG and full occupancy.
            return self.ops.gpu_score_hashes(
                *self._t(), hashes, counts_or_offsets, model_id, filter_words,
                weights, num_pods, self.next_epoch(),
                max_k if max_k is not None else 512, n_tiers)
        return self.ops.cpu_fused_score(
            *self._t(), hashes, counts_or_offsets, model_id, filter_words,
            weights, num_pods, self.next_epoch())

    def compact(self, new_capacity: Optional[int] = None) -> None:
        """Rehash every live entry into a fresh tensor bundle, dropping
        tombstones and dead probe windows (ROADMAP #9 - long-running
        tables). Stamps (approximate-LRU) and pod rows carry over;
        new_capacity (power of two) allows growing/shrinking. Costs 2x
        table memory transiently; callers serialize against writes."""
        import copy

        cfg = copy.copy(self.cfg)
        if new_capacity is not None:
            if new_capacity & (new_capacity - 1):
                raise ValueError("capacity must be a power of two")
            cfg.capacity = new_capacity
        fresh = KvTable(cfg)
        fn = self.ops.gpu_compact if self.is_cuda else self.ops.cpu_compact
        fn(*self._t(), *fresh._t()[:-1])
        self.cfg = cfg
        for name in ("keys", "meta", "stamp", "pods",
                     "e_keys", "e_meta", "e_vals"):
            setattr(self, name, getattr(fresh, name))

    def get_request_keys(self, engine_hashes, model_id):
        fn = (self.ops.gpu_get_request_keys if self.is_cuda
              else self.ops.cpu_get_request_keys)
        return fn(*self._t(), engine_hashes, model_id)

    # -- checkpoint/restore --------------------------------------------
    # The reference index is ephemeral by design (rebuilds from the event
    # stream; durability delegated to Redis - docs/architecture.md:129).
    # The table layout makes snapshots nearly free on MI355X, so we offer
    # them as a native extra: one D2H copy of the tensor bundle.
    def state_dict(self):
        return {
            "keys": self.keys.cpu(),
            "meta": self.meta.cpu(),
            "stamp": self.stamp.cpu(),
            "pods": self.pods.cpu(),
            "e_keys": self.e_keys.cpu(),
            "e_meta": self.e_meta.cpu(),
            "e_vals": self.e_vals.cpu(),
            "capacity": self.keys.numel(),
            "pods_per_key": self.cfg.pods_per_key,
            "epoch": self._epoch,
        }

    def load_state_dict(self, state):
        if state["capacity"] != self.keys.numel() or (
            state["pods_per_key"] != self.cfg.pods_per_key
        ):
            raise ValueError("snapshot shape mismatch")
        for name in ("keys", "meta", "stamp", "pods", "e_keys", "e_meta",
                     "e_vals"):
            getattr(self, name).copy_(state[name].to(self.device))
        self._epoch = int(state.get("epoch", 0))


# TableIndex.score_args: num_pods is padded to whole 64-pod mask words,
# filter_words int64 [W] (or [0]: every pod), weights float32 [MAX_TIERS]
ScoreArgs = namedtuple("ScoreArgs",
                       "model_id num_pods filter_words weights n_tiers")


class TableIndex(Index):
    """Index contract over a KvTable (CPU or GPU device)."""

    def __init__(self, cfg: Optional[TableIndexConfig] = None,
                 registry: Optional[Registry] = None):
        self.cfg = cfg or TableIndexConfig()
        self.table = KvTable(self.cfg)
        self.registry = registry or Registry(self.cfg.tier_names)
        self._write_lock = threading.Lock()  # CPU ops are single-writer
        self.device = self.table.device

    # -- helpers -------------------------------------------------------
    def _hashes_tensor(self, keys: Sequence[Key]):
        return torch.tensor([_to_i64(k.chunk_hash) for k in keys],
                            dtype=torch.int64, device=self.device)

    def _entries_tensor(self, entries: Sequence[PodEntry]):
        vals = []
        for e in entries:
            pid = self.registry.pod_id(e.pod_identifier)
            tid = self.registry.tier_id(e.device_tier)
            vals.append((tid << 24) | (pid + 1))
        return torch.tensor(vals, dtype=torch.int32, device=self.device)

    def _filter_tensor(self, pod_identifier_set: Set[str], num_pods: int):
        if not pod_identifier_set:
            return torch.zeros(0, dtype=torch.int64, device=self.device)
        W = (num_pods + 63) // 64
        words = [0] * W
        for pod in pod_identifier_set:
            pid = self.registry.pod_to_id.get(pod)
            if pid is not None and pid < num_pods:
                words[pid // 64] |= 1 << (pid % 64)
        return torch.tensor([_to_i64(w) for w in words], dtype=torch.int64,
                            device=self.device)

    def _num_pods_padded(self) -> int:
        return max(64, (self.registry.num_pods + 63) // 64 * 64)

    def score_args(self, model_name: str, pods, backend_configs=None,
                   weights: Optional[torch.Tensor] = None) -> "ScoreArgs":
        """What every probe/score op takes besides table and keys, staged
        once.  pods: candidate filter (empty = all).  weights: the given
        tensor, else from backend_configs (None = the default configs)."""
        num_pods = self._num_pods_padded()
        if weights is None:
            weights = self.tier_weights(
                None if backend_configs is None
                else {b.name: b.weight for b in backend_configs})
        return ScoreArgs(self.registry.model_id(model_name), num_pods,
                         self._filter_tensor(set(pods), num_pods), weights,
                         max(1, len(self.registry.id_to_tier)))

    # -- Index contract ------------------------------------------------
    def lookup(self, request_keys: Sequence[Key],
               pod_identifier_set: Set[str]) -> Dict[Key, List[PodEntry]]:
        if not request_keys:
            raise ValueError("no request keys provided for lookup")
        with self.registry.ids_shared():
            return self._lookup(request_keys, pod_identifier_set)

    def _lookup(self, request_keys, pod_identifier_set):
        a = self.score_args(request_keys[0].model_name, pod_identifier_set)
        found, masks = self.table.lookup(
            self._hashes_tensor(request_keys), a.model_id, a.filter_words,
            a.num_pods, n_tiers=a.n_tiers)
        found = found.cpu().tolist()
        masks_l = masks.cpu().tolist()  # one bulk D2H/convert, no per-item
        W = masks.shape[2]
        n_tiers = masks.shape[1]
        pod_names = list(self.registry.id_to_pod)  # "" = released id

        result: Dict[Key, List[PodEntry]] = {}
        for i, key in enumerate(request_keys):
            f = found[i]
            if f == 0:
                continue  # absent: skip, keep walking (in_memory.go:141)
            if f == 2:
                break  # present-but-empty: chain cut (in_memory.go:118-121)
            entries: List[PodEntry] = []
            for t in range(n_tiers):
                tier_name = (self.registry.id_to_tier[t]
                             if t < len(self.registry.id_to_tier) else None)
                if tier_name is None:
                    continue
                for w in range(W):
                    bits = _to_u64(masks_l[i][t][w])
                    while bits:
                        b = (bits & -bits).bit_length() - 1
                        bits &= bits - 1
                        pid = w * 64 + b
                        if pid < len(pod_names) and pod_names[pid]:
                            entries.append(PodEntry(
                                pod_names[pid], tier_name))
            if entries:
                result[key] = entries
        return result

    def add(self, engine_keys: Sequence[Key], request_keys: Sequence[Key],
            entries: Sequence[PodEntry], write_emap: bool = True) -> None:
        if not engine_keys or not request_keys or not entries:
            raise ValueError("no keys or entries provided for adding to index")
        if len(engine_keys) != len(request_keys):
            raise ValueError("mismatch between engine keys and request keys length")
        model_id = self.registry.model_id(request_keys[0].model_name)
        eh = self._hashes_tensor(engine_keys)
        rh = self._hashes_tensor(request_keys)
        with self.registry.ids_shared():
            pe = self._entries_tensor(entries)
            with self._write_lock:
                self.table.insert(eh, rh, model_id, pe, emap_write=write_emap)

    def evict(self, engine_key: Key, entries: Sequence[PodEntry]) -> None:
        if not entries:
            raise ValueError("no entries provided for eviction from index")
        model_id = self.registry.model_id(engine_key.model_name)
        eh = self._hashes_tensor([engine_key])
        with self.registry.ids_shared():
            pe = self._entries_tensor(entries)
            with self._write_lock:
                self.table.evict(eh, model_id, pe)

    def get_request_key(self, engine_key: Key) -> Optional[Key]:
        model_id = self.registry.model_id(engine_key.model_name)
        eh = self._hashes_tensor([engine_key])
        found, out = self.table.get_request_keys(eh, model_id)
        if int(found[0]) == 0:
            return None
        return Key(engine_key.model_name, _to_u64(int(out[0])))

    # -- purge by pod --------------------------------------------------
    def _purge_locked(self, pods: Sequence[str],
                      model_name: Optional[str]) -> dict:
        """clear_pods body; the caller holds _write_lock."""
        reg = self.registry
        known = sorted({p for p in pods if p in reg.pod_to_id})
        out = {"entries_cleared": 0, "keys_tombstoned": 0, "pods": known}
        model_id = -1
        if model_name is not None:
            model_id = reg.model_to_id.get(model_name)
            if model_id is None:
                return out  # a model nobody stored under: nothing to clear
        ids = [reg.pod_to_id[p] for p in known]
        if not ids:
            return out  # empty effective set: no launch
        words = [0] * (max(ids) // 64 + 1)
        for pid in ids:
            words[pid // 64] |= 1 << (pid % 64)
        purge_words = torch.tensor([_to_i64(w) for w in words],
                                   dtype=torch.int64)
        entries, keys = self.table.purge_pods(purge_words, model_id)
        out["entries_cleared"] = entries
        out["keys_tombstoned"] = keys
        return out

    def clear_pods(self, pods: Sequence[str],
                   model_name: Optional[str] = None) -> dict:
        """Remove every entry of these pods (of one model, or of all) and
        tombstone the keys that become empty.  The pods keep their ids:
        they are alive and will report blocks again.  Unknown pod names
        are ignored.  One sweep over the table, on its device."""
        with self.registry.ids_shared(), self._write_lock:
            return self._purge_locked(pods, model_name)

    def retire_pods(self, pods: Sequence[str], compact: bool = False) -> dict:
        """clear_pods for all models, then give the pods' ids back to the
        registry (lowest-free reuse, trailing ids trimmed - the score
        width W shrinks again).

        compact=True purges and renumbers in ONE sweep (the retired pods
        map to -1, the survivors downwards) under the exclusive id gate;
        the result then also carries compact_pod_ids()'s keys.

        The ids are released only after the sweep has completed on the
        device, and still under the write lock, so no entry of a released
        id is left for the id's next owner to inherit.  Caller contract:
        no more events for a retired pod are in flight.  A late event is
        not an error - it re-interns the name under a fresh id - but what
        it stores stays until the pod is retired again."""
        if compact:
            with self.registry.ids_exclusive(), self._write_lock:
                return self._retire_compact_locked([self], pods)
        with self.registry.ids_shared(), self._write_lock:
            out = self._purge_locked(pods, None)
            self.registry.release_pods(out["pods"])
            return out

    # -- compact pod ids -----------------------------------------------
    @staticmethod
    def _remap_tables(tables: Sequence["TableIndex"], reg: "Registry",
                      remap: Optional[List[int]]) -> dict:
        """One remap sweep per table, then the one registry swap.  The
        caller holds reg.ids_exclusive() and every table's write lock."""
        out = {"pods_moved": 0, "entries_moved": 0, "entries_cleared": 0,
               "keys_tombstoned": 0}
        if remap is not None:
            for idx in tables:
                if idx.table.is_cuda:
                    # kernels launched inside shared spans, on any stream
                    torch.cuda.synchronize(idx.device)
            for idx in tables:
                moved, cleared, keys = idx.table.remap_pods(remap)
                out["entries_moved"] += moved
                out["entries_cleared"] += cleared
                out["keys_tombstoned"] += keys
            out["pods_moved"] = sum(1 for old, new in enumerate(remap)
                                    if new >= 0 and new != old)
            reg.apply_pod_compaction(remap)
        out["num_pods"] = reg.num_pods
        out["pod_generation"] = reg.pod_generation
        return out

    @staticmethod
    def _compact_locked(tables: Sequence["TableIndex"]) -> dict:
        reg = tables[0].registry
        return TableIndex._remap_tables(tables, reg,
                                        reg.plan_pod_compaction())

    @staticmethod
    def _retire_compact_locked(tables: Sequence["TableIndex"],
                               pods: Sequence[str]) -> dict:
        """retire_pods(compact=True) body over the tables that share one
        registry; gate and write locks are the caller's."""
        reg = tables[0].registry
        known = sorted({p for p in pods if p in reg.pod_to_id})
        remap = reg.plan_pod_compaction(dropping=known)
        if remap is None and known:
            # the retired pods hold the highest ids: nobody moves, but the
            # sweep still has to drop their entries
            drop = {reg.pod_to_id[p] for p in known}
            remap = [-1 if i in drop or not name else i
                     for i, name in enumerate(reg.id_to_pod)]
        out = TableIndex._remap_tables(tables, reg, remap)
        out["pods"] = known
        return out

    def compact_pod_ids(self) -> dict:
        """Renumber the live pods 0, 1, 2, ... in id order, in one sweep
        over the table, so that the score width W depends on how many
        pods are alive and not on which ids they happen to hold.  Nothing
        to do (no launch, zeros) when no hole lies below the highest live
        id.  entries_cleared / keys_tombstoned are 0 unless a stale entry
        of a free id was found - and dropped.

        Takes the exclusive id gate: waits for every open ids_shared()
        span, and on a GPU table for the kernels they launched.  Id-
        ordered tensors from before the call (fused_scores) are void
        afterwards; registry.pod_generation tells."""
        with self.registry.ids_exclusive(), self._write_lock:
            return self._compact_locked([self])

    # -- fast paths ----------------------------------------------------
    def fused_scores(self, hashes: torch.Tensor, counts_or_offsets: torch.Tensor,
                     model_name: str, pod_identifier_set: Set[str],
                     weights: Optional[torch.Tensor] = None,
                     max_k: Optional[int] = None) -> torch.Tensor:
        """Batched probe + longest-prefix score, one call.

        hashes: int64 flat request hashes; counts (CPU table) or offsets
        [B+1] int32 (GPU table). Returns float32 [B, num_pods] scores in
        registry pod-id order.  Callers that turn the columns back into
        names (scores_to_map) hold registry.ids_shared() from before this
        call until after that; one that keeps the tensor longer checks
        registry.pod_generation."""
        a = self.score_args(model_name, pod_identifier_set, weights=weights)
        # CPU ops are single-writer
        with nullcontext() if self.table.is_cuda else self._write_lock:
            return self.table.score_hashes(
                hashes, counts_or_offsets, a.model_id, a.filter_words,
                a.weights, a.num_pods, max_k, a.n_tiers)

    def tier_weights(self, weight_map: Optional[Dict[str, float]] = None
                     ) -> torch.Tensor:
        """Per-tier-id weight vector; unknown tiers weigh 1.0
        (kvblock_scorer.go:93-99)."""
        if weight_map is None:
            weight_map = {b.name: b.weight
                          for b in default_kv_cache_backend_configs()}
        w = [1.0] * MAX_TIERS
        for i, name in enumerate(self.registry.id_to_tier):
            w[i] = weight_map.get(name, 1.0)
        return torch.tensor(w, dtype=torch.float32, device=self.device)

    def compact(self, new_capacity: Optional[int] = None) -> None:
        """Reclaim tombstoned slots (and optionally resize) - see
        KvTable.compact. Takes the write lock."""
        with self._write_lock:
            self.table.compact(new_capacity)

    def save(self, path: str) -> None:
        """Checkpoint the table + string registries to a file."""
        state = self.table.state_dict()
        state["registry"] = {
            "pods": list(self.registry.id_to_pod),
            "models": list(self.registry.id_to_model),
            "tiers": list(self.registry.id_to_tier),
        }
        torch.save(state, path)

    def load(self, path: str) -> None:
        state = torch.load(path, map_location="cpu", weights_only=False)
        reg = state.pop("registry")
        self.table.load_state_dict(state)
        r = self.registry
        with r._lock:
            r._set_pods(reg["pods"])  # "" entries rebuild the free list
            r.id_to_model = list(reg["models"])
            r.model_to_id = {m: i for i, m in enumerate(r.id_to_model)}
            r.id_to_tier = list(reg["tiers"])
            r.tier_to_id = {t: i for i, t in enumerate(r.id_to_tier)}

    def scores_to_map(self, scores: torch.Tensor) -> List[Dict[str, float]]:
        """float [B, num_pods] -> per-prompt {pod: score} (nonzero only).
        One whole-matrix nonzero + one Python pass over the hits (a
        per-row torch.nonzero loop costs ~50us/row at service batch
        sizes)."""
        sc = scores.cpu()
        B = sc.shape[0]
        out: List[Dict[str, float]] = [{} for _ in range(B)]
        nzi = torch.nonzero(sc)
        if nzi.numel() == 0:
            return out
        vals = sc[nzi[:, 0], nzi[:, 1]].tolist()
        rows = nzi[:, 0].tolist()
        cols = nzi[:, 1].tolist()
        names = list(self.registry.id_to_pod)  # "" = released id
        n_names = len(names)
        for r, c, v in zip(rows, cols, vals):
            if c < n_names and names[c]:
                out[r][names[c]] = v
        return out


class _PinnedUploader:
    """Double-buffered pinned staging for event uploads.

    numpy -> pinned host buffer (CPU memcpy) -> true async H2D DMA,
    instead of pageable `.to(non_blocking=True)` (which bounces through
    the runtime's staging path and serializes).  Two slots rotate; a
    slot's recorded event is synchronized before the slot is rewritten
    so an in-flight DMA never reads a buffer being reused (roadmap #4).
    """

    SLOTS = 2

    def __init__(self):
        self._slots = [dict() for _ in range(self.SLOTS)]
        self._events = [None] * self.SLOTS
        self._i = 0

    def begin(self) -> None:
        import time as _time

        self._i = (self._i + 1) % self.SLOTS
        ev = self._events[self._i]
        if ev is not None:
            # NOT ev.synchronize(): hipEventSynchronize costs ~2.4 ms of
            # interrupt-wakeup latency on this stack even for an already-
            # complete event (measured: scripts/bench_upload.py), which
            # would dominate the ~3 ms batch. query() is ~us and nearly
            # always already true when a slot rotates back around.
            while not ev.query():
                _time.sleep(0)

    def up(self, arr, name: str, device, wait: bool = False) -> torch.Tensor:
        # wait is the pageable uploader's: here the slot's event waits
        src = torch.from_numpy(arr)
        n = src.numel()
        if n == 0:
            return torch.zeros(0, dtype=src.dtype, device=device)
        slot = self._slots[self._i]
        buf = slot.get(name)
        if buf is None or buf.numel() < n or buf.dtype != src.dtype:
            cap = max(1024, 1 << (n - 1).bit_length())
            buf = torch.empty(cap, dtype=src.dtype, pin_memory=True)
            slot[name] = buf
        buf[:n].copy_(src)
        return buf[:n].to(device, non_blocking=True)

    def end(self) -> None:
        # reuse one event per slot: hipEventCreate/Destroy churn per call
        # is measurable on this stack (scripts/bench_upload.py)
        ev = self._events[self._i]
        if ev is None:
            ev = self._events[self._i] = torch.cuda.Event()
        ev.record()


class _PageableUploader:
    """Event uploads straight from pageable memory; nothing to rotate.
    wait=True is torch.tensor(list, device=...)'s blocking copy, back once
    the stream has drained: for the small arrays, not the payload."""

    begin = end = staticmethod(lambda: None)

    def up(self, arr, name: str, device, wait: bool = False) -> torch.Tensor:
        return torch.from_numpy(arr).to(device, non_blocking=not wait)


def _event_uploader(index):
    """Pageable by default: on MI355X pinned+async stalls 38-96 ms now and
    then (scripts/bench_upload.py).  KVIDX_PINNED=1 opts back in."""
    if os.environ.get("KVIDX_PINNED", "0") != "1":
        return _PageableUploader()
    up = getattr(index, "_pinned_up", None)
    if up is None:
        up = index._pinned_up = _PinnedUploader()
    return up


def _upload_events(flat: FlatEvents, route, up, device) -> FlatEvents:
    """flat's arrays as device tensors under the same names."""
    if route.tokens_int32:
        # int32 bit pattern of uint32 token ids: HALF the upload.  Kept in
        # flat, so it lives until after the launch like every other array.
        flat.tokens = flat.tokens.astype(np.uint32).view(np.int32)
    dev = FlatEvents()
    for name in FIELDS:
        setattr(dev, name, up.up(getattr(flat, name), name, device,
                                 wait=name not in ("tokens", "ehashes")))
    if route.op != "gpu_apply_events":
        flat.ev_of = flat.event_of_hash()
        dev.ev_of = up.up(flat.ev_of, "ev_of", device)
    return dev


class NativeIndex(TableIndex):
    """CPU-tensor table (fast CPU backend + GPU-parity reference)."""

    def __init__(self, cfg: Optional[TableIndexConfig] = None, **kw):
        cfg = cfg or TableIndexConfig()
        cfg.device = "cpu"
        super().__init__(cfg, **kw)


class GpuIndex(TableIndex):
    """HBM3E-resident table probed by gfx950 HIP kernels.

    Fails loudly if the HIP extension is missing or no GPU is visible -
    there is no silent CPU fallback on a GPU host."""

    def __init__(self, cfg: Optional[GpuIndexConfig] = None, **kw):
        cfg = cfg or GpuIndexConfig()
        if not torch.cuda.is_available():
            raise RuntimeError(
                "GpuIndex requires a visible AMD GPU (torch.cuda unavailable)"
            )
        super().__init__(cfg, **kw)
        if not self.table.is_cuda:
            raise RuntimeError("GpuIndexConfig.device must be a cuda device")

    def apply_event_batches(self, batches: List[Tuple[str, str, list]],
                            token_processor=None,
                            clear_on_all_blocks_cleared: bool = False) -> None:
        """Apply decoded KV event batches fully on-device.

        batches: list of (pod_identifier, model_name, [events]) in arrival
        order; per-pod ordering is preserved by grouping (one wave per pod
        group processes its events serially - kvevents/pool.go:132-144).

        clear_on_all_blocks_cleared: an AllBlocksCleared event purges its
        pod's entries for that model at the event's position: what the
        burst holds up to there is applied, the pod is swept
        (k_purge_pods, same stream), and the rest of the burst follows.
        The pod keeps its id.  A burst without such an event, or with the
        option off, takes the one-pass path unchanged.
        """
        from ..kvevents.events import AllBlocksCleared

        # named through the class: callers bind this method to plain
        # TableIndex objects (the sharded service's local shard)
        apply = GpuIndex._apply_event_batches
        if clear_on_all_blocks_cleared and any(
                isinstance(ev, AllBlocksCleared)
                for _, _, events in batches for ev in events):
            pending: List[Tuple[str, str, list]] = []
            for pod, model, events in batches:
                start = 0
                for i, ev in enumerate(events):
                    if not isinstance(ev, AllBlocksCleared):
                        continue
                    if i > start:
                        pending.append((pod, model, events[start:i]))
                    if pending:
                        apply(self, pending, token_processor)
                        pending = []
                    self.clear_pods([pod], model)
                    start = i + 1
                if start < len(events):
                    pending.append((pod, model, events[start:]))
            if pending:
                apply(self, pending, token_processor)
            return
        apply(self, batches, token_processor)

    def _apply_event_batches(self, batches: List[Tuple[str, str, list]],
                             token_processor=None) -> None:
        """flatten -> plan (both in event_batch.py) -> upload -> launch."""
        if token_processor is None:
            from .token_processor import ChunkedTokenDatabase

            token_processor = ChunkedTokenDatabase()
        # The kernels compute the request-key chain themselves, so they
        # must run the token processor's algorithm.  One without a native
        # id: raise, and kvevents.Pool falls back to its per-event path.
        hash_algo = token_processor.config.hash_algo
        algo_id = hashing.NATIVE_ALGO_IDS.get(hash_algo)
        if algo_id is None:
            raise ValueError(
                f"hash_algo {hash_algo!r} has no native chain kernel; "
                "apply these events through the per-event path")
        with self.registry.ids_shared():  # from interning to the launch
            GpuIndex._launch_event_batches(self, batches, token_processor,
                                           algo_id)

    def _launch_event_batches(self, batches, token_processor, algo_id):
        flat = flatten_event_batches(batches, self.registry)
        if flat is None:
            return
        block_size = token_processor.block_size
        route = plan_write_route(flat, block_size)
        up = _event_uploader(self)
        up.begin()
        d = _upload_events(flat, route, up, self.device)
        t = self.table
        head = (*t._t(), d.tokens, d.tok_off, d.ehashes, d.eh_off, d.parents,
                d.has_parent, d.ev_type, d.pod_entry)
        tail = (_to_i64(token_processor.config.init_hash()), block_size,
                t.next_epoch(), self.cfg.shard_id, self.cfg.num_shards)
        if route.op == "gpu_apply_events":
            t.ops.gpu_apply_events(*head, d.grp_off, d.model_of, *tail,
                                   algo_id)
        elif route.op == "gpu_apply_events_split":
            t.ops.gpu_apply_events_split(*head, d.grp_off, d.ev_of,
                                         d.model_of, *tail, algo_id)
        else:
            t.ops.gpu_apply_events_split_tr(*head, d.ev_of, d.model_of, *tail,
                                            route.max_tokens, algo_id)
        up.end()
