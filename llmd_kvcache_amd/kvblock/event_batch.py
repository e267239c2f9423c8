"""Host half of the on-device write path, numpy only and tested without a
GPU (tests/test_event_batch.py): flatten_event_batches turns a burst of
decoded KV events into the arrays the apply kernels read, plan_write_route
picks the kernel.  GpuIndex._apply_event_batches uploads and launches."""

from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import numpy as np

from ..kvevents.events import BlockRemoved, BlockStored, get_hash_as_uint64
from ..kvevents.pool import _tier

FIELDS = ("tokens", "tok_off", "ehashes", "eh_off", "parents", "has_parent",
          "ev_type", "pod_entry", "grp_off", "model_of")


class FlatEvents(SimpleNamespace):
    """One burst as parallel arrays, E events in G (pod, model) groups.

    tokens     int64 [sum tokens]   token ids of the stores, event by event
    tok_off    int32 [E+1]          event e's tokens (a remove has none)
    ehashes    int64 [sum hashes]   engine block hashes, u64 bits
    eh_off     int32 [E+1]          event e's hashes
    parents    int64 [E]            parent engine hash, u64 bits (0: none)
    has_parent uint8 [E]
    ev_type    uint8 [E]            0 store, 1 remove
    pod_entry  int32 [E]            (tier id << 24) | (pod id + 1)
    grp_off    int32 [G+1]          group g's events, in arrival order
    model_of   int32 [E]            model id (one launch applies all models)
    ev_of      int32 [sum hashes]   event of each hash; split routes only

    The same fields hold the device tensors once uploaded."""

    ev_of = None

    def event_of_hash(self) -> np.ndarray:
        counts = np.diff(self.eh_off)
        return np.repeat(np.arange(len(counts), dtype=np.int32), counts)


def _hashes_np(raw_list) -> np.ndarray:
    """Block-hash list -> u64 bits as int64; fast path for plain ints,
    per-element fallback for mixed/bytes forms (pool.go:343-367)."""
    try:
        return np.asarray(raw_list, dtype=np.uint64).view(np.int64)
    except (TypeError, ValueError, OverflowError):
        out = []
        for raw in raw_list:
            try:
                out.append(get_hash_as_uint64(raw))
            except Exception:
                continue
        return np.asarray(out, dtype=np.uint64).view(np.int64)


def flatten_event_batches(batches: List[Tuple[str, str, list]],
                          registry) -> Optional[FlatEvents]:
    """batches: (pod, model, [events]) in arrival order, grouped by (pod,
    model) in first-seen order; interns pods, models and tiers.  Malformed
    events are dropped whole, as _digest_block_stored / pool.go drop them
    (CPU and GPU replicas converge); AllBlocksCleared is skipped.  None
    when nothing survives."""
    by_pod: Dict[Tuple[str, str], list] = {}
    for pod, model, events in batches:
        by_pod.setdefault((pod, model), []).extend(events)

    # plain list appends, no per-event objects: this loop is ingest time
    token_arrays, hash_arrays = [], []
    n_tokens = n_hashes = 0
    tok_off, eh_off, grp_off = [0], [0], [0]
    parents, has_parent, ev_type, pod_entry, model_of = [], [], [], [], []

    for (pod, model), events in by_pod.items():
        model_id = registry.model_id(model)
        pod_id = registry.pod_id(pod)
        n_before = len(ev_type)
        for ev in events:
            # parse everything fallible BEFORE appending
            par = hp = 0
            if isinstance(ev, BlockStored):
                remove = 0
                if ev.parent_block_hash is not None:
                    try:
                        par = get_hash_as_uint64(ev.parent_block_hash)
                        hp = 1
                    except Exception:
                        continue  # drop event (bad parent hash)
            elif isinstance(ev, BlockRemoved):
                remove = 1
            else:
                continue  # AllBlocksCleared
            try:
                tier = registry.tier_id(_tier(ev.medium))
            except ValueError:
                continue  # drop event (tier registry full)
            hs = _hashes_np(ev.block_hashes)
            if hs.size == 0:
                continue
            hash_arrays.append(hs)
            n_hashes += hs.size
            eh_off.append(n_hashes)
            if not remove:
                toks = np.asarray(ev.token_ids, dtype=np.int64)
                token_arrays.append(toks)
                n_tokens += toks.size
            tok_off.append(n_tokens)
            parents.append(par)
            has_parent.append(hp)
            ev_type.append(remove)
            model_of.append(model_id)
            pod_entry.append((tier << 24) | (pod_id + 1))
        if len(ev_type) > n_before:
            grp_off.append(len(ev_type))

    if not ev_type:
        return None
    return FlatEvents(
        tokens=np.concatenate(token_arrays or [np.zeros(0, dtype=np.int64)]),
        tok_off=np.asarray(tok_off, dtype=np.int32),
        ehashes=np.concatenate(hash_arrays),
        eh_off=np.asarray(eh_off, dtype=np.int32),
        parents=np.asarray(parents, dtype=np.uint64).view(np.int64),
        has_parent=np.asarray(has_parent, dtype=np.uint8),
        ev_type=np.asarray(ev_type, dtype=np.uint8),
        pod_entry=np.asarray(pod_entry, dtype=np.int32),
        grp_off=np.asarray(grp_off, dtype=np.int32),
        model_of=np.asarray(model_of, dtype=np.int32),
    )


@dataclass
class WriteRoute:
    op: str             # the gpu_apply_events* op that applies the burst
    max_tokens: int     # longest event, the transposed route's image height
    tokens_int32: bool  # tokens go up as int32 bits (uint32 token ids)


def plan_write_route(flat: FlatEvents, block_size: int) -> WriteRoute:
    """Kernel selection, from host-side data only:
     - serial wave-per-group kernel when a burst both stores AND removes
       some engine hash (per-pod op order matters);
     - lane-per-EVENT transposed-chain kernel when no event's parent is
       another event of THIS burst (parents resolve via the engine map):
       8x the chain parallelism, coalesced int32 token loads, HALF the
       upload; the transpose runs on-device (numpy: ~2-5 ms/batch);
     - lane-per-group phase-split kernel otherwise."""
    if flat.ev_type.any():
        stored, removed = set(), set()
        eh_list = flat.ehashes.tolist()
        eh_off = flat.eh_off.tolist()
        for e, t in enumerate(flat.ev_type.tolist()):
            (removed if t else stored).update(eh_list[eh_off[e]:eh_off[e + 1]])
        if stored & removed:
            return WriteRoute("gpu_apply_events", 0, False)
    use_tr = block_size <= 64
    if use_tr and flat.has_parent.any():
        par = flat.parents[flat.has_parent.astype(bool)]
        use_tr = not np.isin(par, flat.ehashes).any()
    if not use_tr:
        return WriteRoute("gpu_apply_events_split", 0, False)
    return WriteRoute("gpu_apply_events_split_tr",
                      max(1, int(np.diff(flat.tok_off).max())), True)
