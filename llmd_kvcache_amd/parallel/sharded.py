"""Multi-GPU sharded index with RCCL mask merging over xGMI.

The reference has no collectives - its global
index is one shared store.  The MI355X-native design shards the
block->pod table across the 8 GPUs of one node and merges per-shard
lookup results with RCCL (torch.distributed backend "nccl" IS RCCL on
ROCm); CPU tests use gloo with the identical code path.

Design:
 - ownership: chunk_hash % world_size == rank; the engine->request map is
   REPLICATED on every rank (it is tiny - 24 B/entry - and replication
   makes parent-chain stitching (kvevents/pool.go:279-296) rank-local);
 - writes: every rank applies the full event stream; the insert kernels
   filter main-table stores by ownership (ops cpu_insert/gpu_insert
   shard args);
 - reads: every rank probes ALL keys of the batch against its shard
   (misses for unowned keys are ~1 HBM read), producing per-key per-tier
   pod bitmasks [K, T, W] that must be merged across shards (SUM == OR:
   shards are disjoint).

Mask-merge data volume (measured, not "small"): a single prompt is
K*T*W*8 bytes (512 keys x 2 tiers x 1 word = 8 KB - latency-bound), but
at the flagship batch (32768 prompts x 512 keys) the mask tensor is
~268 MB per call - BANDWIDTH-bound on xGMI (7 p2p links x ~153 GB/s).
Two merge strategies, chosen by payload size and backend:
 - small batches: one all_reduce (1 collective, lowest latency);
 - large batches on RCCL: prompt-partitioned reduce_scatter - each rank
   receives only the merged masks for ITS contiguous prompt slice
   ((N-1)/N of the volume moved ONCE instead of twice for all_reduce),
   walks that slice (the longest-prefix walk itself now scales across
   ranks), and an all_gather of the per-prompt score rows ([B, P] float
   ~ 8 MB at the flagship shape, 32x smaller than the masks) rebuilds
   the full result everywhere.

Failure semantics: every rank participates in the merge collective
exactly once per call even when its LOCAL probe throws (zero masks +
an error flag riding in the same tensor); peers then raise instead of
returning silently-degraded scores, and no rank is ever left blocked in
the collective (tests/test_sharded.py follower-failure test).
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence, Set, Tuple

import torch
import torch.distributed as dist

from ..kvblock.gpu_index import TableIndex, TableIndexConfig, _to_i64

# payload threshold for switching all_reduce -> reduce_scatter+all_gather
# (below this the extra collective's latency dominates its volume saving)
REDUCE_SCATTER_MIN_BYTES = 8 << 20


class ShardedIndex:
    """Data-parallel sharded table over an initialized process group."""

    def __init__(
        self,
        cfg: Optional[TableIndexConfig] = None,
        group: Optional[dist.ProcessGroup] = None,
    ):
        if not dist.is_initialized():
            raise RuntimeError(
                "ShardedIndex requires torch.distributed to be initialized"
            )
        self.group = group
        self.rank = dist.get_rank(group)
        self.world_size = dist.get_world_size(group)
        cfg = cfg or TableIndexConfig()
        cfg.shard_id = self.rank
        cfg.num_shards = self.world_size
        self.local = TableIndex(cfg)
        self.device = self.local.device
        self.registry = self.local.registry
        # Testing hook: force the reduce_scatter merge strategy even on
        # small payloads / non-NCCL backends (gloo lacks
        # reduce_scatter_tensor; _merge_reduce_scatter then emulates it
        # with all_reduce+slice so the partition/flag/gather logic is
        # CPU-testable).  Must be set identically on every rank.
        self.force_reduce_scatter = False

    # -- write path ----------------------------------------------------
    def add(self, engine_keys, request_keys, entries) -> None:
        """Every rank calls this with the SAME arguments (replicated event
        stream); the shard filter in the insert op keeps only owned keys."""
        self.local.add(engine_keys, request_keys, entries)

    def evict(self, engine_key, entries) -> None:
        self.local.evict(engine_key, entries)

    def get_request_key(self, engine_key):
        return self.local.get_request_key(engine_key)

    def apply_event_batches(self, batches, token_processor=None,
                            clear_on_all_blocks_cleared: bool = False) -> None:
        if clear_on_all_blocks_cleared:
            self.local.apply_event_batches(batches, token_processor,
                                           clear_on_all_blocks_cleared=True)
        else:
            self.local.apply_event_batches(batches, token_processor)

    def clear_pods(self, pods, model_name=None) -> dict:
        """Purge the LOCAL shard.  Like add/evict, every rank calls this
        with the same arguments at the same point of the op order; the
        counts are this shard's."""
        return self.local.clear_pods(pods, model_name)

    def retire_pods(self, pods, compact: bool = False) -> dict:
        """Purge the local shard and release the ids.  Registries are
        replicated, so every rank must retire the same pods at the same
        point of the op order (ShardedIndexService broadcasts it):
        lowest-free id reuse then assigns the same ids everywhere."""
        if compact:
            return self.local.retire_pods(pods, compact=True)
        return self.local.retire_pods(pods)

    def compact_pod_ids(self) -> dict:
        """Renumber the pods of the LOCAL shard and its registry.  The
        plan is a pure function of the registry and registries are
        replicated, so ranks that call this at the same point of the op
        order end up with the same ids; the counts are this shard's."""
        return self.local.compact_pod_ids()

    # -- read path -----------------------------------------------------
    def sharded_scores(
        self,
        hashes: torch.Tensor,
        offsets: torch.Tensor,
        model_name: str,
        pod_identifier_set: Set[str],
        weights: Optional[torch.Tensor] = None,
    ) -> torch.Tensor:
        """Batched scores for B prompts: local shard probe -> collective
        mask merge -> longest-prefix walk.  All ranks return the same
        [B, num_pods] float tensor.  hashes/offsets may live on any
        device; the device moves happen inside the guarded region.

        Collective-participation guarantee: every rank enters the merge
        collective exactly once per call.  A rank whose local probe (or
        device staging) throws contributes zero masks plus an error flag
        carried IN the merge tensor; after the merge every rank sees the
        flag and raises - no silently-degraded scores, no rank blocked
        in a collective.  The strategy choice (all_reduce vs
        reduce_scatter) depends only on symmetric quantities (K, B,
        world, backend, registry shape), so all ranks always pick the
        same collective sequence."""
        K = int(hashes.numel())
        B = int(offsets.numel()) - 1
        n_tiers = max(1, len(self.local.registry.id_to_tier))
        num_pods = self.local._num_pods_padded()
        W = (num_pods + 63) // 64

        local_err: Optional[BaseException] = None
        masks: Optional[torch.Tensor] = None
        try:
            if weights is None:
                weights = self.local.tier_weights()  # device alloc: guarded
            hashes = hashes.to(device=self.device)
            model_id = self.registry.model_id(model_name)
            filt = self.local._filter_tensor(pod_identifier_set, num_pods)
            found, masks = self.local.table.lookup(
                hashes, model_id, filt, num_pods, n_tiers=n_tiers)
            del found  # chain-cut semantics handled by the scoring walk
        except BaseException as e:  # noqa: BLE001 - re-raised below
            local_err = e

        offs_cpu = offsets.to(dtype=torch.int32, device="cpu")
        payload = K * n_tiers * W * 8
        use_rs = self.world_size > 1 and B >= self.world_size and (
            self.force_reduce_scatter
            or (payload >= REDUCE_SCATTER_MIN_BYTES
                and dist.get_backend(self.group) == "nccl")
        )
        if use_rs:
            scores = self._merge_reduce_scatter(
                masks, offs_cpu, weights, num_pods, n_tiers, W, K, B,
                local_err is not None)
        else:
            scores = self._merge_all_reduce(
                masks, offs_cpu, weights, num_pods, n_tiers, W, K,
                local_err is not None)
        if local_err is not None:
            raise local_err
        if scores is None:
            raise RuntimeError(
                "sharded score failed on a peer rank (its shard probe "
                "threw); the request must be retried - merged masks "
                "would be missing that shard's blocks")
        return scores

    def _merge_all_reduce(self, masks, offs_cpu, weights, num_pods,
                          n_tiers, W, K, failed: bool):
        """One all_reduce of [K*T*W + 1] (the +1 is the error flag).
        Returns [B, num_pods] scores, or None if any rank flagged."""
        dev = self.local.table.keys.device
        buf = torch.zeros(K * n_tiers * W + 1, dtype=torch.int64, device=dev)
        if failed:
            buf[-1] = 1
        elif K:
            buf[: K * n_tiers * W].copy_(masks.reshape(-1))
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
        if failed:
            return None
        if int(buf[-1].item()) != 0:
            return None
        merged = buf[: K * n_tiers * W].view(K, n_tiers, W)
        return self._walk(merged, offs_cpu, weights, num_pods)

    def _merge_reduce_scatter(self, masks, offs_cpu, weights, num_pods,
                              n_tiers, W, K, B, failed: bool):
        """Large-batch merge: prompts partitioned into world_size
        contiguous groups (balanced by key count); reduce_scatter hands
        each rank the merged masks for ITS group only ((N-1)/N of the
        mask volume moved once, vs twice for all_reduce); each rank walks
        its group (parallelizing the walk) and an all_gather of the small
        [B_r, P] score rows rebuilds the full result on every rank."""
        dev = self.local.table.keys.device
        TW = n_tiers * W
        bounds = _partition_prompts(offs_cpu, self.world_size)
        kmax = max(
            int(offs_cpu[bounds[r + 1]]) - int(offs_cpu[bounds[r]])
            for r in range(self.world_size)
        )
        bmax = max(bounds[r + 1] - bounds[r] for r in range(self.world_size))
        seg = kmax * TW + 1  # +1: per-segment error flag
        buf = torch.zeros(self.world_size * seg, dtype=torch.int64,
                          device=dev)
        if failed:
            buf.view(self.world_size, seg)[:, -1] = 1
        else:
            flat = masks.reshape(K, TW)
            bview = buf.view(self.world_size, seg)
            for r in range(self.world_size):
                k_lo = int(offs_cpu[bounds[r]])
                k_hi = int(offs_cpu[bounds[r + 1]])
                if k_hi > k_lo:
                    bview[r, : (k_hi - k_lo) * TW].copy_(
                        flat[k_lo:k_hi].reshape(-1))
        out = torch.empty(seg, dtype=torch.int64, device=dev)
        if dist.get_backend(self.group) == "nccl":
            dist.reduce_scatter_tensor(out, buf, op=dist.ReduceOp.SUM,
                                       group=self.group)
        else:
            # gloo has no reduce_scatter_tensor: emulate (same result,
            # more traffic) so CPU tests exercise this exact code path
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
            out.copy_(buf.view(self.world_size, seg)[self.rank])

        # score rows for this rank's prompt group (+1 flag row)
        P = num_pods
        my = torch.zeros(bmax + 1, P, dtype=torch.float32, device=dev)
        peer_failed = int(out[-1].item()) != 0
        if failed or peer_failed:
            my[bmax, 0] = 1.0
        else:
            r = self.rank
            b_lo, b_hi = bounds[r], bounds[r + 1]
            k_lo = int(offs_cpu[b_lo])
            k_hi = int(offs_cpu[b_hi])
            try:
                if b_hi > b_lo:
                    merged = out[: (k_hi - k_lo) * TW].view(
                        k_hi - k_lo, n_tiers, W)
                    local_offs = (offs_cpu[b_lo: b_hi + 1] - k_lo).to(
                        torch.int32)
                    my[: b_hi - b_lo].copy_(
                        self._walk(merged, local_offs, weights, num_pods))
            except BaseException:
                my.zero_()
                my[bmax, 0] = 1.0
        gathered = [torch.empty_like(my) for _ in range(self.world_size)]
        dist.all_gather(gathered, my, group=self.group)
        if any(float(g[bmax, 0].item()) != 0.0 for g in gathered):
            return None
        rows = [
            gathered[r][: bounds[r + 1] - bounds[r]]
            for r in range(self.world_size)
        ]
        return torch.cat(rows, dim=0)

    def _walk(self, masks, offs_cpu, weights, num_pods):
        """Longest-prefix walk over merged masks -> [B, num_pods]."""
        if self.local.table.is_cuda:
            return self.local.table.ops.gpu_score_from_masks(
                masks.contiguous(), offs_cpu.to(self.device), weights,
                num_pods)
        return self.local.table.ops.cpu_score_from_masks(
            masks.contiguous(), offs_cpu, weights.cpu(), num_pods)

    def score_keys(
        self, request_keys: Sequence, pod_identifier_set: Set[str]
    ) -> Dict[str, float]:
        """Single-prompt convenience wrapper (Key objects in, {pod: score}
        out) - the sharded analog of Indexer.get_pod_scores steps 3-4."""
        if not request_keys:
            return {}
        hashes = torch.tensor(
            [_to_i64(k.chunk_hash) for k in request_keys],
            dtype=torch.int64,
            device=self.device,
        )
        offsets = torch.tensor([0, len(request_keys)], dtype=torch.int32)
        with self.registry.ids_shared():
            scores = self.sharded_scores(
                hashes, offsets, request_keys[0].model_name,
                pod_identifier_set
            )
            return self.local.scores_to_map(scores)[0]


def _partition_prompts(offs_cpu: torch.Tensor, world: int) -> Tuple[int, ...]:
    """Contiguous prompt-group boundaries (length world+1) balancing key
    counts across ranks: bounds[r]..bounds[r+1] are rank r's prompts.
    Deterministic from (offsets, world) so every rank computes the same
    partition without communicating."""
    B = int(offs_cpu.numel()) - 1
    total = int(offs_cpu[B])
    bounds = [0]
    for r in range(1, world):
        target = total * r // world
        # first prompt boundary whose cumulative key count reaches target
        b = int(torch.searchsorted(
            offs_cpu[1:].to(torch.int64), target, right=False)) + 1
        b = min(max(b, bounds[-1]), B)
        bounds.append(b)
    bounds.append(B)
    return tuple(bounds)


def registry_fingerprint(registry) -> int:
    """Order-sensitive FNV-1a fingerprint of the interned id spaces.

    Mask merging assumes pod/model/tier ids agree on every rank (the
    replicated event stream assigns them identically).  If a rank ever
    diverged - an error path that dropped one event, a locally-registered
    extra pod - merged masks would silently attribute hits to the wrong
    pods.  ROADMAP #8: detect loudly instead."""
    from ..utils.hashing import fnv1a_64

    acc = b"\x00".join(
        "\x1f".join(ns).encode("utf-8")
        for ns in (registry.id_to_pod, registry.id_to_model,
                   registry.id_to_tier)
    )
    return fnv1a_64(acc)


def check_registry_sync(index, group=None) -> None:
    """Raise on cross-rank registry divergence (call between batches -
    it is one tiny all_gather, latency-bound)."""
    fp = registry_fingerprint(index.registry)
    world = dist.get_world_size(group)
    fps = [None] * world
    dist.all_gather_object(fps, fp, group=group)
    if any(f != fps[0] for f in fps):
        raise RuntimeError(
            f"registry divergence across ranks (fingerprints {fps}): "
            "pod/model/tier id spaces no longer agree - scores from "
            "merged masks would be misattributed. A rank dropped or "
            "reordered events; rebuild the index from the stream."
        )
