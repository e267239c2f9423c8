"""Purge-by-pod sweep (gpu_purge_pods / k_purge_pods) against two
yardsticks timed the same way in the same run:

 - ``pods.clone()``: reads and writes the array the sweep only reads, so
   it moves twice the bytes - the sweep should not be slower;
 - ``gpu_evict`` with the pod's engine hashes: the only removal there was
   before the sweep existed.

Table: capacity 2^21 and 2^26, pods_per_key 10, about half full, 64 pods
(every key held by 3 of them, every pod holding 3/64 of the keys).
Method: warm-up, then device events around each call, median of the
repeats.  The repeated figures are taken on a quiescent table (the pod is
already gone: the sweep reads everything and clears nothing); the one
call that really removes a pod is timed once, for the sweep and for
gpu_evict each on a pod of its own.

Also prints the read-path effect the sweep is for: pod words W and
k_fused_score LDS bytes (512 keys, 2 tiers) of a fleet with 8 live pods
before and after retiring 512 dead ones, and the time of one score call.

    python scripts/bench_pod_purge.py [--out results.json] [--small]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex,
    GpuIndexConfig,
    KvTable,
    _to_i64,
)
from llmd_kvcache_amd.kvblock.keys import Key, PodEntry  # noqa: E402

N_PODS = 64
HOLDERS = (0, 1, 7)  # key group g is held by pods g, g+1, g+7 (mod 64)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def once(fn):
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def words_for(pid):
    return torch.tensor([_to_i64(1 << pid)], dtype=torch.int64, device="cuda")


def bench_capacity(log2cap, warmup, reps):
    cap = 1 << log2cap
    P = 10
    t = KvTable(GpuIndexConfig(capacity=cap, pods_per_key=P))
    n_keys = cap // 2
    per_group = n_keys // N_PODS
    g = torch.Generator(device="cuda")
    g.manual_seed(log2cap)
    groups = []
    for grp in range(N_PODS):
        h = torch.randint(1, 1 << 62, (per_group,), dtype=torch.int64,
                          device="cuda", generator=g)
        ents = torch.tensor([((grp + d) % N_PODS) + 1 for d in HOLDERS],
                            dtype=torch.int32, device="cuda")
        t.insert(h, h, 0, ents)
        groups.append(h)
    torch.cuda.synchronize()
    live = int(((t.meta < 0) & ((t.meta & 0x40000000) == 0)).sum())

    def hashes_of(pid):
        return torch.cat([groups[(pid - d) % N_PODS] for d in HOLDERS])

    res = {"capacity_log2": log2cap, "pods_per_key": P, "live_keys": live,
           "pods_bytes": cap * P * 4}
    # the real removals, once each, on pods 5 (sweep) and 20 (gpu_evict);
    # both kernels have run once before (a sweep with no bit set, an
    # evict of a hash nobody stored), so neither pays its first launch
    w5 = words_for(5)  # on the device already: no upload inside a timing
    t.purge_pods(torch.zeros(1, dtype=torch.int64, device="cuda"), -1)
    t.evict(torch.tensor([12345], dtype=torch.int64, device="cuda"), 0,
            torch.tensor([21], dtype=torch.int32, device="cuda"))
    ms, out = once(lambda: t.purge_pods(w5, -1))
    res["sweep_real_ms"] = ms
    res["sweep_real_counts"] = list(out)
    eh = hashes_of(20)
    ent20 = torch.tensor([21], dtype=torch.int32, device="cuda")
    ms, _ = once(lambda: t.evict(eh, 0, ent20))
    res["evict_real_ms"] = ms
    res["evict_hashes"] = int(eh.numel())
    left = int(((t.pods & 0xFFFFFF) == 21).sum())
    res["evict_left_entries"] = left
    # quiescent repeats
    res["sweep_ms"] = timed(lambda: t.purge_pods(w5, -1), warmup, reps)
    res["clone_ms"] = timed(lambda: t.pods.clone(), warmup, reps)
    # what the op's counter readback alone costs inside such a window: a
    # device-to-host copy of the size of the per-workgroup counters
    part = torch.zeros(2048, 2, dtype=torch.int32, device="cuda")
    res["readback_ms"] = timed(lambda: part.cpu(), warmup, reps)
    res["evict_replay_ms"] = timed(lambda: t.evict(eh, 0, ent20),
                                   warmup, reps)
    med = res["sweep_ms"][0]
    res["sweep_read_GBps"] = (cap * P * 4 + cap * 4) / med / 1e6
    res["clone_rw_GBps"] = 2 * cap * P * 4 / res["clone_ms"][0] / 1e6
    del t, groups
    torch.cuda.empty_cache()
    return res


def bench_width(warmup, reps, live_first):
    """8 live pods among 512 dead ones: W and the score route before and
    after retire_pods.  live_first: the live pods are the oldest names
    (lowest ids), so the dead ones trail and are trimmed at once; else the
    live pods are the newest (highest ids) and W shrinks only when they
    in turn are replaced ("next_rollout": retire them, 8 new names)."""
    idx = GpuIndex(GpuIndexConfig(capacity=1 << 16, pods_per_key=10))
    n_tiers = max(1, len(idx.registry.id_to_tier))
    K, B = 512, 64
    keys = [Key("m", 1000 + i) for i in range(K)]
    dead = [f"dead-{i}" for i in range(512)]
    livep = [f"live-{i}" for i in range(8)]

    def add_live(names):
        for p in names:
            idx.add(keys, keys, [PodEntry(p, "gpu")])

    if live_first:
        add_live(livep)
    for i, p in enumerate(dead):  # names seen once, long gone
        idx.add(keys[i:i + 1], keys[i:i + 1], [PodEntry(p, "gpu")])
    if not live_first:
        add_live(livep)
    hashes = torch.tensor([_to_i64(k.chunk_hash) for k in keys] * B,
                          dtype=torch.int64, device="cuda")
    offs = torch.arange(0, (B + 1) * K, K, dtype=torch.int32, device="cuda")

    def shape():
        n = idx._num_pods_padded()
        W = (n + 63) // 64
        lds = K * n_tiers * W * 8
        return {"num_pods_padded": n, "W": W, "n_tiers": n_tiers,
                "fused_score_lds_bytes": lds, "fused_route": lds <= 64 * 1024}

    def score():
        return idx.fused_scores(hashes, offs, "m", set(), max_k=K)

    out = {"live_first": live_first, "keys_per_prompt": K, "prompts": B,
           "before": shape()}
    out["before"]["score_ms"] = timed(score, warmup, reps)
    ms, counts = once(lambda: idx.retire_pods(dead))
    out["retire_ms"] = ms
    out["retire_counts"] = {k: v for k, v in counts.items() if k != "pods"}
    out["after"] = shape()
    out["after"]["score_ms"] = timed(score, warmup, reps)
    top = idx.scores_to_map(score())[0]
    out["after"]["pods_scored"] = len(top)
    if not live_first:
        idx.retire_pods(livep)
        add_live([f"new-{i}" for i in range(8)])
        out["next_rollout"] = shape()
        out["next_rollout"]["score_ms"] = timed(score, warmup, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true",
                    help="2^16 and 2^18 slots (a quick functional pass)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    caps = (16, 18) if args.small else (21, 26)
    result = {
        "device": torch.cuda.get_device_name(0),
        "sweeps": [bench_capacity(c, args.warmup, args.reps) for c in caps],
        "width": [bench_width(args.warmup, args.reps, order)
                  for order in (True, False)],
    }
    blob = json.dumps(result, indent=1)
    print(blob)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(blob)


if __name__ == "__main__":
    main()
