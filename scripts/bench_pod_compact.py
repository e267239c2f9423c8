"""Pod-id remap sweep (gpu_remap_pods / k_remap_pods) and what
compact_pod_ids buys the read path, each against yardsticks timed the
same way in the same run.

The sweep.  Table: capacity 2^21 and 2^26, pods_per_key 10, about half
full, 64 pods, every key held by 3 of them (the table of
bench_pod_purge.py).  Four things are timed:

 - ``k_purge_pods`` on a quiescent table (reads everything, clears
   nothing) - the existing sweep of the same shape;
 - ``pods.clone()`` - reads and writes the array once;
 - ``remap_pods`` with the identity map - reads everything, writes nothing;
 - ``remap_pods`` with a map that moves every id.  A renumbering can run
   once per table state only, so the calls alternate between a map m
   (a rotation of the 64 ids) and its inverse.

Method: three warm-ups, then device events around each of 15 calls;
median (min .. max).  The maps are on the device before the timing
starts; each remap call includes the op's own validation readback of the
map and its counter readback, as each purge call includes its counter
readback.

The read path.  8 live pods on the highest ids after 512 retired names,
2 tiers, 64 prompts x 512 keys: W, k_fused_score LDS bytes, route and
score-call time before and after compact_pod_ids(), the time of the
compaction call, and the same fleet with its live pods on the lowest ids
as the yardstick.

    python scripts/bench_pod_compact.py [--out results.json] [--small]
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_pod_purge import HOLDERS, N_PODS, once, timed  # noqa: E402

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex,
    GpuIndexConfig,
    KvTable,
    _to_i64,
)
from llmd_kvcache_amd.kvblock.keys import Key, PodEntry  # noqa: E402


def bench_capacity(log2cap, warmup, reps):
    cap = 1 << log2cap
    P = 10
    t = KvTable(GpuIndexConfig(capacity=cap, pods_per_key=P))
    per_group = cap // 2 // N_PODS
    g = torch.Generator(device="cuda")
    g.manual_seed(log2cap)
    for grp in range(N_PODS):
        h = torch.randint(1, 1 << 62, (per_group,), dtype=torch.int64,
                          device="cuda", generator=g)
        ents = torch.tensor([((grp + d) % N_PODS) + 1 for d in HOLDERS],
                            dtype=torch.int32, device="cuda")
        t.insert(h, h, 0, ents)
    torch.cuda.synchronize()
    entries = int((t.pods != 0).sum())
    res = {"capacity_log2": log2cap, "pods_per_key": P,
           "pods_bytes": cap * P * 4, "entries": entries,
           "nonzero_vec16_frac": float(
               (t.pods.view(-1, 4) != 0).any(dim=1).float().mean())}

    def dev(ids):
        return torch.tensor(ids, dtype=torch.int32, device="cuda")

    remap = t.ops.gpu_remap_pods
    ident = dev(list(range(N_PODS)))
    fwd = dev([(i + 1) % N_PODS for i in range(N_PODS)])
    inv = dev([(i - 1) % N_PODS for i in range(N_PODS)])
    none = torch.zeros(1, dtype=torch.int64, device="cuda")
    turn = [0]

    def moved():
        turn[0] ^= 1
        return remap(*t._t(), fwd if turn[0] else inv)

    # what one all-moved call reports (and its inverse puts it back)
    res["moved_counts"] = list(moved())
    moved()
    assert turn[0] == 0
    before = t.pods.clone()
    res["purge_quiescent_ms"] = timed(lambda: t.purge_pods(none, -1),
                                      warmup, reps)
    res["clone_ms"] = timed(lambda: t.pods.clone(), warmup, reps)
    res["remap_identity_ms"] = timed(lambda: remap(*t._t(), ident),
                                     warmup, reps)
    assert (warmup + reps) % 2 == 0, "m and its inverse must pair up"
    res["remap_all_moved_ms"] = timed(moved, warmup, reps)
    res["table_restored"] = bool(torch.equal(before, t.pods))
    # the readbacks inside a remap call: the map in, the counters out
    part = torch.zeros(2048, 3, dtype=torch.int32, device="cuda")
    res["readbacks_ms"] = timed(lambda: (ident.cpu(), part.cpu()),
                                warmup, reps)
    rd = cap * P * 4 + cap * 4
    res["purge_read_GBps"] = rd / res["purge_quiescent_ms"][0] / 1e6
    res["identity_read_GBps"] = rd / res["remap_identity_ms"][0] / 1e6
    res["clone_rw_GBps"] = 2 * cap * P * 4 / res["clone_ms"][0] / 1e6
    wr = res["nonzero_vec16_frac"] * cap * P * 4
    res["all_moved_rw_GBps"] = (rd + wr) / res["remap_all_moved_ms"][0] / 1e6
    del t, before
    torch.cuda.empty_cache()
    return res


def bench_width(warmup, reps, live_first):
    """8 live pods and 512 retired names.  live_first: the live pods hold
    the lowest ids (retire_pods alone trims the width - the yardstick);
    else they hold the highest and only compact_pod_ids() gives the width
    back."""
    idx = GpuIndex(GpuIndexConfig(capacity=1 << 16, pods_per_key=10))
    n_tiers = max(1, len(idx.registry.id_to_tier))
    K, B = 512, 64
    keys = [Key("m", 1000 + i) for i in range(K)]
    dead = [f"dead-{i}" for i in range(512)]
    livep = [f"live-{i}" for i in range(8)]

    def add_live():
        for p in livep:
            idx.add(keys, keys, [PodEntry(p, "gpu")])

    if live_first:
        add_live()
    for i, p in enumerate(dead):
        idx.add(keys[i:i + 1], keys[i:i + 1], [PodEntry(p, "gpu")])
    if not live_first:
        add_live()
    hashes = torch.tensor([_to_i64(k.chunk_hash) for k in keys] * B,
                          dtype=torch.int64, device="cuda")
    offs = torch.arange(0, (B + 1) * K, K, dtype=torch.int32, device="cuda")

    def shape():
        n = idx._num_pods_padded()
        W = (n + 63) // 64
        lds = K * n_tiers * W * 8
        return {"num_pods_padded": n, "W": W, "n_tiers": n_tiers,
                "fused_score_lds_bytes": lds,
                "route": ("k_fused_score" if lds <= 64 * 1024
                          else "lookup + score_from_masks")}

    def score():
        return idx.fused_scores(hashes, offs, "m", set(), max_k=K)

    out = {"live_first": live_first, "keys_per_prompt": K, "prompts": B}
    idx.retire_pods(dead)
    out["after_retire"] = shape()
    out["after_retire"]["score_ms"] = timed(score, warmup, reps)
    want = idx.scores_to_map(score())[0]
    ms, counts = once(idx.compact_pod_ids)
    out["compact_ms"] = ms
    out["compact_counts"] = counts
    out["after_compact"] = shape()
    out["after_compact"]["score_ms"] = timed(score, warmup, reps)
    out["scores_by_name_unchanged"] = idx.scores_to_map(score())[0] == want
    out["pods_scored"] = len(want)
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
