"""Pod census sweep (gpu_pod_census: k_pod_census + k_census_reduce + one
readback) beside the purge sweep with an empty bitmap (gpu_purge_pods:
k_purge_pods + its readback), which reads the same pods and meta bytes and
clears nothing, timed the same way in the same process.

Table: capacity 2^26 (or --log2cap), pods_per_key 10, about half full, the
table of profiles/r08_pod_purge.md (64 pods, every key held by 3 of them).
Three contents of that one table, in this order:

 - "even":   as built - every pod holds 3/64 of the keys, tier 0;
 - "skewed": 90 % of the non-empty entries rewritten to pod 0 (the
             same-address case for the LDS histogram);
 - "wide":   every non-empty entry rewritten to a uniform id below 4096
             and a uniform tier below 4, counted with 4096 x 4 bins (the
             64 KB histogram and the 511-workgroup grid).

Method: warm-up, then device events around each call (they enclose the
readback), alternating census and purge, median of the repeats.  The
census reads 48 B per slot (pods 40, meta 4, e_meta 4), the purge 44.

    python scripts/bench_pod_census.py [--out results.json] [--log2cap N]

--reduce-only BINS runs nothing but census calls with that many bins on an
empty 2^21 table, for a kernel trace: k_census_reduce's time depends on the
grid and the bins, not on what the table holds.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndexConfig,
    KvTable,
)

N_PODS = 64
HOLDERS = (0, 1, 7)  # key group g is held by pods g, g+1, g+7 (mod 64)
P = 10


def build(log2cap):
    cap = 1 << log2cap
    t = KvTable(GpuIndexConfig(capacity=cap, pods_per_key=P))
    g = torch.Generator(device="cuda")
    g.manual_seed(log2cap)
    per_group = cap // 2 // N_PODS
    for grp in range(N_PODS):
        h = torch.randint(1, 1 << 62, (per_group,), dtype=torch.int64,
                          device="cuda", generator=g)
        ents = torch.tensor([((grp + d) % N_PODS) + 1 for d in HOLDERS],
                            dtype=torch.int32, device="cuda")
        t.insert(h, h, 0, ents)
    torch.cuda.synchronize()
    return t


def rewrite(t, fn, seed):
    """pods[i] = fn(random int63) for the non-empty entries, in chunks."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    for chunk in t.pods.chunk(64):
        r = torch.randint(0, 1 << 62, chunk.shape, dtype=torch.int64,
                          device="cuda", generator=g)
        chunk.copy_(torch.where(chunk != 0, fn(r, chunk.to(torch.int64)),
                                torch.zeros_like(r)).to(torch.int32))
    torch.cuda.synchronize()


def skew(r, old):          # 90 %: pod 0, tier 0; the rest stay
    return torch.where(r % 10 < 9, torch.ones_like(r), old)


def widen(r, old):         # uniform id below 4096, uniform tier below 4
    return (((r >> 20) & 3) << 24) | ((r & 4095) + 1)


def time_pair(t, num_pods, n_tiers, warmup, reps):
    empty = torch.zeros(1, dtype=torch.int64, device="cuda")
    fns = {"census": lambda: t.pod_census(-1, num_pods, n_tiers),
           "purge_empty": lambda: t.purge_pods(empty, -1)}
    ms = {k: [] for k in fns}
    for i in range(warmup + reps):
        for name, fn in fns.items():  # alternating
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms[name].append(a.elapsed_time(b))
        if i == 0:
            assert tuple(out) == (0, 0)  # the empty bitmap clears nothing
    res = {k: {"median_ms": statistics.median(v), "min_ms": min(v),
               "max_ms": max(v)} for k, v in ms.items()}
    res["ratio"] = res["census"]["median_ms"] / res["purge_empty"]["median_ms"]
    cap = t.keys.numel()
    res["census_read_GBps"] = cap * (4 * P + 8) / res["census"]["median_ms"] / 1e6
    counts, summary = t.pod_census(-1, num_pods, n_tiers)
    res["summary"] = summary.tolist()
    res["largest_bin_share"] = float(counts.max()) / max(1, int(summary[3]))
    assert int(counts.sum()) + int(summary[4]) == int(summary[3])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2cap", type=int, default=26)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--reduce-only", type=int, default=0, metavar="BINS")
    args = ap.parse_args()
    if args.reduce_only:
        t = KvTable(GpuIndexConfig(capacity=1 << 21, pods_per_key=P))
        n_tiers = 4 if args.reduce_only >= 4 else 1
        for _ in range(50):
            t.pod_census(-1, args.reduce_only // n_tiers, n_tiers)
        return
    t = build(args.log2cap)
    result = {"device": torch.cuda.get_device_name(0),
              "capacity_log2": args.log2cap, "pods_per_key": P,
              "floor_ratio": (4 * P + 8) / (4 * P + 4)}
    result["even_64x2"] = time_pair(t, 64, 2, args.warmup, args.reps)
    rewrite(t, skew, 1)
    result["skewed_64x2"] = time_pair(t, 64, 2, args.warmup, args.reps)
    rewrite(t, widen, 2)
    result["wide_4096x4"] = time_pair(t, 4096, 4, args.warmup, args.reps)
    result["wide_counted_64x2"] = time_pair(t, 64, 2, args.warmup, args.reps)
    blob = json.dumps(result, indent=1)
    print(blob)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(blob)


if __name__ == "__main__":
    main()
