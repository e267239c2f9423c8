#!/usr/bin/env python
"""Call time of GpuIndex.apply_event_batches on bursts with batch-local
parents: the linked wave chain (event_chain_layout "linked") against the
lane-per-group kernel (gpu_apply_events_split, what "rect" plans for them).

  depthD      64 groups x one chain of D one-block events, block size 16:
              event d's parent is event d - 1's block (D levels)
  wide16      8192 events of 1..8 blocks over 64 pods at block size 16;
              every second event of a pod chains from the last block of
              the one before it (2 levels)
  wide128     the same events at block size 128
  mixed16     8192 one-block events plus one of 2048 blocks, block size 16,
              linked in the same way (the long one is a child)

Per (burst, hash, layout): the op that ran, the median, quartiles, minimum
and maximum of `reps` calls (host clock around apply_event_batches and a
device synchronise; the layouts alternate call by call).  The cap is lifted
(event_link_max_levels = 1 << 20), so "linked" always takes the new op and
the depth rows show where it stops paying.  One JSON line per row on
stdout; --out appends them to a file as well.

A checkout without the layout (an earlier commit) is measured with
--layouts rect, which then passes no layout at all.  One process, one
GPU."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex, GpuIndexConfig)
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    ChunkedTokenDatabase, TokenProcessorConfig)
from llmd_kvcache_amd.kvevents.events import BlockStored  # noqa: E402

PODS = 64
DEPTHS = (1, 2, 4, 8, 16, 32, 64)
LONG_AT = 4064  # pod 32's 64th event: an odd one, so a child
WIDE = {  # name -> (block size, blocks per event)
    "wide16": (16, lambda i: 1 + i % 8),
    "wide128": (128, lambda i: 1 + i % 8),
    "mixed16": (16, lambda i: 2048 if i == LONG_AT else 1),
}
BURSTS = tuple(f"depth{d}" for d in DEPTHS) + tuple(WIDE)


def make_burst(name, events):
    rng = np.random.default_rng(7)
    per_pod = [[] for _ in range(PODS)]
    next_hash = 1 << 20

    def store(pod, n, bs, child):
        nonlocal next_hash
        parent = per_pod[pod][-1].block_hashes[-1] if child else None
        per_pod[pod].append(BlockStored(
            list(range(next_hash, next_hash + n)), parent,
            rng.integers(0, 1 << 32, n * bs, dtype=np.int64), bs))
        next_hash += n

    if name.startswith("depth"):
        bs = 16
        for d in range(int(name[5:])):
            for pod in range(PODS):
                store(pod, 1, bs, d > 0)
    else:
        bs, blocks = WIDE[name]
        for i in range(events + (name == "mixed16")):
            store(i % PODS, blocks(i), bs, (i // PODS) % 2 == 1)
    return bs, [(f"pod-{p}", "m", evs) for p, evs in enumerate(per_pod)]


class LastOp:
    """Passes a table's ops through and keeps the last event op's name."""

    def __init__(self, mod):
        self._mod = mod
        self.last = None

    def __getattr__(self, name):
        if name.startswith("gpu_apply_events"):
            self.last = name
        return getattr(self._mod, name)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--bursts", default=",".join(BURSTS))
    ap.add_argument("--algos", default="fnv-64a,sha256-cbor-64")
    ap.add_argument("--layouts", default="rect,linked")
    ap.add_argument("--events", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--capacity-log2", type=int, default=21)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_event_links.py needs a GPU")
    layouts = args.layouts.split(",")
    only_rect = layouts == ["rect"]

    for name in args.bursts.split(","):
        bs, batches = make_burst(name, args.events)
        for algo in args.algos.split(","):
            tp = ChunkedTokenDatabase(TokenProcessorConfig(
                block_size=bs, hash_algo=algo))
            worlds = {}
            for layout in layouts:
                kw = {} if only_rect else {"event_chain_layout": layout,
                                           "event_link_max_levels": 1 << 20}
                idx = GpuIndex(GpuIndexConfig(
                    capacity=1 << args.capacity_log2, pods_per_key=4, **kw))
                idx.table.ops = LastOp(idx.table.ops)
                worlds[layout] = idx
            times = {layout: [] for layout in layouts}
            for rep in range(args.warmup + args.reps):
                for layout, idx in worlds.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    idx.apply_event_batches(batches, tp)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if rep >= args.warmup:
                        times[layout].append(dt * 1e3)
            for layout, idx in worlds.items():
                t = sorted(times[layout])
                q = statistics.quantiles(t, n=4)
                row = dict(label=args.label, burst=name, block_size=bs,
                           algo=algo, layout=layout, op=idx.table.ops.last,
                           reps=len(t), median_ms=round(q[1], 3),
                           q1_ms=round(q[0], 3), q3_ms=round(q[2], 3),
                           min_ms=round(t[0], 3), max_ms=round(t[-1], 3))
                line = json.dumps(row)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")
            del worlds
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
