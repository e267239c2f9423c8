"""Device-chain layouts, measured: Indexer.score_flat_tokens on a GpuIndex
with host int64 tokens under two configurations, alternating within one
process (profiles/r14_ragged_chain.md).

    python scripts/bench_ragged_chain.py [--shapes served,long1,big]
    rocprofv3 --kernel-trace --stats -d DIR -- \\
        python scripts/bench_ragged_chain.py --profile fnv-64a:served:ragged

Shapes (block size 16, fixed seed):
  served  4096 prompts of 1024..8192 tokens: "padded" against "ragged"
  long1   4095 prompts of 1024 tokens and one of 131072
  big     32768 prompts of 1024..8192 tokens and one of 16384
The padded image of long1 and big is over device_chain_max_image_bytes:
"padded" then takes the CPU chain, which "over_cap" is measured against.
Each window runs calls for at least --window seconds and ends in a
synchronise; one JSON line per (algo, shape) with the median and the
min..max of the windows of either side.
"""
import argparse
import json
import statistics
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])

import numpy as np
import torch

from bench_read_routes import BS, make_world, window
from llmd_kvcache_amd.indexer import Config, Indexer, plan_read_route
from llmd_kvcache_amd.kvblock.token_processor import TokenProcessorConfig

SHAPES = {  # name: (prompts of 1024..hi tokens, hi, one extra prompt, sides)
    "served": (4096, 8192, 0, ("padded", "ragged")),
    "long1": (4095, 1024, 131072, ("padded", "over_cap")),
    "big": (32768, 8192, 16384, ("padded", "over_cap")),
}


def make_batch(shape, seed=7):
    n, hi, extra, _ = SHAPES[shape]
    rng = np.random.default_rng(seed)
    lens = rng.integers(1024, hi + 1, size=n)
    if extra:
        lens = np.insert(lens, n // 2, extra)
    off = np.zeros(lens.size + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    flat = rng.integers(0, 1 << 31, size=int(off[-1]), dtype=np.int64)
    return flat, off


def sides_of(algo, shape, flat, off):
    base = make_world(algo, flat, off)["on"]
    idx = base.kv_block_index()
    return {layout: Indexer(Config(
        token_processor=TokenProcessorConfig(block_size=BS, hash_algo=algo),
        device_chain="on", device_chain_layout=layout), kv_block_index=idx)
        for layout in SHAPES[shape][3]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algos", default="fnv-64a,sha256-cbor-64")
    ap.add_argument("--shapes", default="served,long1,big")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile", default="", help="ALGO:SHAPE:LAYOUT, 13 calls")
    args = ap.parse_args()
    assert torch.cuda.is_available()

    if args.profile:
        algo, shape, layout = args.profile.split(":")
        flat, off = make_batch(shape)
        ix = sides_of(algo, shape, flat, off)[layout]
        flat_t, off_t = torch.from_numpy(flat), torch.from_numpy(off)
        for _ in range(13):  # 3 to warm up
            ix.score_flat_tokens(flat_t, off_t, "m", []).cpu()
        torch.cuda.synchronize()
        print(json.dumps({"profile": args.profile, "calls": 13}), flush=True)
        return

    for shape in args.shapes.split(","):
        flat, off = make_batch(shape)
        flat_t, off_t = torch.from_numpy(flat), torch.from_numpy(off)
        nc = (off[1:] - off[:-1]) // BS
        for algo in args.algos.split(","):
            ixs = sides_of(algo, shape, flat, off)
            a, b = SHAPES[shape][3]
            routes = {m: plan_read_route(off_t, BS, algo, True, ixs[m].config)
                      for m in (a, b)}
            want = ixs[a].score_flat_tokens(flat_t, off_t, "m", [])
            got = ixs[b].score_flat_tokens(flat_t, off_t, "m", [])
            assert torch.equal(want, got) and want.max().item() > 0
            per = {a: [], b: []}
            for _ in range(args.rounds):
                for m in (a, b):
                    per[m].append(window(ixs[m], flat_t, off_t, args.window))
            plan = ixs[a].kv_block_index().table.ops.plan_ragged_waves(
                flat_t, off_t, BS)
            row = {"algo": algo, "shape": shape, "prompts": int(nc.size),
                   "tokens": int(off[-1]), "chunks": int(nc.sum()),
                   "padded_image_bytes": routes[a].image_bytes,
                   "padded_hash_bytes": int(nc.size * nc.max() * 8),
                   "ragged_image_bytes": int(plan[2][-1]) * 4,
                   "ragged_hash_bytes": int(nc.sum()) * 8}
            for m in (a, b):
                r = routes[m]
                row[m] = {"route": ("ragged" if r.ragged else "padded")
                          if r.device else "cpu-chain",
                          "ms": round(statistics.median(per[m]) * 1e3, 3),
                          "ms_min": round(min(per[m]) * 1e3, 3),
                          "ms_max": round(max(per[m]) * 1e3, 3)}
            row["ratio"] = round(row[a]["ms"] / row[b]["ms"], 3)
            print(json.dumps(row), flush=True)
            del ixs


if __name__ == "__main__":
    main()
