"""Read-path routes, measured: Indexer.score_flat_tokens on a GpuIndex with
host int64 tokens, the CPU-chain route (device_chain="off") against the
device-chain route ("on"), alternating within one process.

    python scripts/bench_read_routes.py [--md table.md]
    rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -- \\
        python scripts/bench_read_routes.py --profile fnv-64a:256

Block size 16; prompt lengths uniform in 1024..8192 tokens, fixed seed;
batches of 1, 16, 256 and 4096 prompts.  Each shape is warmed up on both
routes, then every window runs calls for at least --window seconds and
ends in a synchronise.  One JSON line per (algo, batch); the crossover
per algo (smallest measured total chunk count from which the device
route stays ahead, rounded up to a power of two) at the end.  --profile
runs one shape on the device route only, each call followed by the D2H
of its scores, for a profiler's per-call breakdown.
"""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, __file__.rsplit("/", 2)[0])

import numpy as np
import torch

from llmd_kvcache_amd.indexer import Config, Indexer
from llmd_kvcache_amd.kvblock.gpu_index import GpuIndex, GpuIndexConfig
from llmd_kvcache_amd.kvblock.token_processor import (
    ChunkedTokenDatabase,
    TokenProcessorConfig,
)
from llmd_kvcache_amd.kvevents.events import BlockStored

BS = 16
PODS = 64
LEN_LO, LEN_HI = 1024, 8192
STORED_PROMPTS = 64   # prompts whose first chunks some pod holds
STORED_CHUNKS = 64


def make_batch(B, seed=7):
    rng = np.random.default_rng(seed)
    lens = rng.integers(LEN_LO, LEN_HI + 1, size=B)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    flat = rng.integers(0, 1 << 31, size=int(off[-1]), dtype=np.int64)
    return flat, off


def make_world(algo, flat, off):
    tpc = TokenProcessorConfig(block_size=BS, hash_algo=algo)
    tp = ChunkedTokenDatabase(tpc)
    idx = GpuIndex(GpuIndexConfig(capacity=1 << 20, pods_per_key=10))
    for i in range(PODS):
        idx.registry.pod_id(f"pod-{i}")
    batch = []
    h = 1
    for b in range(min(STORED_PROMPTS, off.size - 1)):
        toks = flat[off[b]:off[b] + STORED_CHUNKS * BS]
        hs = np.arange(h, h + STORED_CHUNKS, dtype=np.uint64)
        h += STORED_CHUNKS
        batch.append((f"pod-{b % PODS}", "m",
                      [BlockStored(hs, None, toks, BS)]))
    idx.apply_event_batches(batch, tp)
    torch.cuda.synchronize()
    ixs = {mode: Indexer(Config(token_processor=TokenProcessorConfig(
        block_size=BS, hash_algo=algo), device_chain=mode),
        kv_block_index=idx) for mode in ("off", "on")}
    return ixs


def window(ix, flat_t, off_t, seconds):
    torch.cuda.synchronize()
    t0 = time.monotonic()
    calls = 0
    while True:
        ix.score_flat_tokens(flat_t, off_t, "m", [])
        calls += 1
        if time.monotonic() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.monotonic() - t0) / calls


def pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algos", default="fnv-64a,sha256-cbor-64")
    ap.add_argument("--batches", default="1,16,256,4096")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--md", default="")
    ap.add_argument("--profile", default="",
                    help="ALGO:BATCH - device route only, 20 calls")
    args = ap.parse_args()
    assert torch.cuda.is_available()

    if args.profile:
        algo, B = args.profile.split(":")
        flat, off = make_batch(int(B))
        ixs = make_world(algo, flat, off)
        flat_t, off_t = torch.from_numpy(flat), torch.from_numpy(off)
        for _ in range(23):  # 3 to warm up
            ixs["on"].score_flat_tokens(flat_t, off_t, "m", []).cpu()
        torch.cuda.synchronize()
        print(json.dumps({"profile": args.profile, "calls": 23,
                          "tokens": int(off[-1]),
                          "token_bytes": int(off[-1]) * 8}), flush=True)
        return

    rows = []
    for algo in args.algos.split(","):
        for B in (int(x) for x in args.batches.split(",")):
            flat, off = make_batch(B)
            ixs = make_world(algo, flat, off)
            flat_t, off_t = torch.from_numpy(flat), torch.from_numpy(off)
            chunks = int(((off[1:] - off[:-1]) // BS).sum())
            # warm-up, and the two routes agree
            s_off = ixs["off"].score_flat_tokens(flat_t, off_t, "m", [])
            s_on = ixs["on"].score_flat_tokens(flat_t, off_t, "m", [])
            assert torch.equal(s_off, s_on), (algo, B)
            assert s_off.max().item() >= STORED_CHUNKS
            per = {"off": [], "on": []}
            for _ in range(args.rounds):
                for mode in ("off", "on"):
                    per[mode].append(
                        window(ixs[mode], flat_t, off_t, args.window))
            row = {"algo": algo, "batch": B, "chunks": chunks,
                   "tokens": int(off[-1])}
            for mode in ("off", "on"):
                med = statistics.median(per[mode])
                row[f"{mode}_ms"] = round(med * 1e3, 4)
                row[f"{mode}_ms_min"] = round(min(per[mode]) * 1e3, 4)
                row[f"{mode}_ms_max"] = round(max(per[mode]) * 1e3, 4)
                row[f"{mode}_prompts_per_s"] = round(B / med, 1)
            row["speedup_on"] = round(row["off_ms"] / row["on_ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ixs

    cross = {}
    for algo in args.algos.split(","):
        mine = sorted((r for r in rows if r["algo"] == algo),
                      key=lambda r: r["chunks"])
        first = None  # smallest size from which "on" wins at every size
        for r in reversed(mine):
            if r["on_ms"] < r["off_ms"]:
                first = r["chunks"]
            else:
                break
        cross[algo] = {"crossover_chunks": first,
                       "min_chunks": pow2_at_least(first) if first else None}
    print(json.dumps({"crossover": cross}), flush=True)

    if args.md:
        with open(args.md, "w") as f:
            f.write("| algo | prompts | chunks | off ms (min..max) | "
                    "on ms (min..max) | off prompts/s | on prompts/s | "
                    "off/on |\n|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(
                    f"| {r['algo']} | {r['batch']} | {r['chunks']} | "
                    f"{r['off_ms']} ({r['off_ms_min']}..{r['off_ms_max']}) | "
                    f"{r['on_ms']} ({r['on_ms_min']}..{r['on_ms_max']}) | "
                    f"{r['off_prompts_per_s']} | {r['on_prompts_per_s']} | "
                    f"{r['speedup_on']} |\n")
            f.write("\n" + json.dumps({"crossover": cross}) + "\n")


if __name__ == "__main__":
    main()
