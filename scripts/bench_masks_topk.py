"""Top-n from merged masks: gpu_topk_from_masks (one kernel, walk and pick)
against the two kernels the same answer took before it, gpu_score_from_masks
followed by gpu_topk_rows - on the same device masks, in one process,
alternating.

Shapes (prompts x keys x pods x tiers): 32768 x 512 x 64 x 2 (268 MB of
masks) and 4096 x 512 x 4096 x 4 (4.3 GB), each at top_n 1 and 4, each with
  full    every pod is listed by every key (tier (key + pod) % tiers), and
  broken  pod p is listed by its first 1 + 37 p % 128 keys only: every walk
          is over by key 128.
The masks are written straight to the device; no table is involved.

Method: results compared equal first, 3 warm-ups, then device events around
each route (kernels only: the results stay on the device), routes
alternating, 15 repeats: median, minimum and spread ((max - min) / median).
bytes_read is what each route has to read of the masks, from the shapes:
the composed walk stops at the first key nobody lists, the fused one at the
end of that key's tile plus the tile it loaded ahead.

    python scripts/bench_masks_topk.py [--out results.json] [--shapes 0,1]
"""

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402

SHAPES = [(32768, 512, 64, 2), (4096, 512, 4096, 4)]
BREAK = 128


def build_masks(B, K, P, T, broken):
    """int64 [B * K, T, W] on the device, every prompt alike."""
    W = (P + 63) // 64
    k = np.arange(K)[:, None]
    p = np.arange(P)[None, :]
    present = (k < 1 + (37 * p) % BREAK) if broken else np.ones((K, P), bool)
    bits = np.stack([present & ((k + p) % T == t) for t in range(T)], axis=1)
    words = np.packbits(bits.reshape(K, T, W, 64), axis=-1, bitorder="little")
    one = torch.from_numpy(words.view("<u8").reshape(K, T, W).view(np.int64))
    return one.cuda().repeat(B, 1, 1)


def bytes_read(ops, B, K, P, T, broken):
    W = (P + 63) // 64
    key = T * W * 8
    if not broken:
        return {"fused": B * K * key, "composed": B * K * key}
    KT = int(ops.tiled_score_tile_keys(T, W))
    tiles = min(BREAK // KT + 2, (K + KT - 1) // KT)
    return {"fused": B * min(tiles * KT, K) * key,
            "composed": B * (BREAK + 1) * key}


def measure(fns, warmup, reps):
    ms = {k: [] for k in fns}
    for i in range(warmup + reps):
        for name, fn in fns.items():  # alternating
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms[name].append(a.elapsed_time(b))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v),
                "spread": (max(v) - min(v)) / statistics.median(v)}
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    ops = cpu_ext.require()
    result = {"device": torch.cuda.get_device_name(0)}
    weights = torch.tensor([1.0, 0.5, 0.25, 0.125], device="cuda")
    for B, K, P, T in (SHAPES[int(s)] for s in args.shapes.split(",")):
        offsets = torch.arange(B + 1, dtype=torch.int32, device="cuda") * K
        for walk in ("full", "broken"):
            masks = build_masks(B, K, P, T, walk == "broken")
            nbytes = bytes_read(ops, B, K, P, T, walk == "broken")
            for top_n in (1, 4):
                fns = {
                    "fused": lambda: ops.gpu_topk_from_masks(
                        masks, offsets, weights[:T], P, top_n),
                    "composed": lambda: ops.gpu_topk_rows(
                        ops.gpu_score_from_masks(masks, offsets, weights[:T],
                                                 P), top_n),
                }
                got, want = fns["fused"](), fns["composed"]()
                assert torch.equal(got[0], want[0])
                assert torch.equal(got[1], want[1]) and float(got[1].max()) > 0
                res = measure(fns, args.warmup, args.reps)
                for name, r in res.items():
                    r["bytes_read"] = nbytes[name]
                    r["gb_per_s"] = nbytes[name] / r["median_ms"] / 1e6
                key = f"{B}x{K}x{P}x{T}_{walk}_top{top_n}"
                result[key] = res
                print(json.dumps({key: res}), flush=True)
            del masks
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
