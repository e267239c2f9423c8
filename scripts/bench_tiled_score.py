"""Score and top-n past the resident fused kernel's LDS ceiling: the chooser
(gpu_score_hashes / gpu_topk_hashes) against the split route spelled out
(gpu_lookup + gpu_score_from_masks [+ gpu_topk_rows]) and, where the build
has them, the tiled ops called directly - on one table, in one process,
alternating.  On a commit before the tiled kernels the chooser is the split
route, so the same script measures both sides.

Shapes (prompts x keys x pods x tiers): 4096 x 2048 x 256 x 2, 1024 x 8192 x
64 x 2, 4096 x 512 x 4096 x 1, 4096 x 512 x 1088 x 2, each with walks of the
full prompt and with a break at one quarter (the keys behind it are not in
the table, as behind a cached prefix); 32768 x 512 x 64 x 1, which the
resident kernel serves: gpu_fused_score against gpu_tiled_score; and 4096 x
512 x 4096 x 4, the widest masks there are (2 KB per key).

Table: min(prompts, 1024) documents of K keys; prompt b asks for document
b % documents.  Document d is held by pod (7 d) % P over `depth` leading
keys, (7 d + 11) % P over depth / 2 and (7 d + 22) % P over depth / 4, on
tier d % tiers.

Method: values compared equal, 3 warm-ups, then device events around each
route (they enclose the readback of the top-n results; the matrix stays on
the device), routes alternating, 15 repeats: median, minimum and spread
((max - min) / median).

    python scripts/bench_tiled_score.py [--out results.json] [--shapes 0,2]

--trace ROUTE runs ten calls of that route per shape and no timing, for a
kernel trace.
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

SHAPES = [(4096, 2048, 256, 2), (1024, 8192, 64, 2), (4096, 512, 4096, 1),
          (4096, 512, 1088, 2), (32768, 512, 64, 1), (4096, 512, 4096, 4)]
TOP_N = 4


def build(B, K, P, T, depth):
    docs_n = min(B, 1024)
    t = KvTable(GpuIndexConfig(capacity=1 << 24, pods_per_key=4))
    g = torch.Generator(device="cuda")
    g.manual_seed(K + P)
    docs = torch.randint(1, 1 << 62, (docs_n, K), dtype=torch.int64,
                         device="cuda", generator=g)
    d = torch.arange(docs_n, device="cuda")
    for i, off in enumerate((0, 11, 22)):
        entry = (((d % T) << 24) | ((d * 7 + off) % P + 1)).to(torch.int32)
        for e in entry.unique().tolist():
            h = docs[entry == e, :depth >> i].reshape(-1)
            t.insert(h, h, 0, torch.tensor([e], dtype=torch.int32,
                                           device="cuda"))
    torch.cuda.synchronize()
    return t, docs.repeat((B + docs_n - 1) // docs_n, 1)[:B].reshape(-1)


def routes(t, hashes, B, K, P, T):
    ops = t.ops
    offsets = torch.arange(B + 1, dtype=torch.int32, device="cuda") * K
    filt = torch.zeros(0, dtype=torch.int64, device="cuda")
    weights = torch.tensor([1.0, 0.5, 0.25, 1.0], device="cuda")
    args = (hashes, offsets, 0, filt, weights, P)

    def split():
        _, masks = ops.gpu_lookup(*t._t(), hashes, 0, filt, P, t.next_epoch(),
                                  0, 1, T)
        return ops.gpu_score_from_masks(masks, offsets, weights, P)

    def top(fn):
        return lambda: tuple(x.cpu() for x in fn())

    def op(name, *more):
        return lambda: getattr(ops, name)(*t._t(), *args, t.next_epoch(), K, T,
                                          *more)

    resident = P <= 1024 and K * T * ((P + 63) // 64) * 8 <= 64 * 1024
    score = {"chooser": op("gpu_score_hashes")}
    topn = {"chooser": top(op("gpu_topk_hashes", TOP_N))}
    if resident:
        score["fused"] = op("gpu_fused_score")
    else:
        score["split"] = split
        topn["split"] = top(lambda: ops.gpu_topk_rows(split(), TOP_N))
    if hasattr(ops, "gpu_tiled_score"):
        score["tiled"] = op("gpu_tiled_score")
        topn["tiled"] = top(op("gpu_tiled_topk", TOP_N))
    return {"score": score, "topn": topn}


def same(fns):
    outs = [fn() for fn in fns.values()]
    for o in outs[1:]:
        if torch.is_tensor(o):
            assert torch.equal(o, outs[0])
        else:
            assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    first = outs[0] if torch.is_tensor(outs[0]) else outs[0][1]
    return float(first.max())


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
    ap.add_argument("--shapes", default="0,1,2,3,4,5")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0)}
    for B, K, P, T in (SHAPES[int(s)] for s in args.shapes.split(",")):
        for walk, depth in (("full", K), ("quarter", K // 4)):
            t, hashes = build(B, K, P, T, depth)
            for kind, fns in routes(t, hashes, B, K, P, T).items():
                if args.trace:
                    for _ in range(10 if args.trace in fns else 0):
                        fns[args.trace]()
                    continue
                best = same(fns)
                assert best > 0
                res = measure(fns, args.warmup, args.reps)
                res["best_score"] = best
                result[f"{B}x{K}x{P}x{T}_{walk}_{kind}"] = res
                print(json.dumps({f"{B}x{K}x{P}x{T}_{walk}_{kind}": res}),
                      flush=True)
            del t, hashes
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
