"""Score top-n: the pick after the score matrix against the pick inside the
score kernels, on one table, in one process, alternating.

 (a) matrix:  gpu_score_hashes, then torch.topk(scores, n, dim=1) (argmax
              for n = 1), then .cpu() of the result;
 (b) top-n:   gpu_topk_hashes, then .cpu() of its two tensors.

Shapes: 32768 prompts x 512 keys at 64, 256 and 1024 pods, and one
4096-pod point (4096 prompts: lookup + mask walk + k_topk_rows, 1 GB of
masks), each with top_n 1 and 4.  One tier is registered, which is what
lets 512 keys x 1024 pods into the fused kernel's 64 KB.

Table: 4096 documents of 512 keys; prompt b asks for document b % 4096.
Document d is held by pods (7 d) % P over all 512 keys, (7 d + 11) % P over
256 and (7 d + 22) % P over 128, so every prompt has up to three scoring
pods and the walk runs the prompt's whole length.

Method: warm-up, then device events around each route (they enclose the
readback), the two routes alternating, median of the repeats.  The values
of the two routes are compared before timing (torch.topk leaves the order
of equal scores open, so the ids are not).

    python scripts/bench_score_topk.py [--out results.json] [--pods 64,256]

--trace runs ten calls of each route per shape and no timing, for a kernel
trace.
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

DOCS, K = 4096, 512
HOLD = ((0, 512), (11, 256), (22, 128))  # (pod offset, leading keys held)


def build(num_pods):
    t = KvTable(GpuIndexConfig(capacity=1 << 22, pods_per_key=4))
    g = torch.Generator(device="cuda")
    g.manual_seed(num_pods)
    docs = torch.randint(1, 1 << 62, (DOCS, K), dtype=torch.int64,
                         device="cuda", generator=g)
    d = torch.arange(DOCS, device="cuda")
    for off, depth in HOLD:
        pod_of = (d * 7 + off) % num_pods
        for p in pod_of.unique().tolist():
            h = docs[pod_of == p, :depth].reshape(-1)
            t.insert(h, h, 0, torch.tensor([p + 1], dtype=torch.int32,
                                           device="cuda"))
    torch.cuda.synchronize()
    return t, docs


def routes(t, docs, B, num_pods, top_n):
    hashes = docs[torch.arange(B, device="cuda") % DOCS].reshape(-1)
    offsets = torch.arange(B + 1, dtype=torch.int32, device="cuda") * K
    filt = torch.zeros(0, dtype=torch.int64, device="cuda")
    weights = torch.ones(4, dtype=torch.float32, device="cuda")
    args = (hashes, offsets, 0, filt, weights, num_pods)

    def matrix():
        s = t.ops.gpu_score_hashes(*t._t(), *args, t.next_epoch(), K, 1)
        if top_n == 1:
            return (s.argmax(dim=1).cpu(),)
        v, i = torch.topk(s, top_n, dim=1)
        return v.cpu(), i.cpu()

    def topn():
        i, v = t.ops.gpu_topk_hashes(*t._t(), *args, t.next_epoch(), K, 1,
                                     top_n)
        return v.cpu(), i.cpu()

    return {"matrix": matrix, "topn": topn}


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
    res = {k: {"median_ms": statistics.median(v), "min_ms": min(v),
               "max_ms": max(v)} for k, v in ms.items()}
    res["topn_over_matrix"] = (res["topn"]["median_ms"] /
                               res["matrix"]["median_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pods", default="64,256,1024,4096")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "keys_per_prompt": K}
    for num_pods in (int(p) for p in args.pods.split(",")):
        t, docs = build(num_pods)
        B = 4096 if num_pods > 1024 else 32768
        for top_n in (1, 4):
            fns = routes(t, docs, B, num_pods, top_n)
            if args.trace:
                for _ in range(10):
                    for fn in fns.values():
                        fn()
                continue
            if top_n > 1:  # same values; argmax returns no values
                assert torch.equal(fns["matrix"]()[0], fns["topn"]()[0])
            else:
                v, i = fns["topn"]()
                assert (v > 0).all() and (i >= 0).all()
            res = measure(fns, args.warmup, args.reps)
            res["prompts"] = B
            result[f"pods{num_pods}_top{top_n}"] = res
        del t, docs
        torch.cuda.empty_cache()
    blob = json.dumps(result, indent=1)
    print(blob)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(blob)


if __name__ == "__main__":
    main()
