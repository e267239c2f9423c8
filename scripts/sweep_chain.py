"""Hash-chain kernel sweep on MI355X: batch x algo grid.

    python scripts/sweep_chain.py
    python scripts/sweep_chain.py --algo fnv-64a,sha256-cbor-64 \
        --batches 512,4096,32768 --repeats 5
    python scripts/sweep_chain.py --block-size 32 --row-major

--algo takes one or more hash_algo names (utils.hashing.NATIVE_ALGO_IDS);
with several, each batch size is measured for every algo back to back in
the same process, so the rows are directly comparable.  --row-major
measures the [B, max_chunks] output the read path consumes (the FNV
kernel stages it through LDS) instead of the transposed default.  Every
cell is warmed up, then timed `--repeats` times over `--iters` launches
each (host clock around a device synchronise); min / median / max of the
repeats are printed.
"""
import argparse
import statistics
import sys
import time

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import torch

from llmd_kvcache_amd.ops import cpu_ext
from llmd_kvcache_amd.utils import hashing


def _ints(s):
    return tuple(int(x) for x in s.split(",") if x)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--algo", default="fnv-64a",
                    help="comma-separated hash_algo names "
                         f"({', '.join(hashing.NATIVE_ALGO_IDS)})")
    ap.add_argument("--batches", type=_ints,
                    default=(512, 1024, 2048, 4096, 8192, 16384))
    ap.add_argument("--chunks", type=int, default=512,
                    help="chunks per prompt (8k tokens / bs 16)")
    ap.add_argument("--block-size", type=int, default=16)
    ap.add_argument("--row-major", action="store_true",
                    help="write [B, max_chunks] instead of [max_chunks, B]")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=1)
    args = ap.parse_args()

    algos = [a for a in args.algo.split(",") if a]
    for a in algos:
        if a not in hashing.NATIVE_ALGO_IDS:
            ap.error(f"unknown --algo {a!r}")
    mod = cpu_ext.require()
    K = args.chunks
    BS = args.block_size
    row_major = int(args.row_major)
    layout = "row-major" if row_major else "transposed"
    for B in args.batches:
        toks = torch.randint(0, 1 << 31, (K * BS, B), dtype=torch.int32,
                             device="cuda")
        nch = torch.full((B,), K, dtype=torch.int32, device="cuda")
        for algo in algos:
            algo_id = hashing.NATIVE_ALGO_IDS[algo]
            init = hashing.CHAIN_ALGOS[algo][1]("")
            parents = torch.full(
                (B,), init - (1 << 64) if init >= (1 << 63) else init,
                dtype=torch.int64, device="cuda")

            def call():
                return mod.gpu_hash_chain_tr(toks, parents, nch, BS, K, 0,
                                             row_major, algo_id)

            call()  # warmup
            torch.cuda.synchronize()
            times = []
            for _ in range(args.repeats):
                t0 = time.monotonic()
                for _ in range(args.iters):
                    call()
                torch.cuda.synchronize()
                times.append((time.monotonic() - t0) / args.iters)
            dt = statistics.median(times)
            print(f"B={B:6d} bs={BS} {layout} algo={algo} {dt*1e3:8.3f} ms "
                  f"(min {min(times)*1e3:.3f} max {max(times)*1e3:.3f}, "
                  f"n={len(times)})  "
                  f"{B/dt/1e6:8.3f} M prompts/s  "
                  f"{B*K/dt/1e9:6.2f} G chunks/s", flush=True)


if __name__ == "__main__":
    main()
