"""The wave-tiled ingest chain (gpu_apply_events_split_waves) against plain
Python: request keys from golden_chain, pods from an InMemoryIndex fed
through digest_events.  Requires an MI355X."""

import random

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex, GpuIndexConfig)
from llmd_kvcache_amd.kvblock.keys import Key, PodEntry  # noqa: E402
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    ChunkedTokenDatabase, TokenProcessorConfig)
from llmd_kvcache_amd.kvevents.events import (  # noqa: E402
    BlockRemoved, BlockStored)
from tests.sha_chain_cases import golden_chain  # noqa: E402
from tests.test_sha_chain_gpu import _OpsSpy, _rand_tokens  # noqa: E402

WAVES = "gpu_apply_events_split_waves"
M1, M2 = "m1", "m2"
SMALL_E, SMALL_R = 900, 5  # an engine hash whose request key is below 2^32
UNKNOWN = 999_999


def bursts(bs):
    """(seed, burst).  The burst: 141 stores and two removals over two pods
    and two models; 7 of the stores have no engine hash and never leave the
    host, one is dropped for its hash count, 133 chain: three waves, the
    last of 5 events.  Store i has i % 20 chunks (one has 40) and i % bs
    spare tokens; its parent goes by i % 5: none, the seed's 1005, one the
    engine map does not know, 1002 (which both models map, to different
    keys), SMALL_E (which only M1 maps)."""
    rng = random.Random(31)

    def toks(n_blocks, spare=0):
        return _rand_tokens(rng, n_blocks * bs + spare)

    shared = toks(6)
    seed = [
        ("pod-a", M1, [BlockStored(list(range(1000, 1006)), None, shared, bs)]),
        ("pod-b", M1, [BlockStored(list(range(1000, 1006)), None, shared, bs),
                       BlockStored([1100, 1101], None, toks(2), bs)]),
        ("pod-a", M2, [BlockStored([1000, 1001, 1002], None, toks(3), bs)]),
    ]
    parents = (None, 1005, UNKNOWN, 1002, SMALL_E)
    groups = {(p, m): [] for p in ("pod-a", "pod-b") for m in (M1, M2)}
    order = list(groups)
    for i in range(140):
        n = i % 20
        hashes = [10_000 + 64 * i + c for c in range(n)]
        if i == 57:  # one engine hash too many: dropped whole
            hashes.append(10_000 + 64 * i + n)
        groups[order[(i // 5) % 4]].append(
            BlockStored(hashes, parents[i % 5], toks(n, i % bs), bs))
    groups[("pod-a", M1)].insert(3, BlockRemoved([1000]))  # pod-b keeps it
    groups[("pod-b", M1)].insert(5, BlockRemoved([1100]))  # its only pod
    groups[("pod-b", M2)].append(BlockStored(
        [30_000 + c for c in range(40)], 1002, toks(40, bs - 1), bs))
    return seed, [(p, m, evs) for (p, m), evs in groups.items()]


@pytest.mark.parametrize("bs", [4, 64, 3, 17, 128])
@pytest.mark.parametrize("algo", ["fnv-64a", "sha256-cbor-64",
                                  "sha256-cbor-64-low"])
def test_event_waves_against_python(algo, bs):
    from llmd_kvcache_amd.kvblock import InMemoryIndex
    from llmd_kvcache_amd.kvevents.pool import digest_events

    tp = ChunkedTokenDatabase(TokenProcessorConfig(block_size=bs,
                                                   hash_algo=algo))
    gpu = GpuIndex(GpuIndexConfig(capacity=1 << 12, pods_per_key=10,
                                  event_chain_layout="waves"))
    spy = gpu.table.ops = _OpsSpy(gpu.table.ops)
    spy.EVENT_OPS = _OpsSpy.EVENT_OPS + (WAVES,)
    ref = InMemoryIndex()
    golden = {(M1, SMALL_E): SMALL_R}  # (model, engine hash) -> request hash
    for idx in (gpu, ref):
        idx.add([Key(M1, SMALL_E)], [Key(M1, SMALL_R)],
                [PodEntry("pod-a", "gpu")])
    dropped = []
    seed, burst = bursts(bs)
    for batches in (seed, burst):
        for pod, model, events in batches:
            digest_events(ref, tp, pod, model, events)
            for ev in events:
                if not isinstance(ev, BlockStored):
                    continue
                root = golden.get((model, ev.parent_block_hash),
                                  tp.config.init_hash())
                chain = golden_chain(algo, root, ev.token_ids, bs)
                if len(chain) != len(ev.block_hashes):
                    dropped.append((model, ev.block_hashes, chain))
                else:
                    golden.update(((model, eh), rh) for eh, rh
                                  in zip(ev.block_hashes, chain))
        gpu.apply_event_batches(batches, tp)
        assert spy.calls[-1] == WAVES
    torch.cuda.synchronize()

    assert len(golden) > 1300 and len(dropped) == 1
    assert golden[(M1, 1002)] != golden[(M2, 1002)]
    for (model, eh), rh in golden.items():
        rk = Key(model, rh)
        assert gpu.get_request_key(Key(model, eh)) == rk, (model, eh)
        want = ref.lookup([rk], set()).get(rk, [])
        assert set(gpu.lookup([rk], set()).get(rk, [])) == set(want), (model, eh)
    for model, ehs, chain in dropped:
        for eh in ehs:
            assert gpu.get_request_key(Key(model, eh)) is None, eh
        for rh in chain:
            rk = Key(model, rh)
            assert not gpu.lookup([rk], set()).get(rk), rh
    # the removals: 1000 lost pod-a and kept pod-b, 1100 lost its only pod
    rk = Key(M1, golden[(M1, 1000)])
    assert gpu.lookup([rk], set()) == {rk: [PodEntry("pod-b", "gpu")]}
    rk = Key(M1, golden[(M1, 1100)])
    assert not gpu.lookup([rk], set()).get(rk)
