"""The linked wave ingest against plain Python (golden_chain, InMemoryIndex
fed through digest_events) and, where sequential digest is not the contract,
against gpu_apply_events_split.  Requires an MI355X."""

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
from tests.test_event_waves_gpu import (  # noqa: E402
    M1, M2, SMALL_E, SMALL_R, UNKNOWN, bursts as wave_bursts)
from tests.test_sha_chain_gpu import _OpsSpy, _rand_tokens  # noqa: E402

SPLIT, LINKED = "gpu_apply_events_split", "gpu_apply_events_split_linked"
CASES = pytest.mark.parametrize("algo,bs", [
    (a, bs) for a in ("fnv-64a", "sha256-cbor-64", "sha256-cbor-64-low")
    for bs in (4, 17, 128)])


def bursts(bs):
    """(the waves test's seed, linked, odd).  linked: 162 stores and a removal
    in four groups, every batch-local parent an earlier event of its own
    group, so digesting event by event agrees with the group-local rule.
    Level 0 (two waves): 100 stores, parents by i % 5; a store dropped for its
    hash count and the child of its 1004, which the engine map resolves.
    Level 1 (a padded wave): twelve a group; levels 2, 3: two and one a group.
    odd: pod-a stores 1100 anew and 60001 at two blocks (one request key);
    pod-b's parents 1100 and 60001 are in no block of its own group."""
    rng = random.Random(47)

    def toks(n_blocks, spare=0):
        return _rand_tokens(rng, n_blocks * bs + spare)

    parents = (None, 1005, UNKNOWN, 1002, SMALL_E)
    groups = {(p, m): [] for p in ("pod-a", "pod-b") for m in (M1, M2)}
    order = list(groups)
    for i in range(100):
        n = 1 + i % 7
        groups[order[(i // 5) % 4]].append(BlockStored(
            [10_000 + 64 * i + c for c in range(n)], parents[i % 5],
            toks(n, i % bs), bs))
    next_hash = [30_000]

    def child(of, block, n):
        next_hash[0] += 64
        return BlockStored(list(range(next_hash[0], next_hash[0] + n)),
                           of.block_hashes[block], toks(n, n % bs), bs)

    for evs in groups.values():
        l0 = list(evs)
        l1 = [child(l0[k], -1 if k % 2 == 0 else len(l0[k].block_hashes) // 2,
                    1 + k % 4) for k in range(9)]
        l1 += [child(l0[0], -1, 2), child(l0[0], -1, 1)]  # a fork of three
        one = next(ev for ev in l0 if len(ev.block_hashes) == 1)
        l1.append(child(one, 0, 9))  # longer than its parent
        l2 = [child(l1[1], 0, 3), child(l1[11], 4, 1)]
        evs += l1 + l2 + [child(l2[0], 1, 2)]
    a1 = groups[("pod-a", M1)]
    a1.insert(3, BlockRemoved([1000]))  # pod-b keeps it
    a1.insert(7, BlockStored([1003, 1004], None, toks(1), bs))  # dropped
    a1.append(BlockStored([29_000], 1004, toks(1), bs))
    linked = [(p, m, evs) for (p, m), evs in groups.items()]

    twice = toks(3)
    odd = [
        ("pod-a", M1, [BlockStored([1100], None, toks(1), bs),
                       BlockStored([60_000, 60_001], None, twice[:2 * bs], bs),
                       BlockStored([60_000, 60_001, 60_002], None, twice, bs),
                       BlockStored([60_010], 60_001, toks(1), bs)]),
        ("pod-b", M1, [BlockStored([60_020], 1100, toks(1), bs),
                       BlockStored([60_030], 60_001, toks(1), bs),
                       BlockStored([60_040, 60_041], 60_020, toks(2), bs)]),
    ]
    return wave_bursts(bs)[0], linked, odd


def _index(layout):
    gpu = GpuIndex(GpuIndexConfig(capacity=1 << 12, pods_per_key=10,
                                  event_chain_layout=layout,
                                  event_link_max_levels=4))
    spy = gpu.table.ops = _OpsSpy(gpu.table.ops)
    spy.EVENT_OPS = _OpsSpy.EVENT_OPS + (
        "gpu_apply_events_split_waves", LINKED)
    gpu.add([Key(M1, SMALL_E)], [Key(M1, SMALL_R)], [PodEntry("pod-a", "gpu")])
    return gpu, spy


@CASES
def test_event_links_against_python(algo, bs):
    from llmd_kvcache_amd.kvblock import InMemoryIndex
    from llmd_kvcache_amd.kvevents.pool import digest_events

    tp = ChunkedTokenDatabase(TokenProcessorConfig(bs, hash_algo=algo))
    gpu, spy = _index("linked")
    ref = InMemoryIndex()
    ref.add([Key(M1, SMALL_E)], [Key(M1, SMALL_R)], [PodEntry("pod-a", "gpu")])
    golden = {(M1, SMALL_E): SMALL_R}  # (model, engine hash) -> request hash
    dropped = []
    for batches in bursts(bs)[:2]:
        for pod, model, events in batches:
            digest_events(ref, tp, pod, model, events)
            for ev in events:
                if not isinstance(ev, BlockStored):
                    continue
                root = golden.get((model, ev.parent_block_hash),
                                  tp.config.init_hash())
                chain = golden_chain(algo, root, ev.token_ids, bs)
                if len(chain) != len(ev.block_hashes):
                    dropped.append((model, ev.block_hashes))
                else:
                    golden.update(((model, eh), rh) for eh, rh
                                  in zip(ev.block_hashes, chain))
        gpu.apply_event_batches(batches, tp)
    torch.cuda.synchronize()
    assert spy.calls[-1] == LINKED
    assert len(golden) > 500 and dropped == [(M1, [1003, 1004])]
    for (model, eh), rh in golden.items():
        rk = Key(model, rh)
        assert gpu.get_request_key(Key(model, eh)) == rk, (model, eh)
        want = ref.lookup([rk], set()).get(rk, [])
        assert set(gpu.lookup([rk], set()).get(rk, [])) == set(want), (model, eh)


@CASES
def test_event_links_against_split(algo, bs):
    tp = ChunkedTokenDatabase(TokenProcessorConfig(bs, hash_algo=algo))
    (new, new_spy), (old, old_spy) = _index("linked"), _index("rect")
    all_bursts = bursts(bs)
    for batches in all_bursts:
        new.apply_event_batches(batches, tp)
        old.apply_event_batches(batches, tp)
    torch.cuda.synchronize()
    assert new_spy.calls[1:] == [LINKED, LINKED]
    assert old_spy.calls[1:] == [SPLIT, SPLIT]
    hashes = {(model, eh) for batches in all_bursts for _, model, events
              in batches for ev in events for eh in ev.block_hashes}
    rks = [new.get_request_key(Key(model, eh)) for model, eh in hashes]
    assert rks == [old.get_request_key(Key(m, eh)) for m, eh in hashes]
    assert sum(rk is not None for rk in rks) > 500
    for rk in filter(None, rks):
        assert set(new.lookup([rk], set()).get(rk, [])) == \
            set(old.lookup([rk], set()).get(rk, [])), rk
