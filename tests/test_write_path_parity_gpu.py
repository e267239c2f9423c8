"""Write-path kernels against the references they must agree with, fnv-64a:
removals and length-mismatched BlockStored events through each of the three
apply routes (InMemoryIndex fed through digest_events is the reference),
and k_evict with more than one pod entry (cpu_evict on a CPU table is the
reference).  All tests require an MI355X."""

import random

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex, GpuIndexConfig, NativeIndex, TableIndexConfig)
from llmd_kvcache_amd.kvblock.keys import Key, PodEntry  # noqa: E402
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    ChunkedTokenDatabase, TokenProcessorConfig)
from llmd_kvcache_amd.kvevents.events import (  # noqa: E402
    BlockRemoved, BlockStored)
from tests.sha_chain_cases import golden_chain  # noqa: E402
from tests.test_sha_chain_gpu import _OpsSpy, _rand_tokens  # noqa: E402

MODEL = "m"
FNV = "fnv-64a"
BS = 4


def route_batches():
    """[(route op or None, batches)]: a seed batch, then one batch per
    apply route.  Each route batch holds a store, removals of engine
    hashes stored in an EARLIER batch (one block loses its only pod, one
    keeps its other pod) and one BlockStored whose engine-hash count
    differs from len(tokens) // BS, which nothing names as parent.
    Two pods, at most 4 blocks per event."""
    rng = random.Random(29)

    def toks(n_blocks, spare=0):
        return _rand_tokens(rng, n_blocks * BS + spare)

    shared = toks(3)
    seed = [
        ("pod-a", MODEL, [BlockStored([100, 101, 102], None, shared, BS),
                          BlockStored([120, 121, 122], None, toks(3), BS)]),
        ("pod-b", MODEL, [BlockStored([100, 101, 102], None, shared, BS),
                          BlockStored([130, 131], None, toks(2), BS)]),
    ]
    independent = [  # no parent is stored by this batch
        ("pod-a", MODEL, [BlockStored([200, 201], 102, toks(2), BS),
                          BlockRemoved([120]), BlockRemoved([100])]),
        # three engine hashes, two chunks
        ("pod-b", MODEL, [BlockStored([210, 211, 212], None, toks(2), BS)]),
    ]
    chained = [  # 301 is stored by the event before the one it parents
        ("pod-a", MODEL, [BlockStored([300, 301], None, toks(2), BS),
                          BlockStored([302, 303], 301, toks(2), BS),
                          BlockRemoved([121])]),
        # one engine hash, two chunks
        ("pod-b", MODEL, [BlockStored([310], None, toks(2), BS),
                          BlockRemoved([101])]),
    ]
    store_remove = [  # stores and removes engine hash 401 in one batch
        ("pod-a", MODEL, [BlockStored([400, 401, 402], 303, toks(3), BS),
                          BlockRemoved([401]), BlockRemoved([122])]),
        # two engine hashes, one chunk and three spare tokens
        ("pod-b", MODEL, [BlockStored([410, 411], None, toks(1, spare=3),
                                      BS)]),
    ]
    return [(None, seed),
            ("gpu_apply_events_split_tr", independent),
            ("gpu_apply_events_split", chained),
            ("gpu_apply_events", store_remove)]


def assert_same_state(got_index, ref, tp, batches_so_far):
    """Per golden request key the same pods from both indexes, and the same
    get_request_key for every engine hash the reference still maps (it
    forgets an engine hash once its block empties, the table keeps it).
    A mismatched event left nothing behind: none of its engine hashes is
    mapped and none of the request keys of its tokens is present.
    Returns (live, emptied) block counts."""
    golden = {}  # engine hash -> golden request hash, never forgotten
    dropped = []  # (engine hashes, would-be request hashes)
    for _, _, events in batches_so_far:
        for ev in events:
            if not isinstance(ev, BlockStored):
                continue
            parent = (tp.config.init_hash() if ev.parent_block_hash is None
                      else golden[ev.parent_block_hash])
            chain = golden_chain(FNV, parent, ev.token_ids, BS)
            if len(chain) != len(ev.block_hashes):
                dropped.append((ev.block_hashes, chain))
            else:
                golden.update(zip(ev.block_hashes, chain))
    live = emptied = 0
    for eh, rh in golden.items():
        ek, rk = Key(MODEL, eh), Key(MODEL, rh)
        want = ref.lookup([rk], set()).get(rk, [])
        got = got_index.lookup([rk], set()).get(rk, [])
        assert set(got) == set(want), eh
        live += bool(want)
        emptied += not want
        ref_rk = ref.get_request_key(ek)
        if ref_rk is not None:
            assert ref_rk == rk
            assert got_index.get_request_key(ek) == rk, eh
    assert dropped
    for ehs, chain in dropped:
        for eh in ehs:
            assert ref.get_request_key(Key(MODEL, eh)) is None
            assert got_index.get_request_key(Key(MODEL, eh)) is None, eh
        for rh in chain:
            assert rh not in golden.values()
            rk = Key(MODEL, rh)
            assert not ref.lookup([rk], set()).get(rk)
            assert not got_index.lookup([rk], set()).get(rk), rh
    return live, emptied


def test_removals_and_mismatched_events_on_all_routes():
    from llmd_kvcache_amd.kvblock import InMemoryIndex
    from llmd_kvcache_amd.kvevents.pool import digest_events

    tp = ChunkedTokenDatabase(TokenProcessorConfig(block_size=BS,
                                                   hash_algo=FNV))
    gpu = GpuIndex(GpuIndexConfig(capacity=1 << 12, pods_per_key=10))
    spy = gpu.table.ops = _OpsSpy(gpu.table.ops)
    ref = InMemoryIndex()
    applied = []
    emptied_before = 0
    for route, batches in route_batches():
        for pod, model, events in batches:
            digest_events(ref, tp, pod, model, events)
        gpu.apply_event_batches(batches, tp)
        torch.cuda.synchronize()
        applied += batches
        if route is None:
            continue
        assert spy.calls[-1] == route
        live, emptied = assert_same_state(gpu, ref, tp, applied)
        assert live >= 1
        assert emptied > emptied_before  # this batch's removal took effect
        emptied_before = emptied


def test_evict_two_entries_then_the_last():
    """k_evict walks entries outer, slots inner: two of a key's three pods
    go in one call and the third stays; removing the third tombstones the
    key, so lookup misses it while the engine mapping still answers."""
    pods = [PodEntry("pod-a", "gpu"), PodEntry("pod-b", "gpu"),
            PodEntry("pod-c", "cpu")]
    ek, rk = Key(MODEL, 77), Key(MODEL, 0x1234_5678_9ABC_DEF0)
    other_e, other_r = Key(MODEL, 78), Key(MODEL, 0x0FED_CBA9_8765_4321)
    cpu = NativeIndex(TableIndexConfig(capacity=1 << 12, pods_per_key=10))
    gpu = GpuIndex(GpuIndexConfig(capacity=1 << 12, pods_per_key=10))
    for idx in (cpu, gpu):
        idx.add([ek, other_e], [rk, other_r], pods)
        idx.evict(ek, pods[:2])
    for idx in (cpu, gpu):
        assert idx.lookup([rk], set()) == {rk: [pods[2]]}
        assert set(idx.lookup([other_r], set())[other_r]) == set(pods)
        idx.evict(ek, pods[2:])
    for idx in (cpu, gpu):
        assert not idx.lookup([rk], set()).get(rk)
        assert idx.get_request_key(ek) == rk
        assert set(idx.lookup([other_r], set())[other_r]) == set(pods)
