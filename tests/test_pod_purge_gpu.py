"""Purge by pod on the GPU: k_purge_pods against the CPU op, bit for bit,
on tables built on the CPU; the hand-built row cases; rows whose two
purged entries are cleared by different lanes and waves; and GpuIndex end
to end (AllBlocksCleared inside a burst, the ops a burst issues,
retire_pods followed by scoring)."""

import functools

import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(cpu_ext.maybe_load() is None,
                       reason="native extension not built"),
]

from llmd_kvcache_amd.indexer import Config, Indexer  # noqa: E402
from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex,
    GpuIndexConfig,
    KvTable,
    TableIndexConfig,
)
from llmd_kvcache_amd.kvblock.in_memory import InMemoryIndex  # noqa: E402
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    ChunkedTokenDatabase,
    TokenProcessorConfig,
)
from llmd_kvcache_amd.kvevents.events import (  # noqa: E402
    AllBlocksCleared,
    BlockRemoved,
    BlockStored,
)
from llmd_kvcache_amd.kvevents.pool import digest_events  # noqa: E402

from . import pod_purge_cases as cases  # noqa: E402

MODEL = "m"
OTHER = "m2"
N_PODS = 130

# A workgroup takes tiles of 256 rows and the grid is capped at 2048
# workgroups, so the grid-stride loop turns only from 2^19 rows on: the
# last shape is there for it (two tiles per workgroup).
SHAPES = [(64, 1), (64, 10), (1024, 3), (1024, 10), (65536, 10),
          (65536, 16), (1 << 20, 10)]
BITMAPS = {
    "empty": [],
    "one": [63],
    "word_edge": [63, 64],
    "all": list(range(N_PODS)),
}


@functools.lru_cache(maxsize=None)
def _reference_state(capacity, P):
    """The CPU-built table of one shape, as a state dict; built once and
    only ever copied from."""
    return cases.random_table(capacity, P, n_pods=N_PODS,
                              seed=capacity + P).state_dict()


def _pair(capacity, P):
    cpu = KvTable(TableIndexConfig(capacity=capacity, pods_per_key=P))
    gpu = KvTable(TableIndexConfig(capacity=capacity, pods_per_key=P,
                                   device="cuda:0"))
    state = _reference_state(capacity, P)
    cpu.load_state_dict(state)
    gpu.load_state_dict(state)
    return cpu, gpu


@pytest.mark.parametrize("model_id", [-1, 1], ids=["all_models", "model_1"])
@pytest.mark.parametrize("bitmap", list(BITMAPS))
@pytest.mark.parametrize("capacity,P", SHAPES)
def test_gpu_equals_cpu(capacity, P, bitmap, model_id):
    cpu, gpu = _pair(capacity, P)
    words = cases.purge_words(BITMAPS[bitmap])
    want = cpu.purge_pods(words, model_id)
    got = gpu.purge_pods(words, model_id)
    print(f"cap={capacity} P={P} {bitmap} model={model_id}: "
          f"cpu={want} gpu={got}")
    assert got == want
    cases.assert_tables_equal(cases.snapshot(cpu), cases.snapshot(gpu),
                              f"{capacity}x{P} {bitmap}")
    if bitmap == "empty":
        assert want == (0, 0)
    elif model_id == -1:
        assert want[0] > 0 and want[1] > 0  # the case does purge


@pytest.mark.parametrize("model_id", [-1, 0, 1])
@pytest.mark.parametrize("P", cases.HAND_PODS_PER_KEY)
def test_hand_rows_on_gpu(P, model_id):
    t = cases.hand_table(P, device="cuda:0")
    cases.check_hand_table(t, cases.PURGED, model_id)
    for pid in cases.PURGED:
        t = cases.hand_table(P, device="cuda:0")
        cases.check_hand_table(t, [pid], model_id)


@pytest.mark.parametrize("P,slots", [(10, (1, 8)), (3, (0, 2)), (16, (3, 12))])
def test_two_clearing_lanes_tombstone_the_row_once(P, slots):
    """Rows that hold exactly two purged pods, in slots that different
    lanes (at 256-row tile and 64-lane wave edges: different waves) read.
    Whoever clears second must see the row empty: every such row is
    tombstoned, and counted once."""
    C = 65536
    t = KvTable(TableIndexConfig(capacity=C, pods_per_key=P,
                                 device="cuda:0"))
    meta = torch.zeros(C, dtype=torch.int64)
    pods = torch.zeros(C, P, dtype=torch.int64)
    two = torch.arange(0, C, 3)          # the rows under test
    kept = torch.arange(1, C, 3)         # one purged pod and a survivor
    meta[two] = cases.OCC
    meta[kept] = cases.OCC
    pods[two, slots[0]] = cases.entry(63, 0)
    pods[two, slots[1]] = cases.entry(64, 3)
    pods[kept, slots[0]] = cases.entry(64, 0)
    pods[kept, slots[1]] = cases.entry(65, 3)
    t.meta.copy_(meta.to(torch.int32))   # wraps to the int32 bit pattern
    t.pods.copy_(pods.reshape(-1).to(torch.int32))
    t.keys.copy_(torch.arange(1, C + 1))
    entries, keys = t.purge_pods(cases.purge_words([63, 64]), -1)
    assert keys == two.numel()
    assert entries == 2 * two.numel() + kept.numel()
    meta_after = t.meta.cpu().to(torch.int64) & 0xFFFFFFFF
    rows = t.pods.cpu().reshape(C, P)
    live = (meta_after & cases.OCC != 0) & (meta_after & cases.TOMB == 0)
    empty = (rows != 0).sum(dim=1) == 0
    assert int((live & empty).sum()) == 0  # no row left live and empty
    assert bool((meta_after[two] & cases.TOMB != 0).all())
    assert bool((rows[kept, slots[1]] == cases.entry(65, 3)).all())
    assert int((rows != 0).sum()) == kept.numel()


# ---- GpuIndex end to end ----------------------------------------------


def _tp():
    return ChunkedTokenDatabase(TokenProcessorConfig(block_size=4))


def _toks(base, n_blocks):
    return list(range(base, base + 4 * n_blocks))


def _burst_with_clears():
    a, b, c, d = (_toks(0, 3), _toks(100, 2), _toks(200, 4), _toks(300, 2))
    store = lambda h, t: BlockStored(  # noqa: E731
        list(range(h, h + len(t) // 4)), None, t, 4)
    batches = [
        ("pod-1", MODEL, [store(10, a), AllBlocksCleared(), store(20, b)]),
        ("pod-2", MODEL, [store(10, a)]),
        ("pod-2", OTHER, [store(10, a), AllBlocksCleared(), store(30, c)]),
        ("pod-1", MODEL, [store(30, c), BlockRemoved([20]),
                          AllBlocksCleared()]),
        ("pod-3", MODEL, [store(30, c), AllBlocksCleared(),
                          AllBlocksCleared()]),
        ("pod-1", MODEL, [store(40, d)]),
    ]
    return batches, (a, b, c, d)


def _view(idx, tp, token_lists):
    out = []
    for model in (MODEL, OTHER):
        for toks in token_lists:
            keys = tp.tokens_to_kv_block_keys(None, toks, model)
            got = idx.lookup(keys, set())
            out.append([sorted((e.pod_identifier, e.device_tier)
                               for e in got.get(k, [])) for k in keys])
    return out


@pytest.mark.parametrize("option", [True, False])
def test_all_blocks_cleared_keeps_order_within_a_burst(option):
    tp = _tp()
    batches, token_lists = _burst_with_clears()
    gpu = GpuIndex(GpuIndexConfig(capacity=1 << 12, pods_per_key=10))
    ref = InMemoryIndex()
    gpu.apply_event_batches(batches, tp, clear_on_all_blocks_cleared=option)
    torch.cuda.synchronize()
    for pod, model, events in batches:
        digest_events(ref, tp, pod, model, events,
                      clear_on_all_blocks_cleared=option)
    got, want = _view(gpu, tp, token_lists), _view(ref, tp, token_lists)
    assert got == want
    if option:
        a_model = want[0]
        assert a_model == [[("pod-2", "gpu")]] * 3
        assert want[3] == [[("pod-1", "gpu")]] * 2      # d survives
        assert want[2] == [[]] * 4                       # c cleared twice
        assert want[6] == [[("pod-2", "gpu")]] * 4       # c, other model
    # the pods keep their ids: this event retires nobody
    assert gpu.registry.id_to_pod == ["pod-1", "pod-2", "pod-3"]


class _OpsSpy:
    """Records the name of every gpu_* op a table calls."""

    def __init__(self, mod):
        self._mod = mod
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if not name.startswith("gpu_"):
            return fn

        def call(*args, **kw):
            self.calls.append(name)
            return fn(*args, **kw)

        return call


def _spied(batches, **kw):
    gpu = GpuIndex(GpuIndexConfig(capacity=1 << 12, pods_per_key=10))
    spy = _OpsSpy(gpu.table.ops)
    gpu.table.ops = spy
    gpu.apply_event_batches(batches, _tp(), **kw)
    torch.cuda.synchronize()
    return spy.calls, gpu


def test_burst_without_the_event_issues_the_same_ops():
    batches, _ = _burst_with_clears()
    plain = [(p, m, [e for e in evs if not isinstance(e, AllBlocksCleared)])
             for p, m, evs in batches]
    base, _ = _spied(plain)
    assert len(base) == 1 and base[0].startswith("gpu_apply_events")
    # option on, no such event in the burst: today's path, today's launches
    assert _spied(plain, clear_on_all_blocks_cleared=True)[0] == base
    # option off, events present: still a no-op
    assert _spied(batches)[0] == base
    assert _spied(batches, clear_on_all_blocks_cleared=False)[0] == base
    # option on, events present: the sweeps appear between the applies
    calls, _ = _spied(batches, clear_on_all_blocks_cleared=True)
    assert calls.count("gpu_purge_pods") == 5
    assert calls[-1].startswith("gpu_apply_events")


@pytest.mark.parametrize("route", ["off", "on"])
def test_retire_then_score_flat_tokens(route):
    tp = _tp()
    gpu = GpuIndex(GpuIndexConfig(capacity=1 << 12, pods_per_key=10))
    for i in range(70):
        gpu.registry.pod_id(f"p{i}")
    ix = Indexer(Config(token_processor=TokenProcessorConfig(block_size=4),
                        device_chain=route), kv_block_index=gpu)
    a, b = _toks(0, 6), _toks(500, 3)
    store = lambda h, t: BlockStored(  # noqa: E731
        list(range(h, h + len(t) // 4)), None, t, 4)
    gpu.apply_event_batches([
        ("p3", MODEL, [store(10, a)]),
        ("p69", MODEL, [store(10, a[:16])]),
        ("p7", MODEL, [store(10, a[:8]), store(50, b)]),
    ], tp)
    flat = torch.tensor(a + b, dtype=torch.int64)
    off = torch.tensor([0, len(a), len(a) + len(b)], dtype=torch.int64)

    def score():
        s = ix.score_flat_tokens(flat, off, MODEL, [])
        return tuple(s.shape), gpu.scores_to_map(s)

    shape, maps = score()
    assert shape == (2, 128)
    assert maps == [{"p3": 6.0, "p69": 4.0, "p7": 2.0}, {"p7": 3.0}]

    out = gpu.retire_pods(["p3"] + [f"p{i}" for i in range(64, 70)])
    # blocks 2..5 of the first prompt were held by the retired pods alone
    assert out["entries_cleared"] == 10 and out["keys_tombstoned"] == 4
    shape, maps = score()
    assert shape == (2, 64)  # the highest ids went: one pod word less
    assert maps == [{"p7": 2.0}, {"p7": 3.0}]
    assert gpu.registry.num_pods == 64

    # a new pod takes the lowest freed id and scores under its own name
    gpu.apply_event_batches([("fresh", MODEL, [store(10, a[:12])])], tp)
    assert gpu.registry.pod_to_id["fresh"] == 3
    shape, maps = score()
    assert shape == (2, 64)
    assert maps == [{"fresh": 3.0, "p7": 2.0}, {"p7": 3.0}]
