"""Pod-id remap on the GPU: k_remap_pods against the CPU op, bit for bit,
on tables built on the CPU; the hand-built row cases; rows whose two
dropped entries are rewritten by different lanes and waves; the drop-only
map against k_purge_pods; and GpuIndex end to end (bursts, retire,
compact_pod_ids, scoring by name on both read routes)."""

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
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    ChunkedTokenDatabase,
    TokenProcessorConfig,
)
from llmd_kvcache_amd.kvevents.events import BlockStored  # noqa: E402

from . import pod_purge_cases as pc  # noqa: E402
from . import pod_remap_cases as cases  # noqa: E402

MODEL = "m"
N_PODS = 130

# Tiles of 256 rows under a 2048-workgroup cap (the purge's launch shape):
# 2^20 rows is the smallest capacity at which a workgroup takes a second
# tile.  Capacities 1 and 2 are the only ones with a dword tail.
SHAPES = [(1, 1), (2, 3), (64, 10), (512, 3), (1024, 10), (1024, 16),
          (1 << 20, 10)]


def _only_last_moved():
    m = cases.identity(4096)
    m[4000] = -1                  # nobody holds 4000: its id is free
    m[4095] = 4000
    return m


MAPS = {
    "identity": cases.identity(N_PODS),
    "drop_63_64": cases.drop_only((63, 64), N_PODS),
    "compact_two_thirds": None,   # built below, needs a seed
    "reverse": list(range(N_PODS - 1, -1, -1)),
    "n4096_last_id": _only_last_moved(),
}


def _compact_two_thirds():
    import random

    keep = sorted(random.Random(7).sample(range(N_PODS), 2 * N_PODS // 3))
    return cases.compaction(keep, N_PODS)


MAPS["compact_two_thirds"] = _compact_two_thirds()


@functools.lru_cache(maxsize=None)
def _reference_state(capacity, P):
    """The CPU-built table of one shape, as a state dict; built once and
    only ever copied from.  Pod 4095 is planted so the last id has
    entries to move."""
    if capacity <= 2:
        # every dword of the tail in use: one live row per slot
        t = KvTable(TableIndexConfig(capacity=capacity, pods_per_key=P))
        ids = (63, 5, 4095, 64, 129, 0)
        t.meta.fill_(pc.i32(pc.OCC))
        t.keys.copy_(torch.arange(1, capacity + 1))
        t.pods.copy_(torch.tensor(
            [pc.i32(pc.entry(ids[k % 6], k % 4))
             for k in range(capacity * P)], dtype=torch.int32))
        return t.state_dict()
    t = pc.random_table(capacity, P, n_keys=min(300, capacity // 2),
                        n_pods=N_PODS, seed=capacity + P)
    occ = [i for i, m in enumerate(t.meta.tolist())
           if (m & 0xFFFFFFFF) & pc.OCC]
    for i in occ[::9]:
        t.pods[i * P + P - 1] = pc.i32(pc.entry(4095, 2))
    return t.state_dict()


def _pair(capacity, P):
    cpu = KvTable(TableIndexConfig(capacity=capacity, pods_per_key=P))
    gpu = KvTable(TableIndexConfig(capacity=capacity, pods_per_key=P,
                                   device="cuda:0"))
    state = _reference_state(capacity, P)
    cpu.load_state_dict(state)
    gpu.load_state_dict(state)
    return cpu, gpu


@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("capacity,P", SHAPES)
def test_gpu_equals_cpu(capacity, P, name):
    cpu, gpu = _pair(capacity, P)
    before = pc.snapshot(cpu)
    want = cpu.remap_pods(MAPS[name])
    got = gpu.remap_pods(MAPS[name])
    print(f"cap={capacity} P={P} {name}: cpu={want} gpu={got}")
    assert got == want
    pc.assert_tables_equal(pc.snapshot(cpu), pc.snapshot(gpu),
                           f"{capacity}x{P} {name}")
    if name == "identity":
        assert want == (0, 0, 0)
        pc.assert_tables_equal(before, pc.snapshot(gpu), "identity")
    elif capacity >= 512:  # the case does what its name says
        if name == "drop_63_64":
            assert want[0] == 0 and want[1] > 0
        elif name == "reverse":
            assert want[0] > 0 and want[1] == 0
        elif name == "compact_two_thirds":
            assert want[0] > 0 and want[1] > 0 and want[2] > 0
        else:
            assert want[0] > 0


@pytest.mark.parametrize("name", list(cases.HAND_MAPS))
@pytest.mark.parametrize("P", pc.HAND_PODS_PER_KEY)
def test_hand_rows_on_gpu(P, name):
    t = cases.hand_table(P, device="cuda:0")
    cases.check_hand_table_remap(t, cases.HAND_MAPS[name])


@pytest.mark.parametrize("P,slots", [(10, (1, 8)), (3, (0, 2)), (16, (3, 12))])
def test_two_dropping_lanes_tombstone_the_row_once(P, slots):
    """Rows that hold exactly two dropped pods, in slots that different
    lanes (at 256-row tile and 64-lane wave edges: different waves) read:
    every such row is tombstoned, and counted once.  The same row with
    one dropped and one moved entry stays live."""
    C = 65536
    t = KvTable(TableIndexConfig(capacity=C, pods_per_key=P,
                                 device="cuda:0"))
    meta = torch.zeros(C, dtype=torch.int64)
    pods = torch.zeros(C, P, dtype=torch.int64)
    two = torch.arange(0, C, 3)          # two dropped pods
    mixed = torch.arange(1, C, 3)        # one dropped, one moved
    meta[two] = pc.OCC
    meta[mixed] = pc.OCC
    pods[two, slots[0]] = pc.entry(63, 0)
    pods[two, slots[1]] = pc.entry(64, 3)
    pods[mixed, slots[0]] = pc.entry(64, 0)
    pods[mixed, slots[1]] = pc.entry(65, 3)
    t.meta.copy_(meta.to(torch.int32))   # wraps to the int32 bit pattern
    t.pods.copy_(pods.reshape(-1).to(torch.int32))
    t.keys.copy_(torch.arange(1, C + 1))
    remap = cases.identity(66)
    remap[63] = remap[64] = -1
    remap[65] = 2
    remap[2] = 65
    moved, cleared, keys = t.remap_pods(remap)
    assert keys == two.numel()
    assert cleared == 2 * two.numel() + mixed.numel()
    assert moved == mixed.numel()
    meta_after = t.meta.cpu().to(torch.int64) & 0xFFFFFFFF
    rows = t.pods.cpu().reshape(C, P)
    assert bool((meta_after[two] == (pc.OCC | pc.TOMB)).all())
    assert bool((meta_after[mixed] == pc.OCC).all())
    assert bool((rows[mixed, slots[1]] == pc.entry(2, 3)).all())
    assert int((rows != 0).sum()) == mixed.numel()


@pytest.mark.parametrize("capacity,P", [(64, 10), (1024, 3), (1024, 16)])
def test_drop_only_remap_is_the_gpu_purge(capacity, P):
    _, a = _pair(capacity, P)
    _, b = _pair(capacity, P)
    ids = [0, 63, 64, 127, 4095]
    entries, keys = a.purge_pods(pc.purge_words(ids), -1)
    assert b.remap_pods(cases.drop_only(ids)) == (0, entries, keys)
    assert entries > 0 and keys > 0
    pc.assert_tables_equal(pc.snapshot(a), pc.snapshot(b), "drop-only")


def test_gpu_op_wants_the_map_on_the_device():
    t = cases.hand_table(3, device="cuda:0")
    with pytest.raises(RuntimeError):
        t.ops.gpu_remap_pods(*t._t(), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        t.ops.gpu_remap_pods(
            *t._t(), torch.tensor([1, 1], dtype=torch.int32, device="cuda:0"))


# ---- GpuIndex end to end ----------------------------------------------


def _tp():
    return ChunkedTokenDatabase(TokenProcessorConfig(block_size=4))


def _toks(base, n_blocks):
    return list(range(base, base + 4 * n_blocks))


def _store(h, t):
    return BlockStored(list(range(h, h + len(t) // 4)), None, t, 4)


@pytest.mark.parametrize("route", ["off", "on"])
def test_burst_retire_compact_score(route):
    """520 names, the 8 newest survive: scores by name are unchanged by
    the compaction on both read routes, the score width drops from 9 pod
    words to 1, and a new pod lands on the first id past the survivors."""
    tp = _tp()
    gpu = GpuIndex(GpuIndexConfig(capacity=1 << 14, pods_per_key=10))
    ix = Indexer(Config(token_processor=TokenProcessorConfig(block_size=4),
                        device_chain=route), kv_block_index=gpu)
    a, b = _toks(0, 6), _toks(500, 3)
    for i in range(520):
        assert gpu.registry.pod_id(f"p{i}") == i
    batches = []
    for i in range(504, 520):  # 8 pods per prompt: no pod set overflows
        toks = a[:4 * (1 + i % 6)] if i % 2 else b[:4 * (1 + i % 3)]
        batches.append((f"p{i}", MODEL, [_store(10 if i % 2 else 50, toks)]))
    gpu.apply_event_batches(batches, tp)
    flat = torch.tensor(a + b, dtype=torch.int64)
    off = torch.tensor([0, len(a), len(a) + len(b)], dtype=torch.int64)

    def score():
        with gpu.registry.ids_shared():
            s = ix.score_flat_tokens(flat, off, MODEL, [])
            return tuple(s.shape), gpu.scores_to_map(s)

    want = [{f"p{i}": float(1 + i % 6) for i in range(512, 520) if i % 2},
            {f"p{i}": float(1 + i % 3) for i in range(512, 520) if not i % 2}]
    out = gpu.retire_pods([f"p{i}" for i in range(512)])
    assert out["entries_cleared"] > 0
    assert gpu._num_pods_padded() == 576
    shape, maps = score()
    assert shape == (2, 576) and maps == want

    out = gpu.compact_pod_ids()
    assert out["pods_moved"] == 8 and out["num_pods"] == 8
    assert out["entries_moved"] == sum(
        1 + i % 6 if i % 2 else 1 + i % 3 for i in range(512, 520))
    assert out["entries_cleared"] == 0 and out["keys_tombstoned"] == 0
    assert out["pod_generation"] == 1
    assert gpu._num_pods_padded() == 64
    shape, maps = score()
    assert shape == (2, 64) and maps == want
    assert gpu.compact_pod_ids()["pods_moved"] == 0
    assert gpu.registry.pod_generation == 1

    # a further burst for a new pod: first id past the survivors
    gpu.apply_event_batches([("fresh", MODEL, [_store(10, a[:12])])], tp)
    assert gpu.registry.pod_to_id["fresh"] == 8
    shape, maps = score()
    want[0]["fresh"] = 3.0
    assert shape == (2, 64) and maps == want
    keys = tp.tokens_to_kv_block_keys(None, a[:4], MODEL)
    names = sorted(e.pod_identifier for e in gpu.lookup(keys, set())[keys[0]])
    assert names == sorted(want[0])


def test_retire_with_compact_is_one_sweep_on_the_gpu():
    tp = _tp()
    a = _toks(0, 6)

    def build():
        gpu = GpuIndex(GpuIndexConfig(capacity=1 << 12, pods_per_key=10))
        for i in range(70):
            assert gpu.registry.pod_id(f"p{i}") == i
        # 7 pods per prompt: no pod set overflows
        gpu.apply_event_batches(
            [(f"p{i}", MODEL, [_store(100 * (i % 10),
                                      _toks(1000 * (i % 10), 1 + i % 6))])
             for i in range(70)], tp)
        return gpu

    # groups of one burst run concurrently, so two bursts need not leave
    # the same slot order inside a row: build once, copy the table
    one = build()
    two = GpuIndex(GpuIndexConfig(capacity=1 << 12, pods_per_key=10))
    for i in range(70):
        two.registry.pod_id(f"p{i}")
    two.registry.model_id(MODEL)
    two.table.load_state_dict(one.table.state_dict())
    dead = [f"p{i}" for i in range(0, 70, 2)]
    first = two.retire_pods(dead)
    second = two.compact_pod_ids()
    out = one.retire_pods(dead, compact=True)
    assert out["entries_cleared"] == first["entries_cleared"] > 0
    assert out["keys_tombstoned"] == first["keys_tombstoned"]
    assert out["entries_moved"] == second["entries_moved"] > 0
    assert out["num_pods"] == 35 and one._num_pods_padded() == 64
    pc.assert_tables_equal(pc.snapshot(one.table), pc.snapshot(two.table),
                           "retire(compact=True)")
    assert one.registry.id_to_pod == two.registry.id_to_pod
