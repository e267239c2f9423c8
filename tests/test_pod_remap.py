"""Pod-id compaction on the CPU: the native remap sweep against a
pure-Python model, the registry's plan/apply, the id gate, compact_pod_ids
and retire_pods(compact=True) on every backend, the HTTP endpoints and the
sharded service over gloo."""

import json
import os
import socket
import threading
import time
import urllib.error
import urllib.request

import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402

pytestmark = pytest.mark.skipif(
    cpu_ext.maybe_load() is None, reason="native extension not built"
)

from llmd_kvcache_amd.kvblock import gpu_index as gi  # noqa: E402
from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    NativeIndex,
    Registry,
    TableIndexConfig,
)
from llmd_kvcache_amd.kvblock.in_memory import InMemoryIndex  # noqa: E402
from llmd_kvcache_amd.kvblock.keys import Key, PodEntry  # noqa: E402
from llmd_kvcache_amd.scorer import new_kv_block_scorer  # noqa: E402
from llmd_kvcache_amd.utils.idgate import IdGate  # noqa: E402

from . import pod_purge_cases as pc  # noqa: E402
from . import pod_remap_cases as cases  # noqa: E402

MODEL = "m"
COMPACT_KEYS = ("pods_moved", "entries_moved", "entries_cleared",
                "keys_tombstoned", "num_pods", "pod_generation")


# ---- native op on hand-built tables ----------------------------------


@pytest.mark.parametrize("name", list(cases.HAND_MAPS))
@pytest.mark.parametrize("P", pc.HAND_PODS_PER_KEY)
def test_hand_rows_against_model(P, name):
    t = cases.hand_table(P)
    cases.check_hand_table_remap(t, cases.HAND_MAPS[name])


@pytest.mark.parametrize("P", pc.HAND_PODS_PER_KEY)
def test_identity_changes_nothing(P):
    t = cases.hand_table(P)
    before = pc.snapshot(t)
    assert t.remap_pods(cases.identity()) == (0, 0, 0)
    pc.assert_tables_equal(before, pc.snapshot(t), "identity")
    assert t.remap_pods([0]) == (0, 0, 0)  # n = 1, id 0 onto itself
    pc.assert_tables_equal(before, pc.snapshot(t), "identity, n = 1")


@pytest.mark.parametrize("P", pc.HAND_PODS_PER_KEY)
def test_drop_only_is_the_purge(P):
    a, b = cases.hand_table(P), cases.hand_table(P)
    entries, keys = a.purge_pods(pc.purge_words(pc.PURGED), -1)
    moved, cleared, tombs = b.remap_pods(cases.drop_only())
    assert (moved, cleared, tombs) == (0, entries, keys)
    assert entries > 0 and keys > 0
    pc.assert_tables_equal(pc.snapshot(a), pc.snapshot(b), "drop-only")


@pytest.mark.parametrize("P", pc.HAND_PODS_PER_KEY)
def test_compaction_of_the_hand_rows(P):
    t = cases.hand_table(P)
    moved, cleared, tombs = cases.check_hand_table_remap(
        t, cases.compaction())
    meta, pods = pc.table_lists(t)
    rows = pc.hand_rows(P)
    n63 = len(rows[63][1])
    # survivors only: moved to 0.., live, tier bits kept
    assert meta[63] == pc.OCC
    assert pods[63 * P:63 * P + n63] == [
        pc.entry(j, 3 * (j & 1)) for j in range(n63)]
    # held only by dropped pods: tombstoned once
    assert meta[0] == pc.OCC | pc.TOMB and not any(pods[0:P])
    # already tombstoned, stale entry dropped, no second count
    assert meta[32] == pc.OCC | pc.TOMB and pods[32 * P] == 0
    # the other model's row takes part: ids are global
    assert meta[40] == pc.OCC | pc.TOMB | 1 and pods[40 * P] == 0
    # never published: untouched, whatever it holds
    assert meta[13] == 0 and pods[13 * P] == pc.entry(0, 0)
    want_tombs = 2
    if P >= 2:  # a dropped and a moved entry side by side: stays live
        assert meta[20] == pc.OCC
        assert pods[20 * P:20 * P + 2] == [0, pc.entry(1, 1)]
    if P >= 3:
        assert meta[7] == pc.OCC | pc.TOMB
        assert meta[31] == pc.OCC
        assert pods[31 * P + P - 1] == pc.entry(0, 3)  # pod 5 -> 0
        want_tombs += 1
    assert tombs == want_tombs
    assert moved == n63 + (P >= 2) + (P >= 3)


def test_swap_and_cycle_look_each_entry_up_once():
    P = 10
    t = cases.hand_table(P)
    assert cases.check_hand_table_remap(t, cases.swap()) == (
        2 + 1, 0, 0)  # 5 and 4094 in row 63, 5 in row 31
    _, pods = pc.table_lists(t)
    assert pods[63 * P] == pc.entry(4094, 0)       # was 5
    assert pods[63 * P + 4] == pc.entry(5, 0)      # was 4094
    t = cases.hand_table(P)
    cases.check_hand_table_remap(t, cases.cycle3())
    _, pods = pc.table_lists(t)
    assert pods[63 * P:63 * P + 5] == [
        pc.entry(65, 0), pc.entry(62, 3), pc.entry(4094, 0),
        pc.entry(128, 3), pc.entry(5, 0)]


def test_ids_past_the_map_stay():
    t = cases.hand_table(10)
    before = pc.table_lists(t)
    assert cases.check_hand_table_remap(t, cases.N1_DROP)[1] > 0
    meta, pods = pc.table_lists(t)
    changed = [i for i, (a, b) in enumerate(zip(before[1], pods)) if a != b]
    assert all((before[1][i] & 0xFFFFFF) - 1 == 0 for i in changed)


@pytest.mark.parametrize("P", [3, 10])
def test_random_table_against_model(P):
    t = pc.random_table(1024, P, seed=P)
    remap = cases.random_injective(130, seed=P)
    moved, cleared, tombs = cases.check_hand_table_remap(t, remap)
    assert moved > 0 and cleared > 0 and tombs > 0


def test_op_rejects_bad_maps():
    t = cases.hand_table(3)
    ops, args = t.ops, t._t()
    i32 = torch.int32
    bad = [
        torch.zeros(4, dtype=torch.int64),                 # dtype
        torch.zeros((2, 2), dtype=i32),                    # 2-D
        torch.zeros(0, dtype=i32),                         # n = 0
        torch.full((4097,), -1, dtype=i32),                # n = 4097
        torch.tensor([0, -2], dtype=i32),                  # below -1
        torch.tensor([0, 4096], dtype=i32),                # past the last id
        torch.tensor([3, 1, 3], dtype=i32),                # two olds, one new
        torch.arange(8, dtype=i32)[::2],                   # not contiguous
    ]
    before = pc.snapshot(t)
    for remap in bad:
        with pytest.raises(RuntimeError):
            ops.cpu_remap_pods(*args, remap)
    pc.assert_tables_equal(before, pc.snapshot(t), "rejected maps")
    assert ops.cpu_remap_pods(
        *args, torch.full((4096,), -1, dtype=i32))[1] > 0  # n = 4096 is fine


# ---- registry ---------------------------------------------------------


def _registry(names):
    r = Registry()
    with r._lock:
        r._set_pods(names)
    return r


def test_registry_plan_and_apply():
    r = _registry(["p0", "", "p2", "", "p4", "p5"])
    assert r.pod_generation == 0
    plan = r.plan_pod_compaction()
    assert plan == [0, -1, 1, -1, 2, 3]
    r.apply_pod_compaction(plan)
    assert r.id_to_pod == ["p0", "p2", "p4", "p5"]
    assert r.pod_to_id == {"p0": 0, "p2": 1, "p4": 2, "p5": 3}
    assert r.num_pods == 4 and r.pod_generation == 1
    assert r._free_pod_ids == []
    assert r.plan_pod_compaction() is None        # hole-free
    assert r.pod_id("new") == 4                    # appends at the end
    assert Registry().plan_pod_compaction() is None  # empty
    assert _registry(["a", "b"]).plan_pod_compaction() is None
    with pytest.raises(ValueError):
        r.apply_pod_compaction([0, 1])             # wrong length


# ---- TableIndex end to end --------------------------------------------

N_PROMPTS, PROMPT_LEN = 3, 6


def _prompt(i):
    return [Key(MODEL, 1000 * (i + 1) + j) for j in range(PROMPT_LEN)]


def _fleet(n_names):
    """A NativeIndex with n_names pods interned and an InMemoryIndex, fed
    the same adds and evicts: each of the last 24 names (8 per prompt, so
    no pod set overflows) holds the first 1 + i % PROMPT_LEN keys of
    prompt i % N_PROMPTS on tier i % 2, every seventh loses its first key
    again."""
    idx = NativeIndex(TableIndexConfig(capacity=1 << 12, pods_per_key=16,
                                       tier_names=["gpu", "cpu"]))
    ref = InMemoryIndex()
    for i in range(n_names):
        assert idx.registry.pod_id(f"p{i}") == i
    for i in range(max(0, n_names - 24), n_names):
        keys = _prompt(i % N_PROMPTS)[:1 + i % PROMPT_LEN]
        ents = [PodEntry(f"p{i}", ("gpu", "cpu")[i % 2])]
        for x in (idx, ref):
            x.add(keys, keys, ents)
            if i % 7 == 3:
                x.evict(keys[0], ents)
    return idx, ref


def _by_name(idx):
    out = []
    for i in range(N_PROMPTS):
        keys = _prompt(i)
        hashes = torch.tensor([gi._to_i64(k.chunk_hash) for k in keys],
                              dtype=torch.int64)
        counts = torch.tensor([len(keys)], dtype=torch.int32)
        out.append(idx.scores_to_map(
            idx.fused_scores(hashes, counts, MODEL, set()))[0])
    return out


def _ref_by_name(ref):
    scorer = new_kv_block_scorer()
    out = []
    for i in range(N_PROMPTS):
        keys = _prompt(i)
        out.append({p: s for p, s in scorer.score(
            keys, ref.lookup(keys, set())).items() if s})
    return out


def _same(got, want):
    """Per-prompt score maps equal up to float32 rounding of the tier
    weights."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == pytest.approx(w), (got, want)
    return True


def _lookups(idx):
    return [{k.chunk_hash: sorted((e.pod_identifier, e.device_tier)
                                  for e in v)
             for k, v in idx.lookup(_prompt(i), set()).items()}
            for i in range(N_PROMPTS)]


@pytest.mark.parametrize("n_names,n_dead,padded_before", [
    (40, 32, 64), (520, 512, 576)])
def test_compaction_keeps_scores_by_name(n_names, n_dead, padded_before):
    idx, ref = _fleet(n_names)
    dead = [f"p{i}" for i in range(n_dead)]
    idx.retire_pods(dead)
    ref.retire_pods(dead)
    want = _ref_by_name(ref)
    assert any(want) and _same(_by_name(idx), want)
    looks = _lookups(idx)
    assert idx.registry.num_pods == n_names
    assert idx._num_pods_padded() == padded_before

    out = idx.compact_pod_ids()
    assert out == {"pods_moved": 8, "entries_moved": out["entries_moved"],
                   "entries_cleared": 0, "keys_tombstoned": 0,
                   "num_pods": 8, "pod_generation": 1}
    assert out["entries_moved"] > 0
    assert idx.registry.num_pods == 8
    assert idx._num_pods_padded() == 64
    assert idx.registry.id_to_pod == [f"p{i}" for i in range(n_dead, n_names)]
    assert _same(_by_name(idx), want)
    assert _lookups(idx) == looks  # the same names and tiers

    # a second call finds nothing to do
    calls = []
    real = idx.table.remap_pods
    idx.table.remap_pods = lambda *a: calls.append(a) or real(*a)
    assert idx.compact_pod_ids() == {
        "pods_moved": 0, "entries_moved": 0, "entries_cleared": 0,
        "keys_tombstoned": 0, "num_pods": 8, "pod_generation": 1}
    assert calls == [] and idx.registry.pod_generation == 1

    # a new pod takes the first id past the survivors
    k = _prompt(0)[:2]
    for x in (idx, ref):
        x.add(k, k, [PodEntry("fresh", "gpu")])
    assert idx.registry.pod_to_id["fresh"] == 8
    assert _same(_by_name(idx), _ref_by_name(ref))


def test_retire_with_compact_is_retire_then_compact():
    a, _ = _fleet(40)
    b, _ = _fleet(40)
    dead = [f"p{i}" for i in range(0, 40, 3)] + ["nobody"]
    first = a.retire_pods(dead)
    second = a.compact_pod_ids()
    calls = []
    real = b.table.remap_pods
    b.table.remap_pods = lambda *x: calls.append(x) or real(*x)
    out = b.retire_pods(dead, compact=True)
    assert len(calls) == 1  # one sweep
    assert set(out) == set(COMPACT_KEYS) | {"pods"}
    assert out["pods"] == first["pods"]
    assert out["entries_cleared"] == first["entries_cleared"] > 0
    assert out["keys_tombstoned"] == first["keys_tombstoned"] > 0
    assert out["entries_moved"] == second["entries_moved"] > 0
    assert out["pods_moved"] == second["pods_moved"]
    assert (out["num_pods"], out["pod_generation"]) == (26, 1)
    pc.assert_tables_equal(pc.snapshot(a.table), pc.snapshot(b.table),
                           "retire(compact=True)")
    assert a.registry.id_to_pod == b.registry.id_to_pod
    assert a.registry.pod_to_id == b.registry.pod_to_id
    # retiring the highest ids only: nobody moves, the entries still go
    c, _ = _fleet(40)
    d, _ = _fleet(40)
    top = ["p38", "p39"]
    want = c.retire_pods(top)
    got = d.retire_pods(top, compact=True)
    assert got["entries_cleared"] == want["entries_cleared"] > 0
    assert got["pods_moved"] == 0 and got["num_pods"] == 38
    pc.assert_tables_equal(pc.snapshot(c.table), pc.snapshot(d.table), "top")
    assert c.registry.id_to_pod == d.registry.id_to_pod
    # nothing known and no hole: zeros, no sweep
    assert d.retire_pods(["ghost"], compact=True)["entries_moved"] == 0


def test_a_stale_entry_of_a_free_id_is_reported():
    idx, _ = _fleet(12)
    idx.retire_pods(["p2"])
    P = idx.cfg.pods_per_key
    slot = next(i for i, m in enumerate(idx.table.meta.tolist())
                if (m & 0xFFFFFFFF) & pc.OCC)
    free = idx.table.pods[slot * P:slot * P + P].tolist().index(0)
    idx.table.pods[slot * P + free] = pc.entry(2, 0)  # a free id's entry
    out = idx.compact_pod_ids()
    assert out["entries_cleared"] == 1 and out["keys_tombstoned"] == 0
    assert out["num_pods"] == 11


def test_save_after_compaction_loads_by_name(tmp_path):
    idx, ref = _fleet(40)
    dead = [f"p{i}" for i in range(32)]
    idx.retire_pods(dead, compact=True)
    ref.retire_pods(dead)
    path = str(tmp_path / "snap.pt")
    idx.save(path)
    fresh = NativeIndex(TableIndexConfig(capacity=1 << 12, pods_per_key=16,
                                         tier_names=["gpu", "cpu"]))
    fresh.load(path)
    assert fresh.registry.id_to_pod == [f"p{i}" for i in range(32, 40)]
    assert _same(_by_name(fresh), _ref_by_name(ref))


# ---- the id gate ------------------------------------------------------


def _wait_until(cond, what):
    for _ in range(2000):
        if cond():
            return
        time.sleep(0.001)
    raise AssertionError(f"timed out waiting for {what}")


def test_gate_is_reentrant_and_refuses_an_upgrade():
    g = IdGate()
    with g.shared, g.shared:
        with pytest.raises(RuntimeError):
            g.exclusive.__enter__()
    with g.exclusive, g.exclusive, g.shared:
        pass
    with g.exclusive:  # everything was released
        pass


def test_compaction_waits_for_shared_spans():
    idx, _ = _fleet(12)
    idx.retire_pods(["p0"])
    reg = idx.registry
    inside, leave, nested_ok = (threading.Event() for _ in range(3))
    late_in = threading.Event()
    done = []

    def holder():
        with reg.ids_shared():
            inside.set()
            _wait_until(lambda: reg._id_gate.waiting_exclusive == 1,
                        "the compaction to queue up")
            with reg.ids_shared():  # nested: never waits
                nested_ok.set()
            leave.wait(10)

    def compactor():
        done.append(idx.compact_pod_ids())

    def late_reader():
        with reg.ids_shared():
            late_in.set()
            assert done  # let in only after the compaction

    th = threading.Thread(target=holder)
    th.start()
    assert inside.wait(10)
    tc = threading.Thread(target=compactor)
    tc.start()
    assert nested_ok.wait(10)
    tl = threading.Thread(target=late_reader)
    tl.start()
    time.sleep(0.01)
    # the shared holder blocks the compaction, the waiting compaction
    # blocks the new outermost entrant
    assert not done and not late_in.is_set()
    assert reg.pod_generation == 0
    leave.set()
    for t in (th, tc, tl):
        t.join(10)
        assert not t.is_alive()
    assert done[0]["pod_generation"] == 1 and late_in.is_set()


def test_hammer_scores_are_never_misattributed():
    """4 readers score single keys through the indexer while a writer
    retires the oldest pod, compacts and interns a new one.  Pod p{i} only
    ever holds key 5000 + i, so a score for that key under any other name
    is a misattribution."""
    from llmd_kvcache_amd.indexer import Indexer

    class Pool:
        run = shutdown = staticmethod(lambda: None)

    idx = NativeIndex(TableIndexConfig(capacity=1 << 10, pods_per_key=4))
    indexer = Indexer(tokenization_pool=Pool(), kv_block_index=idx)
    key = lambda i: [Key(MODEL, 5000 + i)]  # noqa: E731
    LIVE, ROUNDS, READS = 6, 60, 150
    for i in range(LIVE):
        idx.add(key(i), key(i), [PodEntry(f"p{i}", "gpu")])
    newest = [LIVE - 1]
    bad, hits = [], [0]

    def reader(seed):
        for n in range(READS):
            i = max(0, newest[0] - (n + seed) % (LIVE + 2))
            got = indexer._score_keys(key(i), [])
            if set(got) - {f"p{i}"}:
                bad.append((i, got))
            hits[0] += bool(got)

    def writer():
        for r in range(ROUNDS):
            if r % 2:
                idx.retire_pods([f"p{r}"], compact=True)
            else:
                idx.retire_pods([f"p{r}"])
                idx.compact_pod_ids()
            n = LIVE + r
            idx.add(key(n), key(n), [PodEntry(f"p{n}", "gpu")])
            newest[0] = n

    threads = [threading.Thread(target=reader, args=(s,)) for s in range(4)]
    threads.append(threading.Thread(target=writer))
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
        assert not t.is_alive()
    assert bad == []
    assert hits[0] > 0
    assert idx.registry.pod_generation == ROUNDS
    assert idx.registry.id_to_pod == [
        f"p{i}" for i in range(ROUNDS, ROUNDS + LIVE)]


# ---- other backends ---------------------------------------------------


def _tiered():
    from llmd_kvcache_amd.kvblock.tiered import TieredIndex

    cfg = dict(capacity=1 << 10, pods_per_key=10)
    hot = NativeIndex(TableIndexConfig(**cfg))
    return TieredIndex(hot=hot, cold=NativeIndex(
        TableIndexConfig(**cfg), registry=hot.registry))


@pytest.mark.parametrize("one_sweep", [False, True])
def test_tiered_remaps_both_tiers(one_sweep):
    idx = _tiered()
    both = [Key(MODEL, 1), Key(MODEL, 2)]
    cold_only = [Key(MODEL, 3)]
    for i in range(6):
        idx.add(both, both, [PodEntry(f"p{i}", "gpu")])
    idx.cold.add(cold_only, cold_only, [PodEntry("p5", "gpu")])
    dead = [f"p{i}" for i in range(4)]
    if one_sweep:
        out = idx.retire_pods(dead, compact=True)
        assert out["entries_cleared"] == 2 * 2 * 4 and out["pods"] == dead
    else:
        idx.retire_pods(dead)
        out = idx.compact_pod_ids()
        assert out["entries_cleared"] == 0
    assert out["entries_moved"] == 2 * 2 * 2 + 1  # both tiers, + cold only
    assert out["pods_moved"] == 2 and out["num_pods"] == 2
    assert out["pod_generation"] == 1
    assert idx.registry.id_to_pod == ["p4", "p5"]
    want = {k: [PodEntry("p4", "gpu"), PodEntry("p5", "gpu")] for k in both}
    assert idx.hot.lookup(both, set()) == idx.cold.lookup(both, set()) == want
    # the key that lives in the cold tier alone scores under its own name
    hashes = torch.tensor([3], dtype=torch.int64)
    counts = torch.tensor([1], dtype=torch.int32)
    scores = idx.fused_scores(hashes, counts, MODEL, set())
    assert idx.scores_to_map(scores) == [{"p5": 1.0}]
    assert idx.lookup(cold_only, set()) == {
        cold_only[0]: [PodEntry("p5", "gpu")]}


def test_tiered_with_separate_registries_compacts_each():
    from llmd_kvcache_amd.kvblock.tiered import TieredIndex

    cfg = dict(capacity=256, pods_per_key=4)
    idx = TieredIndex(hot=NativeIndex(TableIndexConfig(**cfg)),
                      cold=NativeIndex(TableIndexConfig(**cfg)))
    k = [Key(MODEL, 1)]
    idx.add(k, k, [PodEntry("a", "gpu"), PodEntry("b", "gpu")])
    idx.retire_pods(["a"])
    out = idx.compact_pod_ids()
    assert out["entries_moved"] == 2 and out["num_pods"] == 1
    assert idx.hot.registry.id_to_pod == idx.cold.registry.id_to_pod == ["b"]
    assert idx.lookup(k, set()) == {k[0]: [PodEntry("b", "gpu")]}


def test_backends_without_dense_ids_return_zeros():
    from llmd_kvcache_amd.kvblock.cost_aware import CostAwareMemoryIndex
    from llmd_kvcache_amd.kvblock.fake_redis import FakeRedisServer
    from llmd_kvcache_amd.kvblock.redis_index import (
        RedisIndex,
        RedisIndexConfig,
    )

    zeros = {"pods_moved": 0, "entries_moved": 0, "entries_cleared": 0,
             "keys_tombstoned": 0, "num_pods": None, "pod_generation": 0}
    k = [Key(MODEL, 1)]
    for idx in (InMemoryIndex(), CostAwareMemoryIndex()):
        idx.add(k, k, [PodEntry("a", "gpu"), PodEntry("b", "gpu")])
        assert idx.compact_pod_ids() == zeros
        out = idx.retire_pods(["a"], compact=True)
        assert out == {**zeros, "entries_cleared": 1, "pods": ["a"]}
        assert idx.lookup(k, set()) == {k[0]: [PodEntry("b", "gpu")]}
    server = FakeRedisServer()
    server.start()
    try:
        idx = RedisIndex(RedisIndexConfig(
            address=f"redis://127.0.0.1:{server.port}"))
        assert idx.compact_pod_ids() == zeros
    finally:
        server.stop()


def test_instrumented_passes_through_and_counts(monkeypatch):
    from llmd_kvcache_amd.kvblock import instrumented

    class Counter:
        n = 0

        def inc(self, v=1):
            self.n += v

    c = Counter()
    monkeypatch.setattr(instrumented.collector, "evictions", c)
    idx = instrumented.InstrumentedIndex(
        NativeIndex(TableIndexConfig(capacity=256, pods_per_key=4)))
    keys = [Key(MODEL, i + 1) for i in range(3)]
    idx.add(keys, keys, [PodEntry("a", "gpu")])
    idx.add(keys[:1], keys[:1], [PodEntry("b", "gpu")])
    out = idx.retire_pods(["a"], compact=True)
    assert out["keys_tombstoned"] == 2 and out["entries_moved"] == 1
    assert c.n == 2
    assert idx.compact_pod_ids()["pods_moved"] == 0 and c.n == 2
    assert idx.registry.id_to_pod == ["b"]


# ---- HTTP -------------------------------------------------------------


def _post(port, path, payload, raw=None):
    body = raw if raw is not None else json.dumps(payload).encode()
    req = urllib.request.Request(
        f"http://127.0.0.1:{port}{path}", data=body,
        headers={"Content-Type": "application/json"})
    try:
        with urllib.request.urlopen(req, timeout=10) as resp:
            return resp.status, json.loads(resp.read())
    except urllib.error.HTTPError as e:
        return e.code, e.read().decode()


class _StubPool:
    def run(self):
        pass

    def shutdown(self):
        pass

    def tokenize(self, render_req, prompt, model):
        return []


def _http_index():
    idx = NativeIndex(TableIndexConfig(capacity=256, pods_per_key=4))
    keys = [Key(MODEL, 10 + i) for i in range(4)]
    for name in "abcd":
        idx.add(keys, keys, [PodEntry(name, "gpu")])
    return idx, keys


def _redis_index(server):
    from llmd_kvcache_amd.kvblock.redis_index import (
        RedisIndex,
        RedisIndexConfig,
    )

    return RedisIndex(RedisIndexConfig(
        address=f"redis://127.0.0.1:{server.port}"))


def test_http_compact_endpoints():
    from llmd_kvcache_amd.indexer import Indexer
    from llmd_kvcache_amd.kvblock.fake_redis import FakeRedisServer
    from llmd_kvcache_amd.service.http_server import HttpService

    def service(index):
        svc = HttpService(Indexer(tokenization_pool=_StubPool(),
                                  kv_block_index=index),
                          host="127.0.0.1", port=0, coalesce=False)
        svc.start()
        return svc

    idx, keys = _http_index()
    svc = service(idx)
    try:
        assert _post(svc.port, "/pods/remove", {"pods": ["a"]})[0] == 200
        assert idx.registry.id_to_pod == ["", "b", "c", "d"]
        code, out = _post(svc.port, "/pods/compact", {})
        assert code == 200 and out == {
            "pods_moved": 3, "entries_moved": 12, "entries_cleared": 0,
            "keys_tombstoned": 0, "num_pods": 3, "pod_generation": 1}
        code, out = _post(svc.port, "/pods/compact", None, raw=b"")
        assert code == 200 and out["pods_moved"] == 0
        assert _post(svc.port, "/pods/compact", {"pods": ["a"]})[0] == 400
        assert _post(svc.port, "/pods/compact", None, raw=b"{no")[0] == 400
        code, out = _post(svc.port, "/pods/remove",
                          {"pods": ["b"], "compact": True})
        assert code == 200 and out == {
            "pods_moved": 2, "entries_moved": 8, "entries_cleared": 4,
            "keys_tombstoned": 0, "num_pods": 2, "pod_generation": 2,
            "pods": ["b"]}
        assert idx.registry.id_to_pod == ["c", "d"]
        for bad in ("yes", 1, None, []):
            code, _ = _post(svc.port, "/pods/remove",
                            {"pods": ["c"], "compact": bad})
            assert code == 400, bad
        assert idx.registry.id_to_pod == ["c", "d"]
        code, out = _post(svc.port, "/pods/remove",
                          {"pods": ["c"], "compact": False})
        assert code == 200 and "pods_moved" not in out
    finally:
        svc.stop()
    server = FakeRedisServer()
    server.start()
    svc = service(_redis_index(server))
    try:
        code, out = _post(svc.port, "/pods/compact", {})
        assert code == 200 and out["num_pods"] is None
        assert out["pods_moved"] == 0
    finally:
        svc.stop()
        server.stop()


def test_asgi_compact_endpoints():
    import asyncio

    from llmd_kvcache_amd.indexer import Indexer
    from llmd_kvcache_amd.kvblock.fake_redis import FakeRedisServer
    from llmd_kvcache_amd.service.asgi import AsgiIndexerApp

    def call(app, path, body):
        sent = []

        async def receive():
            return {"type": "http.request", "body": body, "more_body": False}

        async def send(msg):
            sent.append(msg)

        asyncio.run(app({"type": "http", "method": "POST", "path": path},
                        receive, send))
        return sent[0]["status"], sent[1]["body"]

    def app_for(index):
        return AsgiIndexerApp(Indexer(tokenization_pool=_StubPool(),
                                      kv_block_index=index), coalesce=False)

    idx, keys = _http_index()
    app = app_for(idx)
    assert call(app, "/pods/remove", b'{"pods": ["a"]}')[0] == 200
    code, body = call(app, "/pods/compact", b"")
    assert code == 200 and json.loads(body) == {
        "pods_moved": 3, "entries_moved": 12, "entries_cleared": 0,
        "keys_tombstoned": 0, "num_pods": 3, "pod_generation": 1}
    assert call(app, "/pods/compact", b"{}")[0] == 200
    assert call(app, "/pods/compact", b"[1]")[0] == 400
    assert call(app, "/pods/compact", b"nope")[0] == 400
    code, body = call(app, "/pods/remove",
                      b'{"pods": ["b"], "compact": true}')
    out = json.loads(body)
    assert code == 200 and out["pods_moved"] == 2 and out["pods"] == ["b"]
    assert out["entries_cleared"] == 4 and out["pod_generation"] == 2
    assert idx.registry.id_to_pod == ["c", "d"]
    assert call(app, "/pods/remove",
                b'{"pods": ["c"], "compact": "yes"}')[0] == 400
    assert idx.registry.id_to_pod == ["c", "d"]
    server = FakeRedisServer()
    server.start()
    try:
        code, body = call(app_for(_redis_index(server)), "/pods/compact",
                          b"{}")
        assert code == 200 and json.loads(body)["num_pods"] is None
    finally:
        server.stop()


# ---- sharded service over gloo ----------------------------------------


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world_size, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world_size)
        q.put((rank, "ok", _body_compact_through_service(rank)))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, "err", f"{e}\n{traceback.format_exc()}"))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _body_compact_through_service(rank):
    from llmd_kvcache_amd.kvblock.token_processor import (
        ChunkedTokenDatabase,
        TokenProcessorConfig,
    )
    from llmd_kvcache_amd.kvevents.events import BlockStored, EventBatch
    from llmd_kvcache_amd.kvevents.pool import digest_events
    from llmd_kvcache_amd.parallel.service import ShardedIndexService
    from llmd_kvcache_amd.parallel.sharded import ShardedIndex

    tp = ChunkedTokenDatabase(TokenProcessorConfig(block_size=4))
    sharded = ShardedIndex(TableIndexConfig(capacity=1 << 12, pods_per_key=10))
    svc = ShardedIndexService(sharded, tp)
    state = lambda: (list(sharded.registry.id_to_pod),  # noqa: E731
                     sharded.registry.pod_generation)
    if rank != 0:
        svc.serve()
        return state()

    single = NativeIndex(TableIndexConfig(capacity=1 << 12, pods_per_key=10))
    scorer = new_kv_block_scorer()
    tokens = list(range(32))
    more = list(range(200, 216))
    prompts = [tp.tokens_to_kv_block_keys(None, t, MODEL)
               for t in (tokens, more)]

    def feed(pod, events):
        msg = EventBatch(ts=time.time(), events=events).encode()
        svc.apply_messages([(pod, MODEL, msg)])
        digest_events(single, tp, pod, MODEL, events)

    def agree():
        got_all = []
        for ks in prompts:
            want = {p: s for p, s in scorer.score(
                ks, single.lookup(ks, set())).items() if s}
            got = svc.score(ks, set())
            assert got == pytest.approx(want), (got, want)
            got_all.append(got)
        return got_all

    feed("pod-a", [BlockStored(list(range(100, 108)), None, tokens, 4)])
    feed("pod-b", [BlockStored(list(range(100, 104)), None, tokens[:16], 4)])
    feed("pod-c", [BlockStored(list(range(300, 304)), None, more, 4)])
    feed("pod-d", [BlockStored(list(range(100, 106)), None, tokens[:24], 4)])
    before = agree()
    svc.retire_pods(["pod-a"])
    single.retire_pods(["pod-a"])
    before = agree()
    assert sharded.registry.id_to_pod == ["", "pod-b", "pod-c", "pod-d"]
    out = svc.compact_pod_ids()          # the ("compact",) broadcast
    assert out["pods_moved"] == 3 and out["num_pods"] == 3
    assert out["pod_generation"] == 1
    assert sharded.registry.id_to_pod == ["pod-b", "pod-c", "pod-d"]
    svc.check_sync()
    assert agree() == before             # by name, unchanged
    out = svc.retire_pods(["pod-b"], compact=True)  # ("retire", pods, True)
    single.retire_pods(["pod-b"])
    assert out["pods"] == ["pod-b"] and out["pod_generation"] == 2
    assert sharded.registry.id_to_pod == ["pod-c", "pod-d"]
    svc.check_sync()
    last = agree()
    assert last[0] == {"pod-d": pytest.approx(6.0)}
    feed("pod-e", [BlockStored(list(range(100, 102)), None, tokens[:8], 4)])
    assert sharded.registry.pod_to_id["pod-e"] == 2
    svc.check_sync()
    agree()
    svc.stop()
    return state()


def test_sharded_service_compacts_on_every_rank():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in procs:
        rank, status, payload = q.get()
        assert status == "ok", f"rank {rank} failed: {payload}"
        results[rank] = payload
    for p in procs:
        p.join(timeout=30)
    assert results[0] == results[1] == (["pod-c", "pod-d", "pod-e"], 2)
