"""Purge by pod on the CPU: the native sweep against a pure-Python model
on hand-built tables, the registry's id reuse, every backend's
clear_pods / retire_pods, the AllBlocksCleared option, the HTTP endpoints
and the sharded service over gloo."""

import json
import os
import socket
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
from llmd_kvcache_amd.kvblock.keys import Key, PodEntry  # noqa: E402

from . import pod_purge_cases as cases  # noqa: E402

MODEL = "m"
OTHER = "m2"


# ---- native op on hand-built tables ----------------------------------


@pytest.mark.parametrize("P", cases.HAND_PODS_PER_KEY)
def test_hand_rows_all_models(P):
    t = cases.hand_table(P)
    entries, keys = cases.check_hand_table(t, cases.PURGED, -1)
    meta, pods = cases.table_lists(t)
    rows = cases.hand_rows(P)
    # held only by purged pods: tombstoned
    assert meta[0] & cases.TOMB and not any(pods[0:P])
    # already tombstoned: stale entry gone, meta as before
    assert meta[32] == cases.OCC | cases.TOMB and pods[32 * P] == 0
    # the other model's row goes too under -1
    assert meta[40] & cases.TOMB
    # unpublished and survivor rows are as they were
    assert pods[13 * P] == cases.entry(0, 0) and meta[13] == 0
    assert pods[63 * P:63 * P + P][:len(rows[63][1])] == rows[63][1]
    assert meta[63] == cases.OCC
    want_keys = 2  # rows 0 and 40
    want_entries = len(rows[0][1]) + 1 + 1  # + the stale one + row 40
    if P >= 3:
        # two purged pods, one key; the survivor keeps slot and tier
        assert meta[7] & cases.TOMB
        assert meta[31] == cases.OCC
        assert pods[31 * P + P - 1] == cases.entry(5, 3)
        assert pods[31 * P] == 0
        want_keys += 1
        want_entries += 2 + 1
    assert (entries, keys) == (want_entries, want_keys)


@pytest.mark.parametrize("P", cases.HAND_PODS_PER_KEY)
def test_hand_rows_model_filter(P):
    t = cases.hand_table(P)
    cases.check_hand_table(t, cases.PURGED, 0)
    meta, pods = cases.table_lists(t)
    assert meta[40] == cases.OCC | 1  # model 1: untouched
    assert pods[40 * P] == cases.entry(4095, 3)
    # and only that row under its own filter
    t = cases.hand_table(P)
    assert cases.check_hand_table(t, cases.PURGED, 1) == (1, 1)


@pytest.mark.parametrize("P", cases.HAND_PODS_PER_KEY)
def test_single_pod_bitmaps(P):
    """Each purged id alone, with the narrowest bitmap that holds it: an
    entry whose id lies past the bitmap's end must not match."""
    for pid in cases.PURGED:
        t = cases.hand_table(P)
        cases.check_hand_table(t, [pid], -1)


@pytest.mark.parametrize("P", cases.HAND_PODS_PER_KEY)
def test_empty_bitmap_changes_nothing(P):
    t = cases.hand_table(P)
    before = cases.snapshot(t)
    assert t.purge_pods(cases.purge_words([], 64), -1) == (0, 0)
    cases.assert_tables_equal(before, cases.snapshot(t), "empty bitmap")


def test_op_rejects_bad_bitmaps():
    t = cases.hand_table(3)
    with pytest.raises(RuntimeError):
        t.purge_pods(torch.zeros(65, dtype=torch.int64), -1)
    with pytest.raises(RuntimeError):
        t.purge_pods(torch.zeros(0, dtype=torch.int64), -1)


# ---- NativeIndex ------------------------------------------------------


def _filled_native(P=10):
    """4096 interned pods; the five PURGED ids and survivors hold keys at
    tiers gpu (id 0) and a fourth tier (id 3)."""
    idx = NativeIndex(TableIndexConfig(
        capacity=1 << 10, pods_per_key=P,
        tier_names=["gpu", "cpu", "t2", "t3"]))
    for i in range(gi.MAX_PODS):
        assert idx.registry.pod_id(f"p{i}") == i
    keys = [Key(MODEL, 500 + i) for i in range(6)]
    ekeys = [Key(MODEL, 9000 + i) for i in range(6)]
    for j, pid in enumerate(cases.PURGED):
        idx.add(ekeys, keys, [PodEntry(f"p{pid}", "t3" if j & 1 else "gpu")])
    idx.add(ekeys[:3], keys[:3], [PodEntry("p5", "t3")])
    other = [Key(OTHER, 500 + i) for i in range(6)]
    idx.add(other, other, [PodEntry("p64", "gpu")])
    return idx, keys, ekeys, other


def _scores(idx, keys):
    hashes = torch.tensor([gi._to_i64(k.chunk_hash) for k in keys],
                          dtype=torch.int64)
    counts = torch.tensor([len(keys)], dtype=torch.int32)
    return idx.scores_to_map(
        idx.fused_scores(hashes, counts, keys[0].model_name, set()))[0]


def test_native_clear_and_retire():
    idx, keys, ekeys, other = _filled_native()
    purged = [f"p{p}" for p in cases.PURGED]
    out = idx.clear_pods(purged + ["nobody"], MODEL)
    assert out == {"entries_cleared": 30, "keys_tombstoned": 3,
                   "pods": sorted(purged)}
    # the pods are gone from lookup and scores; the survivor keeps its tier
    got = idx.lookup(keys, set())
    assert got == {k: [PodEntry("p5", "t3")] for k in keys[:3]}
    assert set(_scores(idx, keys)) == {"p5"}
    # the other model was filtered out and still lists p64
    assert idx.lookup(other, set()) == {
        k: [PodEntry("p64", "gpu")] for k in other}
    # the engine map is untouched
    for ek, k in zip(ekeys, keys):
        assert idx.get_request_key(ek) == k
    # ids are kept by clear_pods ...
    assert idx.registry.pod_to_id["p4095"] == 4095
    # ... and a tombstoned key comes back on re-add, without the dead pods
    idx.add(ekeys[5:], keys[5:], [PodEntry("p7", "gpu")])
    assert idx.lookup(keys[5:], set()) == {keys[5]: [PodEntry("p7", "gpu")]}

    # retire: all models, ids released, the width shrinks (4095 was last)
    out = idx.retire_pods(["p64", "p4095", "p4094"])
    assert out["pods"] == ["p4094", "p4095", "p64"]
    assert out["entries_cleared"] == 6 and out["keys_tombstoned"] == 6
    assert idx.lookup(other, set()) == {}
    assert idx.registry.num_pods == 4094
    assert idx.registry.id_to_pod[64] == ""
    assert "p64" not in idx.registry.pod_to_id
    # an empty effective set launches nothing and returns zeros
    calls = []
    real = idx.table.purge_pods
    idx.table.purge_pods = lambda *a, **k: calls.append(a) or real(*a, **k)
    assert idx.retire_pods(["p64", "ghost"]) == {
        "entries_cleared": 0, "keys_tombstoned": 0, "pods": []}
    assert idx.clear_pods([], None)["pods"] == []
    assert idx.clear_pods(["p5"], "no-such-model")["entries_cleared"] == 0
    assert calls == []
    # the freed id's next owner starts clean and scores under its own name
    idx.add(ekeys[:2], keys[:2], [PodEntry("fresh", "gpu")])
    assert idx.registry.pod_to_id["fresh"] == 64
    sc = _scores(idx, keys[:2])
    assert sc["fresh"] == 2.0 and "" not in sc and "p64" not in sc
    assert idx._filter_tensor({"", "p64"}, 4096).tolist() == [0] * 64


def test_resurrected_key_does_not_bring_a_dead_pod_back():
    idx = NativeIndex(TableIndexConfig(capacity=64, pods_per_key=3))
    k, ek = [Key(MODEL, 77)], [Key(MODEL, 78)]
    idx.add(ek, k, [PodEntry("a", "gpu"), PodEntry("b", "gpu")])
    idx.evict(ek[0], [PodEntry("a", "gpu"), PodEntry("b", "gpu")])
    # a stale entry in the tombstoned row (what a raced add leaves)
    slot = idx.table.meta.tolist().index(
        cases.i32(cases.OCC | cases.TOMB))
    idx.table.pods[slot * 3 + 1] = cases.entry(idx.registry.pod_to_id["a"], 0)
    out = idx.retire_pods(["a"])
    assert out["entries_cleared"] == 1 and out["keys_tombstoned"] == 0
    idx.add(ek, k, [PodEntry("c", "gpu")])
    assert idx.registry.pod_to_id["c"] == 0  # reuses a's id
    assert idx.lookup(k, set()) == {k[0]: [PodEntry("c", "gpu")]}


# ---- registry ---------------------------------------------------------


def test_registry_lowest_free_reuse_and_trim():
    r = Registry()
    for i in range(6):
        assert r.pod_id(f"p{i}") == i
    assert sorted(r.release_pods(["p1", "p3", "ghost"])) == [1, 3]
    assert r.id_to_pod == ["p0", "", "p2", "", "p4", "p5"]
    assert r.num_pods == 6
    assert r.pod_id("x") == 1 and r.pod_id("y") == 3 and r.pod_id("z") == 6
    # trailing ids are trimmed, holes below them too once they trail
    r.release_pods(["p5", "z"])
    assert r.num_pods == 5
    r.release_pods(["y", "p4"])
    assert r.id_to_pod == ["p0", "x", "p2"] and r.num_pods == 3
    assert r.pod_id("n") == 3
    with pytest.raises(ValueError):
        r.pod_id("")


def test_save_load_keeps_the_hole(tmp_path):
    idx = NativeIndex(TableIndexConfig(capacity=64, pods_per_key=3))
    k = [Key(MODEL, 5)]
    for p in ("a", "b", "c"):
        idx.add(k, k, [PodEntry(p, "gpu")])
    idx.retire_pods(["b"])
    path = str(tmp_path / "snap.pt")
    idx.save(path)
    fresh = NativeIndex(TableIndexConfig(capacity=64, pods_per_key=3))
    fresh.load(path)
    assert fresh.registry.id_to_pod == ["a", "", "c"]
    assert fresh.registry.pod_to_id == {"a": 0, "c": 2}
    assert fresh.lookup(k, set()) == {
        k[0]: [PodEntry("a", "gpu"), PodEntry("c", "gpu")]}
    assert fresh.registry.pod_id("d") == 1  # the next pod fills the hole
    assert fresh.registry.pod_id("e") == 3


def test_fingerprint_sees_a_released_id():
    from llmd_kvcache_amd.parallel.sharded import registry_fingerprint

    a, b = Registry(), Registry()
    for r in (a, b):
        for p in ("p0", "p1", "p2"):
            r.pod_id(p)
    a.release_pods(["p1"])
    assert registry_fingerprint(a) != registry_fingerprint(b)
    b.release_pods(["p1"])
    assert registry_fingerprint(a) == registry_fingerprint(b)


def test_rollouts_never_exhaust_the_registry():
    """MAX_PODS + 8 rollouts of one pod among a handful alive (five pods
    hold the key at the peak of a rollout, so 10 slots never overflow)."""
    idx = NativeIndex(TableIndexConfig(capacity=256, pods_per_key=10))
    k = [Key(MODEL, 1)]
    for p in ("s0", "s1", "s2"):
        idx.add(k, k, [PodEntry(p, "gpu")])
    for gen in range(gi.MAX_PODS + 8):
        idx.add(k, k, [PodEntry(f"roll-{gen}", "gpu")])
        if gen:
            out = idx.retire_pods([f"roll-{gen - 1}"])
            assert out["entries_cleared"] == 1
        assert idx.registry.num_pods <= 5
    assert idx._num_pods_padded() == 64
    assert {e.pod_identifier for e in idx.lookup(k, set())[k[0]]} == {
        "s0", "s1", "s2", f"roll-{gi.MAX_PODS + 7}"}


# ---- every backend, one scenario --------------------------------------


def _backends():
    from llmd_kvcache_amd.kvblock.cost_aware import CostAwareMemoryIndex
    from llmd_kvcache_amd.kvblock.in_memory import InMemoryIndex
    from llmd_kvcache_amd.kvblock.instrumented import InstrumentedIndex
    from llmd_kvcache_amd.kvblock.tiered import TieredIndex

    cfg = dict(capacity=1 << 10, pods_per_key=10)
    hot = NativeIndex(TableIndexConfig(**cfg))
    tiered = TieredIndex(hot=hot, cold=NativeIndex(
        TableIndexConfig(**cfg), registry=hot.registry))
    return {
        "in_memory": InMemoryIndex(),
        "cost_aware": CostAwareMemoryIndex(),
        "tiered": tiered,
        "instrumented": InstrumentedIndex(InMemoryIndex()),
        "instrumented_native": InstrumentedIndex(
            NativeIndex(TableIndexConfig(**cfg))),
    }


def _scenario(idx):
    """-> the lookups after each step, as comparable values."""
    keys = [Key(MODEL, 100 + i) for i in range(8)]
    okeys = [Key(OTHER, 100 + i) for i in range(4)]
    idx.add(keys, keys, [PodEntry("a", "gpu")])
    idx.add(keys[:6], keys[:6], [PodEntry("b", "cpu")])
    idx.add(keys[2:4], keys[2:4], [PodEntry("c", "gpu")])
    idx.add(okeys, okeys, [PodEntry("a", "gpu"), PodEntry("c", "cpu")])

    def look():
        out = []
        for ks in (keys, okeys):
            got = idx.lookup(ks, set())
            out.append({k.chunk_hash: sorted(
                (e.pod_identifier, e.device_tier) for e in v)
                for k, v in got.items()})
        return out

    seen = [look()]
    c1 = idx.clear_pods(["a", "nobody"], MODEL)
    seen.append(look())
    c2 = idx.retire_pods(["c"])
    seen.append(look())
    idx.add(keys[6:], keys[6:], [PodEntry("d", "gpu")])  # comes back
    seen.append(look())
    counts = [(c["entries_cleared"], c["keys_tombstoned"]) for c in (c1, c2)]
    return seen, counts


def test_backends_agree_with_native():
    want, want_counts = _scenario(
        NativeIndex(TableIndexConfig(capacity=1 << 10, pods_per_key=10)))
    # keys 6 and 7 were held by "a" alone
    assert want_counts == [(8, 2), (2 + 4, 0)]
    assert want[1][0] == {
        **{100 + i: [("b", "cpu")] for i in (0, 1, 4, 5)},
        **{100 + i: [("b", "cpu"), ("c", "gpu")] for i in (2, 3)}}
    assert want[1][1] == want[0][1]  # the other model was not cleared
    for name, idx in _backends().items():
        got, counts = _scenario(idx)
        assert got == want, name
        if name != "tiered":  # two tiers: every count doubles
            assert counts == want_counts, name
        else:
            assert counts == [(2 * e, 2 * k) for e, k in want_counts]


def test_tiered_releases_ids_once():
    idx = _backends()["tiered"]
    k = [Key(MODEL, 1)]
    idx.add(k, k, [PodEntry("a", "gpu"), PodEntry("b", "gpu")])
    out = idx.retire_pods(["a"])
    assert out == {"entries_cleared": 2, "keys_tombstoned": 0, "pods": ["a"]}
    assert idx.registry.id_to_pod == ["", "b"]
    assert idx.hot.lookup(k, set()) == idx.cold.lookup(k, set()) == {
        k[0]: [PodEntry("b", "gpu")]}


def test_instrumented_counts_tombstoned_keys(monkeypatch):
    from llmd_kvcache_amd.kvblock import instrumented

    class Counter:
        n = 0

        def inc(self, v=1):
            self.n += v

    c = Counter()
    monkeypatch.setattr(instrumented.collector, "evictions", c)
    idx = _backends()["instrumented_native"]
    keys = [Key(MODEL, i + 1) for i in range(3)]
    idx.add(keys, keys, [PodEntry("a", "gpu")])
    idx.add(keys[:1], keys[:1], [PodEntry("b", "gpu")])
    assert idx.retire_pods(["a"])["keys_tombstoned"] == 2
    assert c.n == 2


def test_redis_and_base_index_refuse():
    from llmd_kvcache_amd.kvblock.fake_redis import FakeRedisServer
    from llmd_kvcache_amd.kvblock.index import Index
    from llmd_kvcache_amd.kvblock.redis_index import (
        RedisIndex,
        RedisIndexConfig,
    )

    for fn in (lambda i: i.clear_pods(["a"]), lambda i: i.retire_pods(["a"])):
        with pytest.raises(NotImplementedError):
            fn(Index())
    server = FakeRedisServer()
    server.start()
    try:
        idx = RedisIndex(RedisIndexConfig(
            address=f"redis://127.0.0.1:{server.port}"))
        with pytest.raises(NotImplementedError, match="operator"):
            idx.clear_pods(["a"], MODEL)
        with pytest.raises(NotImplementedError, match="operator"):
            idx.retire_pods(["a"])
    finally:
        server.stop()


# ---- events -----------------------------------------------------------


def _event_burst():
    from llmd_kvcache_amd.kvevents.events import AllBlocksCleared, BlockStored

    a = BlockStored([11, 12], None, list(range(8)), 4)
    b = BlockStored([21, 22], None, list(range(100, 108)), 4)
    return a, b, AllBlocksCleared()


def _pods_of(idx, tp, tokens):
    keys = tp.tokens_to_kv_block_keys(None, tokens, MODEL)
    got = idx.lookup(keys, set())
    return [sorted(e.pod_identifier for e in got.get(k, [])) for k in keys]


@pytest.mark.parametrize("make", [
    lambda: NativeIndex(TableIndexConfig(capacity=256, pods_per_key=4)),
    lambda: __import__(
        "llmd_kvcache_amd.kvblock.in_memory", fromlist=["x"]).InMemoryIndex(),
], ids=["native", "in_memory"])
def test_all_blocks_cleared_option(make):
    from llmd_kvcache_amd.kvblock.token_processor import (
        ChunkedTokenDatabase,
        TokenProcessorConfig,
    )
    from llmd_kvcache_amd.kvevents.pool import (
        EventsConfig,
        EventsPool,
        digest_events,
    )

    tp = ChunkedTokenDatabase(TokenProcessorConfig(block_size=4))
    a, b, cleared = _event_burst()
    ta, tb = list(range(8)), list(range(100, 108))

    # off (the default): the event is a no-op, as before
    idx = make()
    digest_events(idx, tp, "pod-2", MODEL, [a])
    digest_events(idx, tp, "pod-1", MODEL, [a, cleared, b])
    assert _pods_of(idx, tp, ta) == [["pod-1", "pod-2"]] * 2
    assert _pods_of(idx, tp, tb) == [["pod-1"]] * 2

    # on: [store A, AllBlocksCleared, store B] leaves only B for that
    # pod; another pod holding A keeps it; the pod keeps its id
    idx = make()
    pool = EventsPool(EventsConfig(concurrency=1,
                                   clear_on_all_blocks_cleared=True), idx, tp)
    pool.digest_events("pod-2", MODEL, [a])
    pool.digest_events("pod-1", MODEL, [a, cleared, b])
    assert _pods_of(idx, tp, ta) == [["pod-2"]] * 2
    assert _pods_of(idx, tp, tb) == [["pod-1"]] * 2
    if hasattr(idx, "registry"):
        assert idx.registry.pod_to_id == {"pod-2": 0, "pod-1": 1}
    # only that model is cleared
    digest_events(idx, tp, "pod-1", OTHER, [cleared],
                  clear_on_all_blocks_cleared=True)
    assert _pods_of(idx, tp, tb) == [["pod-1"]] * 2


def test_events_option_loads_from_json():
    from llmd_kvcache_amd.config import (
        events_config_from_dict,
        events_config_from_json,
    )
    from llmd_kvcache_amd.kvevents.pool import EventsConfig

    assert EventsConfig().clear_on_all_blocks_cleared is False
    cfg = events_config_from_json(json.dumps(
        {"kv_events": {"clear_on_all_blocks_cleared": True,
                       "concurrency": 2}}))
    assert cfg.clear_on_all_blocks_cleared is True and cfg.concurrency == 2
    assert events_config_from_dict({}).clear_on_all_blocks_cleared is False


# ---- wire front: a freed id is never emitted --------------------------


def test_freed_id_scores_zero_and_has_no_name():
    """service/wirefront.py hands registry.id_to_pod to the C++ front
    unchanged; that is safe because a freed id's column is all zero (the
    front emits nonzero scores only) - pinned here on the matrix the
    front would read."""
    idx = NativeIndex(TableIndexConfig(capacity=256, pods_per_key=4))
    keys = [Key(MODEL, 10 + i) for i in range(4)]
    idx.add(keys, keys, [PodEntry("a", "gpu"), PodEntry("b", "gpu")])
    idx.retire_pods(["a"])
    hashes = torch.tensor([gi._to_i64(k.chunk_hash) for k in keys],
                          dtype=torch.int64)
    scores = idx.fused_scores(hashes, torch.tensor([4], dtype=torch.int32),
                              MODEL, set())
    names = list(idx.registry.id_to_pod)
    assert names == ["", "b"]
    assert float(scores[0, 0]) == 0.0 and float(scores[0, 1]) == 4.0
    assert idx.scores_to_map(scores) == [{"b": 4.0}]


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


def _service(index):
    from llmd_kvcache_amd.indexer import Indexer
    from llmd_kvcache_amd.service.http_server import HttpService

    indexer = Indexer(tokenization_pool=_StubPool(), kv_block_index=index)
    svc = HttpService(indexer, host="127.0.0.1", port=0, coalesce=False)
    svc.start()
    return svc


def test_http_pod_endpoints():
    idx = NativeIndex(TableIndexConfig(capacity=256, pods_per_key=4))
    keys = [Key(MODEL, 10 + i) for i in range(4)]
    okeys = [Key(OTHER, 10 + i) for i in range(2)]
    idx.add(keys, keys, [PodEntry("a", "gpu"), PodEntry("b", "gpu")])
    idx.add(okeys, okeys, [PodEntry("b", "gpu")])
    svc = _service(idx)
    try:
        code, out = _post(svc.port, "/pods/clear",
                          {"pods": ["b"], "model": MODEL})
        assert code == 200 and out == {
            "entries_cleared": 4, "keys_tombstoned": 0, "pods": ["b"]}
        assert idx.lookup(okeys, set()) != {}
        assert "b" in idx.registry.pod_to_id
        code, out = _post(svc.port, "/pods/remove", {"pods": ["b", "zz"]})
        assert code == 200 and out == {
            "entries_cleared": 2, "keys_tombstoned": 2, "pods": ["b"]}
        assert idx.registry.id_to_pod == ["a"]
        for bad in ({}, {"pods": []}, {"pods": "a"}, {"pods": [1]},
                    {"pods": [""]}, {"pods": ["a"], "model": 3}, ["a"]):
            for path in ("/pods/clear", "/pods/remove"):
                assert _post(svc.port, path, bad)[0] == 400, (path, bad)
        assert _post(svc.port, "/pods/remove", None, raw=b"{nope")[0] == 400
    finally:
        svc.stop()


def test_http_answers_501_where_the_backend_cannot():
    from llmd_kvcache_amd.kvblock.index import Index

    svc = _service(Index())
    try:
        for path in ("/pods/clear", "/pods/remove"):
            code, text = _post(svc.port, path, {"pods": ["a"]})
            assert code == 501 and "cannot purge by pod" in text
    finally:
        svc.stop()


def test_asgi_pod_endpoints():
    import asyncio

    from llmd_kvcache_amd.indexer import Indexer
    from llmd_kvcache_amd.kvblock.index import Index
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

    idx = NativeIndex(TableIndexConfig(capacity=256, pods_per_key=4))
    k = [Key(MODEL, 3)]
    idx.add(k, k, [PodEntry("a", "gpu")])
    app = AsgiIndexerApp(Indexer(tokenization_pool=_StubPool(),
                                 kv_block_index=idx), coalesce=False)
    code, body = call(app, "/pods/remove", b'{"pods": ["a"]}')
    assert code == 200 and json.loads(body) == {
        "entries_cleared": 1, "keys_tombstoned": 1, "pods": ["a"]}
    assert call(app, "/pods/clear", b'{"pods": []}')[0] == 400
    assert call(app, "/pods/clear", b"nope")[0] == 400
    app = AsgiIndexerApp(Indexer(tokenization_pool=_StubPool(),
                                 kv_block_index=Index()), coalesce=False)
    assert call(app, "/pods/clear", b'{"pods": ["a"]}')[0] == 501


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
        q.put((rank, "ok", _body_retire_through_service(rank)))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, "err", f"{e}\n{traceback.format_exc()}"))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _body_retire_through_service(rank):
    from llmd_kvcache_amd.kvblock.token_processor import (
        ChunkedTokenDatabase,
        TokenProcessorConfig,
    )
    from llmd_kvcache_amd.kvevents.events import (
        AllBlocksCleared,
        BlockStored,
        EventBatch,
    )
    from llmd_kvcache_amd.kvevents.pool import digest_events
    from llmd_kvcache_amd.parallel.service import ShardedIndexService
    from llmd_kvcache_amd.parallel.sharded import ShardedIndex
    from llmd_kvcache_amd.scorer import new_kv_block_scorer

    tp = ChunkedTokenDatabase(TokenProcessorConfig(block_size=4))
    sharded = ShardedIndex(TableIndexConfig(capacity=1 << 12, pods_per_key=10))
    svc = ShardedIndexService(sharded, tp, clear_on_all_blocks_cleared=True)
    if rank != 0:
        svc.serve()
        return list(sharded.registry.id_to_pod)

    single = NativeIndex(TableIndexConfig(capacity=1 << 12, pods_per_key=10))
    scorer = new_kv_block_scorer()
    tokens = list(range(32))
    more = list(range(200, 216))
    keys = tp.tokens_to_kv_block_keys(None, tokens, MODEL)

    def feed(pod, events):
        msg = EventBatch(ts=time.time(), events=events).encode()
        svc.apply_messages([(pod, MODEL, msg)])
        digest_events(single, tp, pod, MODEL, events,
                      clear_on_all_blocks_cleared=True)

    def agree():
        for ks in (keys, tp.tokens_to_kv_block_keys(None, more, MODEL)):
            want = {p: s for p, s in scorer.score(
                ks, single.lookup(ks, set())).items() if s}
            got = svc.score(ks, set())
            assert got == pytest.approx(want), (got, want)
        return got

    feed("pod-a", [BlockStored(list(range(100, 108)), None, tokens, 4)])
    feed("pod-b", [BlockStored(list(range(100, 104)), None, tokens[:16], 4)])
    feed("pod-c", [BlockStored(list(range(300, 304)), None, more, 4)])
    agree()
    out = svc.retire_pods(["pod-b"])
    single.retire_pods(["pod-b"])
    assert out["pods"] == ["pod-b"]
    svc.check_sync()
    agree()
    # a new pod takes the freed id on every rank
    feed("pod-d", [BlockStored(list(range(100, 106)), None, tokens[:24], 4)])
    assert sharded.registry.id_to_pod == ["pod-a", "pod-d", "pod-c"]
    svc.check_sync()
    agree()
    # ("clear", pods, model) keeps the id; AllBlocksCleared does the same
    svc.clear_pods(["pod-a"], MODEL)
    single.clear_pods(["pod-a"], MODEL)
    feed("pod-c", [AllBlocksCleared(),
                   BlockStored(list(range(300, 302)), None, more[:8], 4)])
    svc.check_sync()
    last = agree()
    assert last == {"pod-c": pytest.approx(2.0)}
    svc.stop()
    return list(sharded.registry.id_to_pod)


def test_sharded_service_retires_and_reuses_ids():
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
    assert results[0] == results[1] == ["pod-a", "pod-d", "pod-c"]
