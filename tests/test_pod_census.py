"""Pod census on the CPU: the native count against a plain torch count of
the same meta / pods / e_meta tensors (exact equality), and pod_census on
every backend, the sharded merge and the HTTP endpoint."""

import functools
import json
import urllib.request

import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402

pytestmark = pytest.mark.skipif(
    cpu_ext.maybe_load() is None, reason="native extension not built"
)

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    KvTable,
    NativeIndex,
    TableIndexConfig,
)
from llmd_kvcache_amd.kvblock.in_memory import InMemoryIndex  # noqa: E402
from llmd_kvcache_amd.kvblock.keys import Key, PodEntry  # noqa: E402

OCC, TOMB = 0x80000000, 0x40000000

# (capacity, P, num_pods, n_tiers, model_id, content): every shape, fleet,
# model filter and content of the issue's lists at least once.  2^20 rows
# is where a workgroup takes a second tile; 4096 x 4 is the 64 KB histogram.
CASES = [
    (1, 1, 1, 1, -1, "same"),     # under 4 rows: the dword-by-dword path
    (2, 3, 1, 1, -1, "same"),
    (4, 3, 64, 2, -1, "full"),    # the smallest table read as vectors
    (64, 1, 1, 1, -1, "same"),
    (64, 10, 64, 2, 1, "unknown"),
    (1024, 3, 130, 4, -1, "dead"),
    (1024, 3, 64, 2, 2, "full"),
    (65536, 16, 4096, 4, 1, "uniform"),
    (1 << 20, 10, 64, 2, -1, "same"),
    (1 << 20, 10, 130, 4, 1, "dead"),
]


@functools.lru_cache(maxsize=None)
def tensors(capacity, P, num_pods, n_tiers, content):
    """Seeded (meta, pods, e_meta) as int32 bit patterns; three models.
    "dead" and "unknown" tables have tombstoned and unoccupied slots that
    still hold entries; "unknown" has ids up to num_pods + 5 and tiers up
    to 3; "same" is one (pod, tier) everywhere; "full" has no zero entry."""
    g = torch.Generator().manual_seed(capacity * 31 + P)
    C = capacity
    r = lambda hi, *shape: torch.randint(0, hi, shape, generator=g)  # noqa: E731

    def meta_words(dead_share):
        kind = r(8, C) if dead_share else torch.full((C,), 7)
        m = OCC | r(3, C)
        m = torch.where(kind == 1, m | TOMB, m)
        return torch.where(kind == 0, torch.zeros_like(m), m)

    unknown = content == "unknown"
    ids = r(num_pods + (6 if unknown else 0), C, P)
    tiers = r(4 if unknown else n_tiers, C, P)
    if content == "same":
        ids, tiers = ids * 0 + (num_pods - 1), tiers * 0 + (n_tiers - 1)
    entries = (tiers << 24) | (ids + 1)
    if content not in ("same", "full"):
        entries = torch.where(r(3, C, P) > 0, entries, torch.zeros_like(entries))
    meta = meta_words(content in ("dead", "unknown"))
    return (meta.to(torch.int32), entries.reshape(-1).to(torch.int32),
            meta_words(True).to(torch.int32))


@functools.lru_cache(maxsize=None)
def reference(capacity, P, num_pods, n_tiers, model_id, content):
    """(counts [num_pods, n_tiers], summary [6]) by masks and bincount."""
    meta, pods, e_meta = (t.to(torch.int64) & 0xFFFFFFFF for t in
                          tensors(capacity, P, num_pods, n_tiers, content))

    def slots(m):
        match = ((m & OCC) != 0) & ((m & 0xFFFF) == model_id
                                    if model_id >= 0 else m == m)
        return match & ((m & TOMB) == 0), match & ((m & TOMB) != 0)

    live, tomb = slots(meta)
    rows = pods.reshape(capacity, P)
    e = rows[(rows != 0) & live[:, None]]
    pid, tier = (e & 0xFFFFFF) - 1, (e >> 24) & 0xF
    known = (pid < num_pods) & (tier < n_tiers)
    counts = torch.bincount(pid[known] * n_tiers + tier[known],
                            minlength=num_pods * n_tiers)
    full = live & ((rows != 0).sum(1) == P)
    summary = [int(live.sum()), int(tomb.sum()), int(full.sum()), e.numel(),
               int((~known).sum()), int(slots(e_meta)[0].sum())]
    return counts.reshape(num_pods, n_tiers), torch.tensor(summary)


def check_case(device, capacity, P, num_pods, n_tiers, model_id, content):
    t = KvTable(TableIndexConfig(capacity=capacity, pods_per_key=P,
                                 device=device))
    for dst, src in zip((t.meta, t.pods, t.e_meta),
                        tensors(capacity, P, num_pods, n_tiers, content)):
        dst.copy_(src)
    counts, summary = t.pod_census(model_id, num_pods, n_tiers)
    want_counts, want = reference(capacity, P, num_pods, n_tiers, model_id,
                                  content)
    print(f"{capacity}x{P} {num_pods}x{n_tiers} model {model_id} {content}: "
          f"summary {summary.tolist()} want {want.tolist()}")
    assert summary.tolist() == want.tolist()
    assert torch.equal(counts, want_counts)
    live, _, full, entries, unknown, _ = want.tolist()
    assert entries == int(want_counts.sum()) + unknown and live > 0
    assert (unknown > 0) == (content == "unknown")
    if content in ("same", "full"):
        assert full == live and entries == live * P
    if content == "same":
        assert int(want_counts[-1, -1]) == entries
    return t


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_cpu_op_equals_plain_count(case):
    t = check_case("cpu", *case)
    if case[0] == 64:  # the checks both ops share
        for bad in ((-2, 1, 1), (0x10000, 1, 1), (-1, 0, 1), (-1, 4097, 1),
                    (-1, 1, 0), (-1, 1, 5)):
            with pytest.raises(RuntimeError):
                t.pod_census(*bad)


# ---- the index layers --------------------------------------------------


def feed(idx):
    """Two models, two tiers, a removed block; every pod set fits."""
    a = [Key("m", 10 + i) for i in range(5)]
    b = [Key("other", 10 + i) for i in range(3)]
    idx.add(a, a, [PodEntry("p0", "gpu"), PodEntry("p1", "cpu")])
    idx.add(a[:2], a[:2], [PodEntry("p2", "gpu")])
    idx.add(b, b, [PodEntry("p1", "gpu"), PodEntry("p0", "cpu")])
    idx.evict(a[0], [PodEntry("p2", "gpu")])
    idx.evict(b[2], [PodEntry("p1", "gpu"), PodEntry("p0", "cpu")])


def native():
    idx = NativeIndex(TableIndexConfig(capacity=256, pods_per_key=4,
                                       tier_names=["gpu", "cpu"]))
    idx.registry.pod_id("idle")
    return idx


def holding(pods):
    return {p: {t: n for t, n in tiers.items() if n}
            for p, tiers in pods.items() if any(tiers.values())}


@pytest.mark.parametrize("model", [None, "m", "other", "nobody"])
def test_native_and_in_memory_agree(model):
    idx, ref = native(), InMemoryIndex()
    feed(idx)
    feed(ref)
    out, want = idx.pod_census(model), ref.pod_census(model)
    assert want["tables"] == [] and want["model"] == out["model"] == model
    assert holding(out["pods"]) == want["pods"]
    assert set(out["pods"]) == {"idle", "p0", "p1", "p2"}
    assert out["pods"]["idle"] == {"gpu": 0, "cpu": 0}
    if model is None:
        assert want["pods"] == {"p0": {"gpu": 5, "cpu": 2},
                                "p1": {"cpu": 5, "gpu": 2}, "p2": {"gpu": 1}}
        assert out["tables"] == [{
            "capacity": 256, "keys_live": 7, "keys_tombstoned": 1,
            "keys_full": 0, "entries": 15, "emap_occupied": 8}]
    if model == "nobody":
        assert out["tables"][0]["keys_live"] == 0
        assert "nobody" not in idx.registry.model_to_id
    # a released id's stale entry is what entries_unknown is for
    assert out["entries_unknown"] == 0
    idx.registry.release_pods(["p2"])
    after = idx.pod_census(model)
    assert "p2" not in after["pods"]
    assert after["entries_unknown"] == want["pods"].get("p2", {}).get("gpu", 0)


def test_tiered_instrumented_cost_aware_and_redis():
    from llmd_kvcache_amd.kvblock.cost_aware import CostAwareMemoryIndex
    from llmd_kvcache_amd.kvblock.fake_redis import FakeRedisServer
    from llmd_kvcache_amd.kvblock.instrumented import InstrumentedIndex
    from llmd_kvcache_amd.kvblock.redis_index import (
        RedisIndex,
        RedisIndexConfig,
    )
    from llmd_kvcache_amd.kvblock.tiered import TieredIndex

    tiered = TieredIndex(hot=native(), cold=native())
    feed(tiered.hot)
    k = [Key("m", 99)]
    tiered.cold.add(k, k, [PodEntry("p0", "gpu"), PodEntry("cold", "cpu")])
    out = InstrumentedIndex(tiered).pod_census()
    assert out["pods"]["p0"] == {"gpu": 6, "cpu": 2}
    assert out["pods"]["cold"] == {"gpu": 0, "cpu": 1}
    assert out["pods"]["idle"] == {"gpu": 0, "cpu": 0}
    assert [t["entries"] for t in out["tables"]] == [15, 2]
    cost = CostAwareMemoryIndex()
    feed(cost)
    assert cost.pod_census("other")["pods"] == {"p1": {"gpu": 2},
                                                "p0": {"cpu": 2}}
    server = FakeRedisServer()
    server.start()
    try:
        with pytest.raises(NotImplementedError):
            RedisIndex(RedisIndexConfig(
                address=f"redis://127.0.0.1:{server.port}")).pod_census()
    finally:
        server.stop()


def test_merge_census_adds_shards_but_not_the_replicated_map():
    from llmd_kvcache_amd.parallel.sharded import merge_census

    def shard(pods, unknown, live, emap):
        return {"model": "m", "pods": pods, "entries_unknown": unknown,
                "tables": [{"capacity": 64, "keys_live": live,
                            "keys_tombstoned": 1, "keys_full": 2,
                            "entries": 3 * live, "emap_occupied": emap}]}

    got = merge_census([
        shard({"a": {"gpu": 2, "cpu": 0}, "b": {"gpu": 0, "cpu": 0}}, 1, 4, 9),
        shard({"a": {"gpu": 3, "cpu": 1}, "b": {"gpu": 0, "cpu": 5}}, 0, 6, 11),
    ])
    assert got == {
        "model": "m", "entries_unknown": 1,
        "pods": {"a": {"gpu": 5, "cpu": 1}, "b": {"gpu": 0, "cpu": 5}},
        "tables": [{"capacity": 64, "keys_live": 10, "keys_tombstoned": 2,
                    "keys_full": 4, "entries": 30, "emap_occupied": 11}]}


def test_http_census_endpoint():
    from llmd_kvcache_amd.indexer import Indexer
    from llmd_kvcache_amd.service.http_server import HttpService

    class Pool:
        run = shutdown = staticmethod(lambda: None)

    idx = native()
    feed(idx)
    svc = HttpService(Indexer(tokenization_pool=Pool(), kv_block_index=idx),
                      host="127.0.0.1", port=0, coalesce=False)
    svc.start()
    try:
        for query, model in (("", None), ("?model=other", "other")):
            with urllib.request.urlopen(
                    f"http://127.0.0.1:{svc.port}/pods/census{query}",
                    timeout=10) as resp:
                assert resp.status == 200
                assert json.loads(resp.read()) == idx.pod_census(model)
    finally:
        svc.stop()
