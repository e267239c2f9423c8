"""ShardedIndex top-n over gloo: sharded_top_pods against cpu_score_topk of
sharded_scores under both merge strategies, error-flag propagation, and
the Indexer surface.  Workers start as in tests/test_sharded.py."""

import random

import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402

from . import test_sharded as ts  # noqa: E402

pytestmark = pytest.mark.skipif(
    cpu_ext.maybe_load() is None, reason="native extension not built"
)

MODEL = ts.MODEL
_ts_worker = ts._worker


def _worker(rank, world_size, port, fn_name, q):
    # ts._worker looks its body up in its own module: lend it ours
    ts.__dict__.setdefault(fn_name, globals()[fn_name])
    _ts_worker(rank, world_size, port, fn_name, q)


def run(monkeypatch, fn_name, world_size=2):
    monkeypatch.setattr(ts, "_worker", _worker)
    return ts.run_distributed(fn_name, world_size=world_size)


def _sharded(force_rs, capacity=1 << 12):
    from llmd_kvcache_amd.kvblock.gpu_index import TableIndexConfig
    from llmd_kvcache_amd.parallel.sharded import ShardedIndex

    idx = ShardedIndex(TableIndexConfig(capacity=capacity, pods_per_key=10))
    idx.force_reduce_scatter = force_rs
    return idx


def _flat(prompts):
    from llmd_kvcache_amd.kvblock.gpu_index import _to_i64

    flat = [_to_i64(k.chunk_hash) for p in prompts for k in p]
    counts = torch.tensor([0] + [len(p) for p in prompts])
    return (torch.tensor(flat, dtype=torch.int64),
            torch.cumsum(counts, 0).to(torch.int32))


def _topk_vs_scores(world_size, force_rs):
    from llmd_kvcache_amd.kvblock.keys import Key, PodEntry

    rng = random.Random(91)  # the same stream on every rank
    idx = _sharded(force_rs)
    for _ in range(80):
        start, n = rng.randrange(50), rng.randrange(1, 8)
        keys = [Key(MODEL, 7000 + start + i) for i in range(n)]
        # two pods per write share prefix and tier: equal scores
        pod, tier = rng.randrange(8), rng.choice(["gpu", "cpu"])
        idx.add(keys, keys, [PodEntry(f"pod-{pod}", tier),
                             PodEntry(f"pod-{pod + 8}", tier)])
    bad = []
    for trial in range(6):
        prompts = [[]]  # a prompt without keys rides along
        for _ in range(rng.randrange(world_size, world_size * 3 + 1)):
            start, n = rng.randrange(50), rng.randrange(1, 10)
            prompts.append([Key(MODEL, 7000 + start + i) for i in range(n)])
        flat, offsets = _flat(prompts)
        scores = idx.sharded_scores(flat, offsets, MODEL, set())
        for top_n in (1, 4, 16):
            ids, top = idx.sharded_top_pods(flat, offsets, MODEL, set(), top_n)
            want_ids, want_top = cpu_ext.require().cpu_score_topk(scores,
                                                                  top_n)
            if not (torch.equal(ids, want_ids) and torch.equal(
                    top.view(torch.int32), want_top.view(torch.int32))):
                bad.append((trial, top_n, ids.tolist(), want_ids.tolist()))
    return bad


def _body_topk_all_reduce(rank, world_size):
    return _topk_vs_scores(world_size, False)


def _body_topk_reduce_scatter(rank, world_size):
    return _topk_vs_scores(world_size, True)


@pytest.mark.parametrize("world_size", [2, 4])
@pytest.mark.parametrize("body", ["_body_topk_all_reduce",
                                  "_body_topk_reduce_scatter"])
def test_sharded_top_pods_is_topk_of_sharded_scores(monkeypatch, body,
                                                    world_size):
    results = run(monkeypatch, body, world_size)
    for rank, bad in results.items():
        assert bad == [], f"rank {rank}: {bad[:2]}"


def _body_topk_probe_failure(rank, world_size):
    from llmd_kvcache_amd.kvblock.keys import Key, PodEntry

    outcomes = []
    for force_rs in (False, True):
        idx = _sharded(force_rs, capacity=1 << 10)
        keys = [Key(MODEL, 40 + i) for i in range(8)]
        idx.add(keys, keys, [PodEntry("pod-a", "gpu")])
        flat, offsets = _flat([keys[:4], keys[4:]])
        if rank == 1:
            real = idx.local.table.lookup
            idx.local.table.lookup = lambda *a, **kw: (_ for _ in ()).throw(
                RuntimeError("injected"))
        outcome = "no-raise"
        try:
            idx.sharded_top_pods(flat, offsets, MODEL, set(), 2)
        except RuntimeError as e:
            outcome = "peer" if "peer rank" in str(e) else "local"
        if rank == 1:
            idx.local.table.lookup = real
        # no collective is left half done: the next call answers in full
        ids, top = idx.sharded_top_pods(flat, offsets, MODEL, set(), 2)
        outcomes.append((outcome, ids.tolist(), top.tolist()))
    return outcomes


def test_sharded_top_pods_probe_failure_raises_everywhere(monkeypatch):
    results = run(monkeypatch, "_body_topk_probe_failure")
    full = [[0, -1]] * 2, [[4.0, 0.0]] * 2
    assert results[0] == [("peer", *full)] * 2
    assert results[1] == [("local", *full)] * 2


def _body_indexer_top_pods(rank, world_size):
    from llmd_kvcache_amd.indexer import Config, Indexer
    from llmd_kvcache_amd.kvblock.keys import PodEntry
    from llmd_kvcache_amd.kvblock.token_processor import TokenProcessorConfig

    idx = _sharded(False)
    ix = Indexer(Config(token_processor=TokenProcessorConfig(block_size=4)),
                 kv_block_index=idx)
    tokens = list(range(1, 25))  # six blocks
    keys = ix.tokens_processor.tokens_to_kv_block_keys(None, tokens, MODEL)
    # ids in interning order: pod-z 0, pod-a 1, pod-m 2
    idx.add(keys, keys, [PodEntry("pod-z", "gpu"), PodEntry("pod-a", "gpu")])
    idx.add(keys[:3], keys[:3], [PodEntry("pod-m", "gpu")])
    return ix.top_pods_tokens_batch([tokens, tokens[:4], [1, 2]], MODEL, [], 2)


def test_indexer_top_pods_over_sharded_index_orders_ties_by_id(monkeypatch):
    results = run(monkeypatch, "_body_indexer_top_pods")
    for rank, top in results.items():
        assert top == [[("pod-z", 6.0), ("pod-a", 6.0)],
                       [("pod-z", 1.0), ("pod-a", 1.0)], []], f"rank {rank}"
