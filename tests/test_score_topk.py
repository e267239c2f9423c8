"""Score top-n on the host: cpu_score_topk against the contract written in
numpy, Indexer.top_pods_tokens_batch on a table backend and on a generic
one, and the "top_k" field of POST /score_batch."""

import http.client
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.indexer import Config, Indexer  # noqa: E402
from llmd_kvcache_amd.kvblock import (  # noqa: E402
    InMemoryIndex,
    InMemoryIndexConfig,
)
from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    NativeIndex,
    TableIndexConfig,
)
from llmd_kvcache_amd.kvblock.keys import PodEntry  # noqa: E402
from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402
from llmd_kvcache_amd.scorer import KVCacheBackendConfig  # noqa: E402
from llmd_kvcache_amd.tokenization.pool import TokenizationPool  # noqa: E402

from . import test_services as svc  # noqa: E402
from .score_topk_cases import expected_topk, tie_matrix  # noqa: E402


@pytest.mark.parametrize("top_n", [1, 3, 16])
@pytest.mark.parametrize("P", [1, 64, 65, 4096])
def test_cpu_score_topk_is_the_contract(P, top_n):
    m = tie_matrix(P, seed=P)
    ids, scores = cpu_ext.require().cpu_score_topk(torch.from_numpy(m), top_n)
    want_ids, want_scores = expected_topk(m, top_n)
    assert np.array_equal(ids.numpy(), want_ids)
    assert np.array_equal(scores.numpy(), want_scores)


def _indexer(index):
    """Tier weights exact in binary; hold[i]: (pod, tier, leading blocks)."""
    cfg = Config(backend_configs=[KVCacheBackendConfig("gpu", 1.0),
                                  KVCacheBackendConfig("cpu", 0.5)])
    cfg.token_processor.block_size = 4
    pool = TokenizationPool(cfg.tokenizers_pool,
                            tokenizer=svc.FixedTokenizer())
    idx = Indexer(cfg, tokenization_pool=pool, kv_block_index=index)
    prompts = [f"{i}: top-n prompt, one of four " * 5 for i in range(4)]
    hold = [
        [("pod-a", "gpu", 8), ("pod-b", "cpu", 8), ("pod-c", "gpu", 8)],
        [("pod-d", "gpu", 2), ("pod-a", "cpu", 6), ("pod-b", "gpu", 3)],
        [("pod-b", "cpu", 1)],
        [],
    ]
    if hasattr(index, "registry"):  # table backend: ids in name order
        for name in "abcd":
            index.registry.pod_id(f"pod-{name}")
    token_lists = [svc.FixedTokenizer().encode(p, "m")[0] for p in prompts]
    for toks, pods in zip(token_lists, hold):
        keys = idx.tokens_processor.tokens_to_kv_block_keys(None, toks, "m")
        for pod, tier, depth in pods:
            index.add(keys[:depth], keys[:depth], [PodEntry(pod, tier)])
    return idx, prompts, token_lists


def _backends():
    return [NativeIndex(TableIndexConfig(capacity=1 << 10, pods_per_key=4)),
            InMemoryIndex(InMemoryIndexConfig(size=10_000, pod_cache_size=10))]


@pytest.mark.parametrize("top_n", [1, 2, 16])
@pytest.mark.parametrize("index", _backends(), ids=["native", "in_memory"])
def test_top_pods_tokens_batch_is_the_sorted_score_map(index, top_n):
    idx, _, token_lists = _indexer(index)
    maps = idx.score_tokens_batch(token_lists, "m", [])
    assert maps[0] == {"pod-a": 8.0, "pod-b": 4.0, "pod-c": 8.0}
    want = [sorted(m.items(), key=lambda ps: (-ps[1], ps[0]))[:top_n]
            for m in maps]
    got = idx.top_pods_tokens_batch(token_lists, "m", [], top_n)
    assert [[tuple(ps) for ps in row] for row in got] == want
    # the candidate filter applies before the pick
    got = idx.top_pods_tokens_batch(token_lists, "m", ["pod-b", "pod-c"], 1)
    assert [tuple(ps) for ps in got[0]] == [("pod-c", 8.0)]


def test_top_n_and_weights_are_checked():
    idx, _, token_lists = _indexer(_backends()[0])
    for bad in (0, 17, 2.0, True, None):
        with pytest.raises(ValueError):
            idx.top_pods_tokens_batch(token_lists, "m", [], bad)
    for w in (-1.0, float("nan")):
        idx.config.backend_configs[1].weight = w
        with pytest.raises(ValueError):
            idx.top_pods_tokens_batch(token_lists, "m", [], 2)
        idx.score_tokens_batch(token_lists, "m", [])  # accepted as before


def test_score_batch_top_k():
    from llmd_kvcache_amd.service.asgi import build_app
    from llmd_kvcache_amd.service.http_server import HttpService

    idx, prompts, token_lists = _indexer(_backends()[0])
    body = {"prompts": prompts, "model": "m"}
    top = [[["pod-a", 8.0], ["pod-c", 8.0]], [["pod-a", 3.0], ["pod-b", 3.0]],
           [["pod-b", 0.5]], []]
    app = build_app(idx)
    assert svc.TestAsgiApp.call(app, "POST", "/score_batch",
                                {**body, "top_k": 2}) == (200, {"top": top})
    # without the field: the answer it always gave
    assert svc.TestAsgiApp.call(app, "POST", "/score_batch", body) == (
        200, {"scores": idx.score_tokens_batch(token_lists, "m", [])})
    for bad in (0, 17, "3", 1.5, True, None):
        status, _ = svc.TestAsgiApp.call(app, "POST", "/score_batch",
                                         {**body, "top_k": bad})
        assert status == 400

    http_svc = HttpService(idx, host="127.0.0.1", port=0)
    http_svc.start()
    try:
        conn = http.client.HTTPConnection("127.0.0.1", http_svc.port,
                                          timeout=5)
        for top_k, want in ((2, (200, {"top": top})), (17, (400, None))):
            conn.request("POST", "/score_batch",
                         json.dumps({**body, "top_k": top_k}))
            r = conn.getresponse()
            raw = r.read()
            assert (r.status, json.loads(raw) if want[1] else None) == want
    finally:
        http_svc.stop()
