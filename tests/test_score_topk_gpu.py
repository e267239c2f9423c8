"""Score top-n on MI355X, exactly, against the contract written in numpy
over the CPU table's score matrix of the same content: a GpuIndex and a
NativeIndex fed the same add() calls, 8 prompts of K keys (HOLD in _world),
tier weights 1.0 / 0.5 (exact in binary: the contract alone decides ties).
Every case runs unfiltered and with a filter that drops the best pods."""

import functools
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.indexer import Config, Indexer  # noqa: E402
from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex,
    GpuIndexConfig,
    NativeIndex,
    TableIndexConfig,
    _to_i64,
)
from llmd_kvcache_amd.kvblock.keys import Key, PodEntry  # noqa: E402
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    TokenProcessorConfig,
)
from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402
from llmd_kvcache_amd.scorer import KVCacheBackendConfig  # noqa: E402

from .score_topk_cases import expected_topk, tie_matrix  # noqa: E402

B = 8
WEIGHTS = [1.0, 0.5, 1.0, 1.0]
TIERS = ["gpu", "cpu"]
EPOCH = 1_000_000


def _pair():
    kw = dict(capacity=1 << 12, pods_per_key=24)
    return GpuIndex(GpuIndexConfig(**kw)), NativeIndex(TableIndexConfig(**kw))


@functools.lru_cache(maxsize=None)
def _world(num_pods, K, n_tiers):
    """-> gpu index, flat hashes, counts, {filtered: (words, reference)}."""
    rng = random.Random(num_pods * 1000 + K * 10 + n_tiers)
    gpu, cpu = _pair()
    for idx in (gpu, cpu):
        assert idx.registry.model_id("m") == 0
        for p in range(num_pods):
            assert idx.registry.pod_id(f"p{p:04d}") == p
    W = (num_pods + 63) // 64
    last = n_tiers - 1
    spread = sorted({p % num_pods for p in (0, 64, 65, 200)})
    hi = ((W - 1) // 4) * 4 * 64 + 5          # a word of wave 0
    lo = 70 if W > 1 else 3                   # wave 1 (W > 1), lower id
    many = sorted({(i * 53) % num_pods for i in range(20)})
    HOLD = [  # (pod, tier, leading keys held) per prompt
        [],                                        # no hit
        [(num_pods - 1, 0, K), (3, last, K)],      # fewer than top_n
        [(p, 0, K) for p in spread],               # ties across waves
        [(hi, 0, K), (lo, last, max(1, K // 2))],  # high id wins from wave 0
        [(p, i % n_tiers, 1 + (i * 7) % K) for i, p in enumerate(many)],
        [(w * 64 + w, 0, K) for w in range(W)],    # a pod in every word
        [(p, 0, 1) for p in spread],               # the one-key prompt
        [(hi, last, K), (lo, 0, K)],
    ]
    prompts = [[rng.randrange(1, 2**64) for _ in range(1 if b == 6 else K)]
               for b in range(B)]
    for keys, hold in zip(prompts, HOLD):
        ks = [Key("m", h) for h in keys]
        for pod, tier, depth in hold:
            for idx in (gpu, cpu):
                idx.add(ks[:depth], ks[:depth],
                        [PodEntry(f"p{pod:04d}", TIERS[tier])])
    flat = torch.tensor([_to_i64(h) for p in prompts for h in p],
                        dtype=torch.int64)
    counts = torch.tensor([len(p) for p in prompts], dtype=torch.int32)
    allow = [(1 << 64) - 1] * W
    for p in (hi, spread[0], num_pods - 1):   # the best pods of 1, 2, 3
        allow[p // 64] &= ~(1 << (p % 64))
    refs = {}
    for filtered in (False, True):
        words = [_to_i64(a) for a in allow] if filtered else []
        refs[filtered] = (words, cpu.table.ops.cpu_fused_score(
            *cpu.table._t(), flat, counts, 0,
            torch.tensor(words, dtype=torch.int64),
            torch.tensor(WEIGHTS), num_pods, EPOCH).numpy())
    assert (refs[False][1] > 0).sum(axis=1).tolist()[:5] == [
        0, 2, len(spread), 2, len(many)]
    return gpu, flat, counts, refs


def _dev_args(flat, counts, words):
    offsets = torch.zeros(B + 1, dtype=torch.int32)
    offsets[1:] = torch.cumsum(counts, 0)
    return (flat.cuda(), offsets.cuda(), 0,
            torch.tensor(words, dtype=torch.int64, device="cuda"),
            torch.tensor(WEIGHTS, device="cuda"))


def _check(got, matrix, top_n):
    ids, scores = got
    want_ids, want_scores = expected_topk(matrix, top_n)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(scores.cpu().numpy(), want_scores)


@pytest.mark.parametrize("top_n", [1, 3, 16])
@pytest.mark.parametrize("n_tiers", [1, 2])
@pytest.mark.parametrize("K", [1, 40])
@pytest.mark.parametrize("num_pods", [64, 320, 1024])
def test_fused_topk(num_pods, K, n_tiers, top_n):
    gpu, flat, counts, refs = _world(num_pods, K, n_tiers)
    for words, matrix in refs.values():
        got = gpu.table.ops.gpu_fused_topk(
            *gpu.table._t(), *_dev_args(flat, counts, words), num_pods, EPOCH,
            K, n_tiers, top_n)
        _check(got, matrix, top_n)


@pytest.mark.parametrize("top_n", [1, 3, 16])
def test_fused_topk_rows(top_n):
    """Padded rows, junk behind each row's keys, prompt 2 with n_keys 0."""
    num_pods, K, n_tiers = 320, 40, 2
    gpu, flat, counts, refs = _world(num_pods, K, n_tiers)
    rows = torch.nn.functional.pad(torch.nn.utils.rnn.pad_sequence(
        flat.split(counts.tolist()), batch_first=True, padding_value=0x5EED),
        (0, 3), value=0x5EED)
    n_keys = counts.clone()
    n_keys[2] = 0
    for words, matrix in refs.values():
        matrix = matrix.copy()
        matrix[2] = 0
        _, _, _, filt, weights = _dev_args(flat, counts, words)
        got = gpu.table.ops.gpu_fused_topk_rows(
            *gpu.table._t(), rows.cuda(), n_keys.cuda(), 0, filt, weights,
            num_pods, EPOCH, K, n_tiers, top_n)
        _check(got, matrix, top_n)


@pytest.mark.parametrize("top_n", [1, 16])
@pytest.mark.parametrize("P", [1, 64, 65, 257, 1088, 4096])
def test_topk_rows(P, top_n):
    m = tie_matrix(P, seed=P)
    got = cpu_ext.require().gpu_topk_rows(torch.from_numpy(m).cuda(), top_n)
    _check(got, m, top_n)


@pytest.mark.parametrize("top_n", [3, 16])
def test_topk_hashes_split_route(top_n):
    num_pods, K, n_tiers = 1088, 40, 2  # 17 words: past the fused kernel
    gpu, flat, counts, refs = _world(num_pods, K, n_tiers)
    for words, matrix in refs.values():
        got = gpu.table.ops.gpu_topk_hashes(
            *gpu.table._t(), *_dev_args(flat, counts, words), num_pods, EPOCH,
            K, n_tiers, top_n)
        _check(got, matrix, top_n)


def test_topk_flat_tokens():
    gpu, cpu = _pair()
    cfg = dict(token_processor=TokenProcessorConfig(block_size=16),
               backend_configs=[KVCacheBackendConfig("gpu", 1.0),
                                KVCacheBackendConfig("cpu", 0.5)])
    ix_gpu = Indexer(Config(device_chain="on", **cfg), kv_block_index=gpu)
    ix_cpu = Indexer(Config(**cfg), kv_block_index=cpu)
    rng = random.Random(7)
    lens = [7, 83, 160, 16, 0, 48, 331, 96]  # 7: shorter than one block
    prompts = [[rng.randrange(1, 50_000) for _ in range(n)] for n in lens]
    for idx in (gpu, cpu):
        for p in range(70):
            idx.registry.pod_id(f"p{p:04d}")
    for i, toks in enumerate(prompts):
        keys = ix_cpu.tokens_processor.tokens_to_kv_block_keys(None, toks, "m")
        for j, depth in enumerate(range(len(keys), 0, -2)):
            pod = PodEntry(f"p{(i * 9 + j * 23) % 70:04d}", TIERS[j % 2])
            for idx in (gpu, cpu):
                idx.add(keys[:depth], keys[:depth], [pod])
    flat = torch.tensor([t for p in prompts for t in p], dtype=torch.int64)
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens), 0)
    matrix = ix_cpu.score_flat_tokens(flat, off, "m", []).numpy()
    assert (matrix > 0).sum(axis=1).tolist()[:3] == [0, 3, 5]
    for top_n in (1, 4):
        got = ix_gpu.top_pods_flat_tokens(flat, off, "m", [], top_n)
        _check(got, matrix, top_n)
