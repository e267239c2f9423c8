"""gpu_tiled_topk[_rows] on MI355X against cpu_score_topk over
cpu_fused_score, ids and scores, in the worlds of test_tiled_score_gpu; a
world of ties across words and waves and of fewer scoring pods than top_n;
and the choosers: TableIndex.fused_scores / fused_top_pods at 1088 pods and
Indexer.score_flat_tokens (device chain) past 64 KB of masks, against a CPU
table of the same content."""

import functools
import random

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.indexer import Config, Indexer  # noqa: E402
from llmd_kvcache_amd.kvblock import gpu_index as gi  # noqa: E402
from llmd_kvcache_amd.kvblock.keys import Key, PodEntry  # noqa: E402
from llmd_kvcache_amd.kvblock.token_processor import TokenProcessorConfig  # noqa: E402,E501

from .test_tiled_score_gpu import MODEL, SHAPES, WEIGHTS, _batch, _build, _cpu_copy  # noqa: E402,E501

TIERS = ["gpu", "cpu", "disk", "remote"]


@functools.lru_cache(maxsize=None)
def _matrices(num_pods, n_tiers, ppk):
    """cpu_fused_score of the world's batch, without and with the filter."""
    table, KT, prompts, content, pad = _build(num_pods, n_tiers, ppk)
    flat, offsets, counts, rows, filters = _batch(num_pods, prompts, pad)
    return [table.ops.cpu_fused_score(*_cpu_copy(table), flat, counts, MODEL,
                                      f, torch.tensor(WEIGHTS), num_pods, 1)
            for f in filters]


@pytest.mark.parametrize("top_n", [1, 4, 16])
@pytest.mark.parametrize("num_pods,n_tiers,ppk", SHAPES)
def test_tiled_topk_matches_cpu(num_pods, n_tiers, ppk, top_n):
    table, KT, prompts, content, pad = _build(num_pods, n_tiers, ppk)
    ops = table.ops
    flat, offsets, counts, rows, filters = _batch(num_pods, prompts, pad)
    for filt, matrix in zip(filters, _matrices(num_pods, n_tiers, ppk)):
        want = ops.cpu_score_topk(matrix, top_n)
        tail = (MODEL, filt.cuda(), torch.tensor(WEIGHTS).cuda(), num_pods,
                table.next_epoch(), 3 * KT, n_tiers, top_n)
        for got in (ops.gpu_tiled_topk(*table._t(), flat.cuda(),
                                       offsets.cuda(), *tail),
                    ops.gpu_tiled_topk_rows(*table._t(), rows.cuda(),
                                            counts.cuda(), *tail)):
            assert torch.equal(got[0].cpu(), want[0])
            assert torch.equal(got[1].cpu(), want[1])


def _pair(num_pods, **kw):
    kw = dict(capacity=1 << 13, pods_per_key=24, **kw)
    pair = (gi.GpuIndex(gi.GpuIndexConfig(**kw)),
            gi.NativeIndex(gi.TableIndexConfig(**kw)))
    for idx in pair:
        for p in range(num_pods):
            assert idx.registry.pod_id(f"p{p:04d}") == p
    return pair


@pytest.mark.parametrize("top_n", [1, 4, 16])
def test_tiled_topk_ties_and_short_tail_through_the_choosers(top_n):
    """Prompt 0: 20 pods tied on one score, in all 17 words and so in all
    four waves; prompt 1: two pods.  1088 pods: the resident kernel
    refuses."""
    num_pods, K = 1088, 70
    gpu, cpu = _pair(num_pods)
    rng = random.Random(5)
    tied = sorted((i % 17) * 64 + (i * 7 + 3) % 64 for i in range(20))
    assert len(set(tied)) == 20 and len({p // 64 for p in tied}) == 17
    prompts = [[rng.randrange(1, 2**64) for _ in range(K)] for _ in range(2)]
    for keys, pods in zip(prompts, (tied, [1000, 70])):
        ks = [Key("m", h) for h in keys]
        for idx in (gpu, cpu):
            idx.add(ks, ks, [PodEntry(f"p{p:04d}", "gpu") for p in pods])
    flat = torch.tensor([gi._to_i64(h) for p in prompts for h in p])
    counts = torch.tensor([K, K], dtype=torch.int32)
    offsets = torch.tensor([0, K, 2 * K], dtype=torch.int32).cuda()
    matrix = cpu.fused_scores(flat, counts, "m", set())
    assert torch.equal(
        gpu.fused_scores(flat.cuda(), offsets, "m", set(), max_k=K).cpu(),
        matrix)
    ids, top = (t.cpu() for t in gpu.fused_top_pods(
        flat.cuda(), offsets, "m", set(), max_k=K, top_n=top_n))
    want = cpu.fused_top_pods(flat, counts, "m", set(), top_n=top_n)
    assert torch.equal(ids, want[0]) and torch.equal(top, want[1])
    assert ids[0].tolist() == tied[:top_n]  # equal scores: ascending id
    assert top[0].tolist() == [float(K)] * top_n
    assert ids[1].tolist() == ([70, 1000] + [-1] * 16)[:top_n]
    assert top[1].tolist() == ([float(K)] * 2 + [0.0] * 16)[:top_n]


def test_score_flat_tokens_past_the_lds_ceiling():
    """1100 chunks x 4 tiers x 5 pod words x 8 B > 64 KB of masks."""
    gpu, cpu = _pair(260, tier_names=list(TIERS))
    tp = TokenProcessorConfig(block_size=4)
    ix_gpu = Indexer(Config(token_processor=tp, device_chain="on"),
                     kv_block_index=gpu)
    ix_cpu = Indexer(Config(token_processor=tp), kv_block_index=cpu)
    rng = random.Random(11)
    lens = [0, 4400, 13, 800, 0]
    prompts = [[rng.randrange(1, 1 << 31) for _ in range(n)] for n in lens]
    for i, toks in enumerate(prompts):
        keys = ix_cpu.tokens_processor.tokens_to_kv_block_keys(None, toks, "m")
        for j in range(3 if keys else 0):  # prefixes of different depth
            depth = max(1, len(keys) * (j + 1) // 3)
            pod = PodEntry(f"p{(i * 3 + j * 5) * 43 % 260:04d}",
                           TIERS[(i + j) % 4])
            for idx in (gpu, cpu):
                idx.add(keys[:depth], keys[:depth], [pod])
    flat = torch.tensor([t for p in prompts for t in p], dtype=torch.int64)
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens), 0)
    want = ix_cpu.score_flat_tokens(flat, off, "m", [])
    assert (want > 0).sum(dim=1).tolist() == [0, 3, 3, 3, 0]
    assert torch.equal(ix_gpu.score_flat_tokens(flat, off, "m", []).cpu(),
                       want)
    got = ix_gpu.top_pods_flat_tokens(flat, off, "m", [], 4)
    want = cpu.table.ops.cpu_score_topk(want, 4)
    assert torch.equal(got[0].cpu(), want[0])
    assert torch.equal(got[1].cpu(), want[1])
