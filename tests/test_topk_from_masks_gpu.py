"""gpu_topk_from_masks on MI355X against cpu_topk_from_masks on the same
masks, bit for bit, and the CPU twin against the composition it stands
for (cpu_score_from_masks, then cpu_score_topk)."""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402

pytestmark = pytest.mark.gpu

WEIGHTS = [1.0, 0.8, 0.5, 0.3]


def build_masks(rng, num_pods, T, K, prefix):
    """int64 [K, T, W]: pod p is listed by keys 0..prefix[p]-1, under one
    random tier per key.  Every third pod is a copy of the pod before it
    (equal scores: the id decides); every bit past num_pods is set."""
    W = (num_pods + 63) // 64
    tier = rng.integers(0, T, size=(K, num_pods))
    twin = np.arange(2, num_pods, 3)
    tier[:, twin] = tier[:, twin - 1]
    prefix[twin] = prefix[twin - 1]
    present = np.arange(K)[:, None] < prefix[None, :]
    bits = np.ones((K, T, W * 64), dtype=bool)
    for t in range(T):
        bits[:, t, :num_pods] = present & (tier == t)
    words = np.packbits(bits.reshape(K, T, W, 64), axis=-1, bitorder="little")
    return words.view("<u8").reshape(K, T, W).view(np.int64)


@functools.lru_cache(maxsize=None)
def case(num_pods, T):
    """One batch per fleet shape, built once: masks, offsets, weights."""
    ops = cpu_ext.require()
    W = (num_pods + 63) // 64
    KT = int(ops.tiled_score_tile_keys(T, W))
    rng = np.random.default_rng(num_pods * 8 + T)
    long = 2 * KT + 1

    def some(K, *always):  # a few distinct prefix lengths, then `always`
        p = rng.choice(np.array([0, 1, K // 2, K]), size=num_pods)
        p[:len(always)] = always[:num_pods]
        return p

    prompts = [
        (long, some(long, long)),            # never breaks; both buffers
        (1, some(1)),                        # starts at an odd key offset
        (0, some(0)),                        # no keys: offsets repeat
        (KT - 1, some(KT - 1)),
        (KT, some(KT, KT)),
        (KT + 1, np.minimum(some(KT + 1, KT), KT)),  # last pod drops at KT
        (long, np.zeros(num_pods, dtype=np.int64)),  # nobody at key 0
        (long, np.minimum(some(long, KT + 2), KT + 2)),  # exit in tile 2
    ]
    masks = np.concatenate(
        [build_masks(rng, num_pods, T, K, p) for K, p in prompts])
    offsets = np.cumsum([0] + [K for K, _ in prompts]).astype(np.int32)
    return (torch.from_numpy(masks), torch.from_numpy(offsets),
            torch.tensor(WEIGHTS[:T], dtype=torch.float32))


@pytest.mark.parametrize("top_n", [1, 16])
@pytest.mark.parametrize("num_pods,T", [(1, 1), (64, 1), (70, 2), (320, 1),
                                        (1100, 4), (4096, 4)])
def test_gpu_topk_from_masks_is_the_cpu_twin(num_pods, T, top_n):
    ops = cpu_ext.require()
    masks, offsets, weights = case(num_pods, T)
    want_ids, want_top = ops.cpu_topk_from_masks(masks, offsets, weights,
                                                 num_pods, top_n)
    comp_ids, comp_top = ops.cpu_score_topk(
        ops.cpu_score_from_masks(masks, offsets, weights, num_pods), top_n)
    assert torch.equal(want_ids, comp_ids)
    assert torch.equal(want_top.view(torch.int32), comp_top.view(torch.int32))
    assert (want_ids < num_pods).all()  # the bits past num_pods never score
    assert (want_ids[2] == -1).all() and (want_ids[6] == -1).all()
    assert want_ids[0, 0] >= 0

    ids, top = ops.gpu_topk_from_masks(masks.cuda(), offsets.cuda(),
                                       weights.cuda(), num_pods, top_n)
    assert torch.equal(ids.cpu(), want_ids)
    assert torch.equal(top.cpu().view(torch.int32),
                       want_top.view(torch.int32))
