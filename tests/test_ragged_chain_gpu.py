"""The ragged device chain on MI355X, every comparison exact:

 - gpu_hash_chain_ragged against hash_chain_batch on the same flat tokens,
   hashes and offsets both (CSR on both sides, so a store past a prompt's
   own chunks lands in its neighbour's and shows);
 - Indexer.score_flat_tokens / top_pods_flat_tokens under
   device_chain_layout "ragged" and "over_cap" against the CPU-chain route;
 - wire_score_flat with device_chain=2 against device_chain=0;
 - batches without a whole chunk.
"""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.indexer import plan_read_route  # noqa: E402
from llmd_kvcache_amd.kvblock.gpu_index import _to_i64  # noqa: E402
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    TokenProcessorConfig,
)
from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402
from llmd_kvcache_amd.utils import hashing  # noqa: E402

from .test_device_read_path_gpu import SPECIAL, _world  # noqa: E402

# whole chunks at the edges of the 16-chunk flush, odd counts among them so
# that CSR rows start at even and at odd slots
CHUNKS = [0, 1, 15, 16, 17, 31, 32, 33]
# token counts at the edges of the 64-position staging tile
TOKENS = [63, 64, 65, 127, 128, 129]
LONG = 1203  # 300 chunks at block size 4: waves of different trip counts


def _ragged(B, bs):
    """-> flat int64 tokens, int64 offsets [B+1] (numpy).  B == 1 is one
    prompt of 33 chunks and a remainder; otherwise the lengths cycle through
    CHUNKS (plus a remainder below a chunk) and TOKENS, the first and last
    prompts are empty and prompt 5 is LONG tokens."""
    lens = [CHUNKS[i % 14] * bs + i % 3 if i % 14 < 8 else TOKENS[i % 14 - 8]
            for i in range(B)]
    if B == 1:
        lens = [33 * bs + 1]
    else:
        lens[0] = lens[-1] = 0
    if B > 5:
        lens[5] = LONG
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    rng = np.random.default_rng(B * 100 + bs)
    flat = rng.integers(-2**63, 2**63 - 1, size=int(off[-1]), dtype=np.int64)
    for i in range(0, flat.size, 5):
        flat[i] = SPECIAL[(i // 5) % len(SPECIAL)]
    return flat, off


@functools.lru_cache(maxsize=None)
def _case(algo, bs, B):
    """-> tokens, offsets, init, and hash_chain_batch's (hashes, offsets)."""
    flat, off = _ragged(B, bs)
    tok, off_t = torch.from_numpy(flat), torch.from_numpy(off)
    init = _to_i64(TokenProcessorConfig(hash_algo=algo).init_hash())
    want = cpu_ext.require().hash_chain_batch(
        tok, off_t, torch.full((B,), init, dtype=torch.int64), bs,
        hashing.NATIVE_ALGO_IDS[algo])
    return tok, off_t, init, want


CHAIN_CASES = [("fnv-64a", 4), ("fnv-64a", 16), ("fnv-64a", 64)] + [
    (a, 16) for a in sorted(hashing.NATIVE_ALGO_IDS) if a != "fnv-64a"]


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("src", ["host_i64", "dev_i64", "dev_i32"])
@pytest.mark.parametrize("algo,bs", CHAIN_CASES)
def test_ragged_chain_matches_cpu_chain(algo, bs, src, B):
    tok, off_t, init, (want, want_off) = _case(algo, bs, B)
    if src == "dev_i64":
        tok = tok.cuda()
    elif src == "dev_i32":
        low = (tok.numpy() & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        tok = torch.from_numpy(low).cuda()
    got, h_off = cpu_ext.require().gpu_hash_chain_ragged(
        tok, off_t, init, bs, hashing.NATIVE_ALGO_IDS[algo])
    assert got.is_cuda and got.dtype == torch.int64
    assert h_off.is_cuda and h_off.dtype == torch.int32
    assert torch.equal(h_off.cpu(), want_off.to(torch.int32))
    assert torch.equal(got.cpu(), want)
    assert want.numel() >= 33


def _pair(ixs, flat, off, pods, top_n):
    if top_n is None:
        return [(ixs[m].score_flat_tokens(flat, off, "m", pods),)
                for m in ("on", "off")]
    return [ixs[m].top_pods_flat_tokens(flat, off, "m", pods, top_n)
            for m in ("on", "off")]


# the second world is one the resident score kernel refuses (1100 chunks x
# 4 tiers x 5 pod words of masks): the tiled chooser, from CSR input
WORLDS = [{}, dict(bs=4, n_pods=260, tiers=["gpu", "cpu", "disk", "remote"],
                   lens=[0, 4400, 13, 4 * 200, 0])]


@pytest.mark.parametrize("world", WORLDS, ids=["resident", "tiled"])
@pytest.mark.parametrize("layout,cap", [("ragged", 1 << 30),
                                        ("over_cap", 1024)])
def test_indexer_ragged_routes_equal_cpu_chain(layout, cap, world):
    gpu, spy, ixs, flat, off = _world(device_chain_layout=layout,
                                      device_chain_max_image_bytes=cap,
                                      **world)
    tp = ixs["on"].tokens_processor
    route = plan_read_route(off, tp.block_size, "fnv-64a", True,
                            ixs["on"].config)
    assert route.device and route.ragged
    for pods in ([], ["pod-0", "pod-3"]):
        for top_n in (None, 3):
            got, want = _pair(ixs, flat, off, pods, top_n)
            for g, w in zip(got, want):
                assert g.is_cuda and torch.equal(g, w)
            assert pods or want[-1].abs().sum().item() > 0
    assert spy.device_calls == 0  # never the padded op


@pytest.mark.parametrize("algo", sorted(hashing.NATIVE_ALGO_IDS))
def test_wire_score_flat_ragged_chain(algo):
    gpu, spy, ixs, flat, off = _world(algo=algo)
    tp = ixs["on"].tokens_processor
    P = gpu._num_pods_padded()
    args = (flat, off, gpu.registry.model_id("m"),
            gpu._filter_tensor({"pod-1", "pod-4"}, P), gpu.tier_weights(), P)
    tail = (_to_i64(tp.config.init_hash()), 16,
            len(gpu.registry.id_to_tier), hashing.NATIVE_ALGO_IDS[algo])
    ops = gpu.table.ops
    want, got = (ops.wire_score_flat(*gpu.table._t(), *args,
                                     gpu.table.next_epoch(), *tail,
                                     device_chain=d) for d in (0, 2))
    assert not got.is_cuda and want.abs().sum().item() > 0
    assert torch.equal(got, want)


@pytest.mark.parametrize("toks,offs", [(0, [0]), (20, [0, 0, 15, 20, 20])])
def test_ragged_empty_batches(toks, offs):
    gpu, spy, ixs, _, _ = _world(device_chain_layout="ragged")
    B, P = len(offs) - 1, gpu._num_pods_padded()
    tok = torch.arange(toks, dtype=torch.int64)
    off = torch.tensor(offs, dtype=torch.int64)
    ops = gpu.table.ops
    hashes, h_off = ops.gpu_hash_chain_ragged(tok, off, 0, 16, 0)
    assert hashes.is_cuda and tuple(hashes.shape) == (0,)
    assert h_off.is_cuda and h_off.cpu().tolist() == [0] * (B + 1)
    args = (*gpu.table._t(), tok, off, 0, gpu._filter_tensor(set(), P),
            gpu.tier_weights(), P, gpu.table.next_epoch(), 0, 16, 2, 0)
    s = ops.gpu_score_flat_tokens_ragged(*args)
    assert s.is_cuda and tuple(s.shape) == (B, P)
    assert s.abs().sum().item() == 0
    ids, top = ops.gpu_topk_flat_tokens_ragged(*args, 2)
    assert tuple(ids.shape) == tuple(top.shape) == (B, 2)
    assert (ids == -1).all().item() and top.abs().sum().item() == 0
    s = ixs["on"].score_flat_tokens(tok, off, "m", [])
    assert tuple(s.shape) == (B, P) and s.abs().sum().item() == 0
