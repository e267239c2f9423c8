"""The stream chain kernels on MI355X (the ragged device chain at block
sizes outside 4/8/16/32/64), every comparison exact:

 - gpu_hash_chain_ragged against hash_chain_batch, hashes and offsets;
 - Indexer.score_flat_tokens / top_pods_flat_tokens at block size 24 under
   device_chain_block_sizes "any" against the CPU-chain route, and the
   default "fixed" staying on the CPU chain.
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

# whole chunks at the edges of the 16-chunk flush, rows at even and odd slots
CHUNKS = [0, 1, 15, 16, 17, 33]


@functools.lru_cache(maxsize=None)
def _case(algo, bs, B):
    """-> int64 tokens, offsets, init, hash_chain_batch's (hashes, offsets).
    Prompt i has CHUNKS[i % 6] chunks and a remainder below a chunk (B == 1:
    33 chunks).  Prompts 0, 3, .. hold one-byte tokens only, 1, 4, ..
    five-byte tokens only - neighbours in a wave, so their SHA block counts
    per segment differ - and 2, 5, .. any int64, SPECIAL among them."""
    lens = [CHUNKS[(i + 5 * (B == 1)) % 6] * bs + i % 3 % bs for i in range(B)]
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    rng = np.random.default_rng(B * 1000 + bs)
    flat = rng.integers(-2**63, 2**63 - 1, size=int(off[-1]), dtype=np.int64)
    flat[::5] = np.resize(SPECIAL, flat[::5].size)
    for i in range(B):
        row = flat[off[i]:off[i + 1]]
        if i % 3 == 0:
            row[:] = rng.integers(0, 24, size=row.size)
        elif i % 3 == 1:
            row[:] = rng.integers(65536, 2**32, size=row.size)
    tok, off_t = torch.from_numpy(flat), torch.from_numpy(off)
    init = _to_i64(TokenProcessorConfig(hash_algo=algo).init_hash())
    want = cpu_ext.require().hash_chain_batch(
        tok, off_t, torch.full((B,), init, dtype=torch.int64), bs,
        hashing.NATIVE_ALGO_IDS[algo])
    return tok, off_t, init, want


CASES = [("fnv-64a", bs) for bs in (1, 24, 100, 256)] + [
    (a, bs) for a in ("sha256-cbor-64", "sha256-cbor-64-low")
    for bs in (24, 65, 256)]


@pytest.mark.parametrize("B", [1, 64, 65])
@pytest.mark.parametrize("src", ["host_i64", "dev_i32"])
@pytest.mark.parametrize("algo,bs", CASES)
def test_stream_chain_matches_cpu_chain(algo, bs, src, B):
    tok, off_t, init, (want, want_off) = _case(algo, bs, B)
    if src == "dev_i32":
        low = (tok.numpy() & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        tok = torch.from_numpy(low).cuda()
    got, h_off = cpu_ext.require().gpu_hash_chain_ragged(
        tok, off_t, init, bs, hashing.NATIVE_ALGO_IDS[algo])
    assert torch.equal(h_off.cpu(), want_off.to(torch.int32))
    assert torch.equal(got.cpu(), want)
    assert want.numel() >= 33


@pytest.mark.parametrize("sizes,device", [("any", True), ("fixed", False)])
def test_indexer_block_size_24(sizes, device):
    gpu, spy, ixs, flat, off = _world(bs=24, lens=[0, 24 * 5 + 3, 23, 24, 0],
                                      device_chain_block_sizes=sizes)
    route = plan_read_route(off, 24, "fnv-64a", True, ixs["on"].config)
    assert route.device == device and route.ragged == device
    want = ixs["off"].score_flat_tokens(flat, off, "m", [])
    assert torch.equal(ixs["on"].score_flat_tokens(flat, off, "m", []), want)
    assert want.cpu()[1].max().item() > 0
    for g, w in zip(ixs["on"].top_pods_flat_tokens(flat, off, "m", [], 3),
                    ixs["off"].top_pods_flat_tokens(flat, off, "m", [], 3)):
        assert torch.equal(g, w)
