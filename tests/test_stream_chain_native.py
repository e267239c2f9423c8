"""Host twin of the stream chain kernels (tokens_to_chunk_hashes_stream:
the begin / group / end FNV pieces and the segmented SHA-256 driver, at
any block size) against the pure-Python chain, every comparison exact."""

import random

import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402
from llmd_kvcache_amd.utils import hashing  # noqa: E402
from tests.sha_chain_cases import SHA_ALGOS, golden_chain  # noqa: E402
from tests.test_device_read_path_gpu import SPECIAL  # noqa: E402

pytestmark = pytest.mark.skipif(
    cpu_ext.maybe_load() is None, reason="native extension not built"
)

# a tail only; whole groups with and without a tail; the 1 -> 2 and 2 -> 3
# byte array headers; the edges of the 64-token SHA segment
BLOCK_SIZES = [1, 15, 16, 17, 23, 24, 63, 64, 65, 131, 255, 256]
# every CBOR width of a token, and the 32-bit narrowing edges
VALUES = [0, 23, 24, 255, 256, 65535, 65536] + [
    t & 0xFFFFFFFF for t in SPECIAL]


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("algo", sorted(hashing.NATIVE_ALGO_IDS))
def test_stream_chain_matches_python_chain(algo, bs):
    """Three chunks: link 1 under a parent of every width, links 2 and 3
    under a 64-bit hash."""
    ops = cpu_ext.require()
    rng = random.Random(bs)
    tokens = [VALUES[rng.randrange(len(VALUES))] for _ in range(3 * bs)]
    tokens += tokens[:bs // 2]  # a remainder below a chunk is dropped
    for parent in (hashing.CHAIN_ALGOS[algo][1]("seed"), 0, 24, 65535,
                   2**32 - 1, 2**32):
        want = golden_chain(algo, parent, tokens, bs)
        assert len(want) == 3
        got = ops.tokens_to_chunk_hashes_stream(
            tokens, parent, bs, hashing.NATIVE_ALGO_IDS[algo])
        assert got == want, parent


@pytest.mark.parametrize("bs", [42, 43, 50, 51])
@pytest.mark.parametrize("algo", SHA_ALGOS)
def test_stream_sha_padding_edges(algo, bs):
    """One-byte tokens under a 64-bit parent: a payload of bs + 13 bytes,
    55, 56, 63 and 64 mod 64."""
    ops = cpu_ext.require()
    tokens = [(7 * i) % 24 for i in range(3 * bs)]
    parent = 2**64 - 1
    assert len(hashing.cbor_chunk_payload(parent, tokens[:bs])) == bs + 13
    assert ops.tokens_to_chunk_hashes_stream(
        tokens, parent, bs, hashing.NATIVE_ALGO_IDS[algo]) == golden_chain(
            algo, parent, tokens, bs)


def test_stream_chain_block_size_range():
    ops = cpu_ext.require()
    for bs in (0, 65536):
        with pytest.raises(RuntimeError):
            ops.tokens_to_chunk_hashes_stream([1] * 8, 0, bs, 0)
