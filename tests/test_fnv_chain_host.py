"""Host build of the FNV chain link the GPU read path runs
(chunk_hash_fast: paired high token bytes under one select, the
wide-parent item) against chunk_hash through hash_chain_batch and the
pure-Python golden, on every CBOR width boundary of tokens and parents.
tokens_to_chunk_hashes_fast is the op that reaches the helper: it takes
the wide-parent path for every parent above 0xFFFFFFFF and the generic
one below, which is what a wave of the kernel decides by vote."""

import itertools

import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402
from llmd_kvcache_amd.utils import hashing  # noqa: E402

pytestmark = pytest.mark.skipif(
    cpu_ext.maybe_load() is None, reason="native extension not built"
)

EDGE_TOKENS = [0, 23, 24, 255, 256, 65535, 65536, 2**31 - 1, 2**32 - 1]
EDGE_PARENTS = [0, 23, 24, 255, 256, 65535, 65536, 2**32 - 1, 2**32,
                2**64 - 1]


def _i64(h):
    return h - (1 << 64) if h >= (1 << 63) else h


def _u64(h):
    return h + (1 << 64) if h < 0 else h


def _golden(parent, tokens, bs):
    out, h = [], parent
    for c in range(len(tokens) // bs):
        h = hashing.chunk_hash(h, tokens[c * bs:(c + 1) * bs])
        out.append(h)
    return out


def _prompts(bs):
    """Every edge token at the first, a middle and the last position of a
    chunk, the other positions cycling through all the widths; two
    chunks, so the second link takes a full 64-bit parent."""
    out = []
    for e, pos in itertools.product(range(len(EDGE_TOKENS)),
                                    (0, bs // 2, bs - 1)):
        toks = [EDGE_TOKENS[(e + 2 * j + 1) % len(EDGE_TOKENS)]
                for j in range(2 * bs)]
        toks[pos] = EDGE_TOKENS[e]
        toks[bs + pos] = EDGE_TOKENS[e]
        out.append(toks)
    return out


@pytest.mark.parametrize("bs", [4, 16, 64])
def test_fast_link_matches_chunk_hash(bs):
    ops = cpu_ext.require()
    prompts = _prompts(bs)
    cases = list(itertools.product(EDGE_PARENTS, prompts))
    flat = torch.tensor([t for _, p in cases for t in p], dtype=torch.int64)
    off = torch.arange(0, (len(cases) + 1) * 2 * bs, 2 * bs,
                       dtype=torch.int64)
    parents = torch.tensor([_i64(p) for p, _ in cases], dtype=torch.int64)
    ref, chunk_off = ops.hash_chain_batch(flat, off, parents, bs, 0)
    ref = [_u64(h) for h in ref.tolist()]
    assert chunk_off.tolist() == list(range(0, 2 * len(cases) + 1, 2))
    for i, (parent, toks) in enumerate(cases):
        want = ref[2 * i:2 * i + 2]
        assert want == _golden(parent, toks, bs), (parent, i)
        got = ops.tokens_to_chunk_hashes_fast(toks, parent, bs, 0)
        assert list(got) == want, (parent, i)
