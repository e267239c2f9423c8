"""Row-major output of the fnv-64a chain kernel, which stages 16 chunks
per prompt in LDS and writes them as whole 128-byte lines: at block size
16 every batch size around the 64-lane wave and the 8-prompt store group,
every chunk count around the 16-chunk flush (below it, exactly on it, one
past it, two flushes and a tail; odd counts take the 8-byte store path,
even ones the 16-byte one), against the transposed output and the
pure-Python golden chain.  Block sizes 4 and 64 run the same kernel
template and take the same chunk counts at one two-wave batch."""

import random

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.utils import hashing  # noqa: E402
from tests.sha_chain_cases import golden_chain  # noqa: E402

FNV = "fnv-64a"
MAX_CHUNKS = [1, 15, 16, 17, 33]
JUNK = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def ops():
    from llmd_kvcache_amd.ops import cpu_ext

    mod = cpu_ext.require()
    assert mod.HAS_HIP
    return mod


def _i64(h):
    return h - (1 << 64) if h >= (1 << 63) else h


def _run(ops, tt, par, nch, bs, max_chunks, row_major):
    """The op, called right after the caching allocator got back a block
    of the output's size full of non-zero bytes."""
    B = par.numel()
    junk = torch.full((B * max_chunks,), JUNK, dtype=torch.int64,
                      device="cuda")
    torch.cuda.synchronize()
    del junk
    return ops.gpu_hash_chain_tr(tt, par, nch, bs, max_chunks, 0, row_major,
                                 hashing.NATIVE_ALGO_IDS[FNV])


def _check_row_major(ops, bs, B, max_chunks):
    import numpy as np

    rng = random.Random(1000 * B + max_chunks)
    toks = np.array(
        [[rng.randrange(2**32) >> rng.choice((0, 8, 16, 24, 28))
          for _ in range(max_chunks * bs)] for _ in range(B)],
        dtype=np.uint32)
    parents = [rng.randrange(2**32, 2**64) for _ in range(B)]
    parents[B // 2] = 24  # <= 0xFFFFFFFF: its wave runs the generic parent body
    tt = torch.from_numpy(np.ascontiguousarray(toks.T).view(np.int32)).cuda()
    par = torch.tensor([_i64(p) for p in parents], dtype=torch.int64,
                       device="cuda")
    # one golden chain per prompt at full length; shorter prompts are
    # its prefixes
    want = torch.tensor(
        [[_i64(h) for h in golden_chain(FNV, parents[b], toks[b].tolist(), bs)]
         for b in range(B)], dtype=torch.int64)
    assert tuple(want.shape) == (B, max_chunks)

    mixed = [rng.randrange(max_chunks + 1) for _ in range(B)]
    mixed[0] = max_chunks
    mixed[-1] = 0 if B > 1 else max_chunks
    for n_chunks in (mixed, [0] * B, [max_chunks] * B):
        nch = torch.tensor(n_chunks, dtype=torch.int32, device="cuda")
        row = _run(ops, tt, par, nch, bs, max_chunks, 1).cpu()
        tr = _run(ops, tt, par, nch, bs, max_chunks, 0).cpu()
        assert tuple(row.shape) == (B, max_chunks)
        assert tuple(tr.shape) == (max_chunks, B)
        assert torch.equal(row, tr.t())
        keep = (torch.arange(max_chunks)[None, :] <
                torch.tensor(n_chunks)[:, None])
        assert torch.equal(row, torch.where(keep, want, 0))


@pytest.mark.parametrize("max_chunks", MAX_CHUNKS)
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_row_major_equals_transposed_and_golden(ops, B, max_chunks):
    _check_row_major(ops, 16, B, max_chunks)


@pytest.mark.parametrize("max_chunks", MAX_CHUNKS)
@pytest.mark.parametrize("bs", [4, 64])
def test_row_major_other_block_sizes(ops, bs, max_chunks):
    _check_row_major(ops, bs, 65, max_chunks)
