"""gpu_hash_chain_tr on MI355X against the pure-Python golden
(hashing.CHAIN_ALGOS): every token and parent CBOR width, the wave-voted
wide-parent path next to the generic one, and the "unused slots are 0"
contract now that the op hands the kernels uninitialised memory."""

import random

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.utils import hashing  # noqa: E402
from tests.sha_chain_cases import golden_chain  # noqa: E402

FNV = "fnv-64a"
SHA = "sha256-cbor-64"
EDGE_TOKENS = [0, 23, 24, 255, 256, 65535, 65536, 2**31 - 1, 2**32 - 1]
SMALL_PARENTS = [0, 23, 24, 255, 256, 65535, 65536, 2**32 - 1]
WIDE_PARENTS = [2**32, 2**64 - 1]
EDGE_PARENTS = SMALL_PARENTS + WIDE_PARENTS
WIDTH_SHIFTS = (0, 8, 16, 24, 28)  # token widths 5/5/3/2/1 bytes


@pytest.fixture(scope="module")
def ops():
    from llmd_kvcache_amd.ops import cpu_ext

    mod = cpu_ext.require()
    assert mod.HAS_HIP
    return mod


def _i64(h):
    return h - (1 << 64) if h >= (1 << 63) else h


def _u64(h):
    return h + (1 << 64) if h < 0 else h


def _tokens_t(prompts, rows):
    """[rows, B] int32 (uint32 bit pattern), zero padded."""
    import numpy as np

    t = np.zeros((rows, len(prompts)), dtype=np.uint32)
    for b, p in enumerate(prompts):
        t[:len(p), b] = p
    return torch.from_numpy(t.view(np.int32)).cuda()


def _rand_tokens(rng, n):
    return [rng.randrange(2**32) >> rng.choice(WIDTH_SHIFTS)
            for _ in range(n)]


def _wide(rng):
    return rng.randrange(2**32, 2**64)


def _check(ops, algo, prompts, parents, bs, max_chunks, ilp=0,
           row_major=0):
    """Runs the op twice, each time right after the caching allocator got
    back a buffer of the output's size full of non-zero bytes, and
    compares every slot: the golden chain, then exact zeros."""
    B = len(prompts)
    n_chunks = [len(p) // bs for p in prompts]
    assert max(n_chunks) <= max_chunks
    tt = _tokens_t(prompts, max_chunks * bs)
    par = torch.tensor([_i64(p) for p in parents], dtype=torch.int64,
                       device="cuda")
    nch = torch.tensor(n_chunks, dtype=torch.int32, device="cuda")
    want = [golden_chain(algo, parents[b], prompts[b], bs) for b in range(B)]
    for _ in range(2):
        junk = torch.full((B * max_chunks,), -0x5A5A5A5A5A5A5A5B,
                          dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        del junk
        out = ops.gpu_hash_chain_tr(tt, par, nch, bs, max_chunks, ilp,
                                    row_major,
                                    hashing.NATIVE_ALGO_IDS[algo]).cpu()
        assert tuple(out.shape) == ((B, max_chunks) if row_major
                                    else (max_chunks, B))
        for b in range(B):
            col = (out[b] if row_major else out[:, b]).tolist()
            n = len(want[b])
            assert [_u64(h) for h in col[:n]] == want[b], b
            assert col[n:] == [0] * (max_chunks - n), b
        del out


def test_token_width_boundaries(ops):
    """Every edge token at the first, a middle and the last position of a
    chunk; the other positions cycle through all widths with a per-lane
    phase, so neighbouring lanes differ in width at every position."""
    bs, prompts = 16, []
    for pos in (0, 7, 15):
        for e in range(len(EDGE_TOKENS)):
            toks = [EDGE_TOKENS[(e + 2 * j + 1) % len(EDGE_TOKENS)]
                    for j in range(2 * bs)]
            toks[pos] = EDGE_TOKENS[e]
            toks[bs + pos] = EDGE_TOKENS[(e + 4) % len(EDGE_TOKENS)]
            prompts.append(toks)
    rng = random.Random(5)
    parents = [_wide(rng) if b % 3 else EDGE_PARENTS[b % 10]
               for b in range(len(prompts))]
    for row_major in (0, 1):
        _check(ops, FNV, prompts, parents, bs, 2, row_major=row_major)


def test_parents_all_wide(ops):
    """Fast parent path already in chunk 0, in both waves."""
    rng = random.Random(6)
    B, bs = 70, 16
    prompts = [_rand_tokens(rng, 3 * bs) for _ in range(B)]
    parents = [WIDE_PARENTS[b % 2] if b % 4 == 0 else _wide(rng)
               for b in range(B)]
    _check(ops, FNV, prompts, parents, bs, 3)


@pytest.mark.parametrize("small", SMALL_PARENTS)
def test_one_small_parent_in_the_wave(ops, small):
    """Generic path in chunk 0 (one lane votes no), fast from chunk 1."""
    rng = random.Random(small % 1000)
    B, bs = 64, 16
    prompts = [_rand_tokens(rng, 3 * bs) for _ in range(B)]
    parents = [_wide(rng) for _ in range(B)]
    parents[37] = small
    _check(ops, FNV, prompts, parents, bs, 3)


def test_only_second_wave_mixed(ops):
    """130 lanes: waves 0 and 2 all wide, wave 1 cycles through every
    parent width - the vote is per wave."""
    rng = random.Random(8)
    B, bs = 130, 16
    prompts = [_rand_tokens(rng, 3 * bs) for _ in range(B)]
    parents = [EDGE_PARENTS[b % 10] if 64 <= b < 128 else _wide(rng)
               for b in range(B)]
    for row_major in (0, 1):
        _check(ops, FNV, prompts, parents, bs, 3, row_major=row_major)


def _ragged(rng, B, bs):
    """n_chunks from {0, 1, 3, 5} mixed within a wave; lanes 64..127 stop
    at 3 and lanes 128..191 have none, so whole waves finish early."""
    def n(b):
        if 128 <= b < 192:
            return 0
        k = (0, 1, 3, 5)[(b * 7 + b // 3) % 4]
        return min(k, 3) if 64 <= b < 128 else k

    prompts = [_rand_tokens(rng, n(b) * bs) for b in range(B)]
    parents = [EDGE_PARENTS[b % 10] if b % 6 == 0 else _wide(rng)
               for b in range(B)]
    return prompts, parents


@pytest.mark.parametrize("row_major", [0, 1])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_ragged_lengths_and_zero_slots(ops, B, row_major):
    prompts, parents = _ragged(random.Random(B), B, 16)
    _check(ops, FNV, prompts, parents, 16, 5, row_major=row_major)


@pytest.mark.parametrize("row_major", [0, 1])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_ragged_lengths_and_zero_slots_sha(ops, B, row_major):
    prompts, parents = _ragged(random.Random(B), B, 16)
    _check(ops, SHA, prompts, parents, 16, 5, row_major=row_major)


@pytest.mark.parametrize("bs,ilp", [(4, 0), (8, 0), (32, 0), (64, 0),
                                    (16, 0), (16, 1)])
def test_other_instantiations(ops, bs, ilp):
    """Every FNV kernel the op can launch: each block size, and at 16 both
    values the retired ilp argument still accepts."""
    prompts, parents = _ragged(random.Random(bs * 10 + ilp), 257, bs)
    for row_major in (0, 1):
        _check(ops, FNV, prompts, parents, bs, 5, ilp=ilp,
               row_major=row_major)


def test_ilp_above_one_is_rejected(ops):
    """ilp is no selector any more: one chain per lane is the only kernel."""
    tt = _tokens_t([[1] * 16], 16)
    par = torch.zeros(1, dtype=torch.int64, device="cuda")
    nch = torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="ilp must be 0 or 1"):
        ops.gpu_hash_chain_tr(tt, par, nch, 16, 1, 2, 0, 0)
