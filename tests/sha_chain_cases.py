"""Shared case builders for the sha256-cbor-64 native chain tests
(test_sha_chain_native.py on the CPU, test_sha_chain_gpu.py on the
device).  The golden everywhere is hashing.CHAIN_ALGOS[name]: pure
Python over hashlib."""

from functools import lru_cache

from llmd_kvcache_amd.utils import hashing

SHA_ALGOS = ("sha256-cbor-64", "sha256-cbor-64-low")

# parent values by canonical-CBOR encoded length (1/2/3/5/9 bytes)
PARENTS_BY_LEN = {
    1: (0, 23),
    2: (24, 255),
    3: (256, 65535),
    5: (65536, 2**32 - 1),
    9: (2**32, 2**64 - 1),
}
# token values by encoded length (1/2/3/5 bytes)
TOKENS_BY_LEN = {
    1: (0, 23),
    2: (24, 255),
    3: (256, 65535),
    5: (65536, 2**32 - 1),
}


def _token_lens(n, total):
    """n token encoding lengths from {1,2,3,5} summing to `total`, or
    None when unreachable (e.g. 16 tokens cannot make 79)."""
    reach = [{0: []}]
    for _ in range(n):
        nxt = {}
        for s, lens in reach[-1].items():
            for ln in (1, 2, 3, 5):
                if s + ln <= total and s + ln not in nxt:
                    nxt[s + ln] = lens + [ln]
        reach.append(nxt)
    return reach[-1].get(total)


@lru_cache(maxsize=None)
def length_sweep_cases(block_size, lo, hi):
    """One-chunk cases (parent, tokens) whose CBOR payload is EXACTLY L
    bytes, for every L in lo..hi and every parent width that can reach
    it.  Returns a tuple of (L, parent, tokens).  A length no
    combination of encodings reaches is left out - callers assert which
    (at block size 16 only 91: it needs 16 tokens totalling 79 bytes
    after a 9-byte parent, and one short of all-5-byte is impossible
    with widths 1/2/3/5)."""
    hdr = len(hashing.cbor_encode_uint(block_size, major=4))
    cases = []
    pick = 0
    for L in range(lo, hi + 1):
        for plen, pvals in PARENTS_BY_LEN.items():
            lens = _token_lens(block_size, L - 1 - plen - hdr - 1)
            if lens is None:
                continue
            # rotate so mixed widths land at varying positions
            r = pick % block_size
            lens = lens[r:] + lens[:r]
            tokens = []
            for ln in lens:
                vals = TOKENS_BY_LEN[ln]
                tokens.append(vals[pick % 2])
                pick += 1
            parent = pvals[(len(cases) + L) % 2]
            payload = hashing.cbor_chunk_payload(parent, tokens)
            assert len(payload) == L, (L, len(payload))
            cases.append((L, parent, tuple(tokens)))
    return tuple(cases)


def golden_chain(algo, parent, tokens, block_size):
    link = hashing.CHAIN_ALGOS[algo][0]
    out = []
    h = parent
    for c in range(len(tokens) // block_size):
        h = link(h, tokens[c * block_size:(c + 1) * block_size])
        out.append(h)
    return out
