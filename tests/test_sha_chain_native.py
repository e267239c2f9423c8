"""Native (C++) sha256-cbor-64 chain: the host ops, the host build of the
device-shared code, and every Python layer that routes to them, against
the pure-Python hashlib golden (hashing.CHAIN_ALGOS)."""

import hashlib
import json
import random
import socket

import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402
from llmd_kvcache_amd.utils import hashing  # noqa: E402
from tests.sha_chain_cases import (  # noqa: E402
    SHA_ALGOS, golden_chain, length_sweep_cases)

pytestmark = pytest.mark.skipif(
    cpu_ext.maybe_load() is None, reason="native extension not built"
)

MODEL = "m"


@pytest.fixture(scope="module")
def ops():
    return cpu_ext.require()


def _i64(h):
    return h - (1 << 64) if h >= (1 << 63) else h


def _u64(h):
    return h + (1 << 64) if h < 0 else h


def test_algo_registry():
    """One name->id table; every native algo has a Python golden; the
    low-64 variant selects digest bytes 24..32 for links and the root."""
    assert hashing.NATIVE_ALGO_IDS == {
        "fnv-64a": 0, "sha256-cbor-64": 1, "sha256-cbor-64-low": 2}
    assert set(hashing.NATIVE_ALGO_IDS) <= set(hashing.CHAIN_ALGOS)
    link, init = hashing.CHAIN_ALGOS["sha256-cbor-64-low"]
    d = hashlib.sha256(hashing.cbor_chunk_payload(7, [1, 2, 3])).digest()
    assert link(7, [1, 2, 3]) == int.from_bytes(d[24:32], "big")
    assert link(7, [1, 2, 3]) == int.from_bytes(d, "big") & (2**64 - 1)
    assert init("seed") == int.from_bytes(
        hashlib.sha256(b"seed").digest()[24:32], "big")


def _check_cases(ops, cases, bs):
    for algo in SHA_ALGOS:
        aid = hashing.NATIVE_ALGO_IDS[algo]
        link = hashing.CHAIN_ALGOS[algo][0]
        for L, parent, tokens in cases:
            want = [link(parent, tokens)]
            toks = list(tokens)
            got = ops.tokens_to_chunk_hashes(toks, parent, bs, aid)
            assert got == want, ("host", algo, L, parent)
            got = ops.tokens_to_chunk_hashes_fast(toks, parent, bs, aid)
            assert got == want, ("device-shared", algo, L, parent)


def test_payload_length_sweep_bs16(ops):
    """Every reachable payload length 20..92 at block size 16 (SHA
    padding boundaries 55/56 and 63/64 included), all parent/token
    widths.  91 bytes is the one length no encoding mix reaches."""
    cases = length_sweep_cases(16, 20, 92)
    assert {c[0] for c in cases} == set(range(20, 93)) - {91}
    parents = {c[1] for c in cases}
    assert parents == {0, 23, 24, 255, 256, 65535, 65536, 2**32 - 1,
                       2**32, 2**64 - 1}
    assert {t for c in cases for t in c[2]} == {
        0, 23, 24, 255, 256, 65535, 65536, 2**32 - 1}
    _check_cases(ops, cases, 16)


def test_payload_length_sweep_bs32(ops):
    """Block size 32: lengths through the 2->3 block boundary (119/120)
    and past the 127/128 word-buffer boundary."""
    cases = length_sweep_cases(32, 37, 130)
    assert {c[0] for c in cases} == set(range(37, 131))
    _check_cases(ops, cases, 32)


def test_maximal_chunk_bs64(ops):
    """One maximal 333-byte payload: 6 SHA blocks."""
    parent = 2**64 - 1
    tokens = [2**32 - 1] * 64
    assert len(hashing.cbor_chunk_payload(parent, tokens)) == 333
    _check_cases(ops, [(333, parent, tuple(tokens))], 64)


@pytest.mark.parametrize("algo", SHA_ALGOS)
@pytest.mark.parametrize("bs", [4, 16, 17, 64])
def test_three_chunk_chains(ops, algo, bs):
    """3-chunk chains: links 2 and 3 take a full 9-byte hash parent."""
    rng = random.Random(bs)
    aid = hashing.NATIVE_ALGO_IDS[algo]
    widths = (24, 256, 65536, 2**32)
    for trial in range(20):
        tokens = [rng.randrange(widths[rng.randrange(4)])
                  for _ in range(3 * bs + trial % 3)]  # partial tail dropped
        parent = hashing.CHAIN_ALGOS[algo][1](f"seed{trial}")
        want = golden_chain(algo, parent, tokens, bs)
        assert len(want) == 3
        assert ops.tokens_to_chunk_hashes(tokens, parent, bs, aid) == want
        assert ops.tokens_to_chunk_hashes_fast(tokens, parent, bs,
                                               aid) == want


def test_fnv_default_unchanged(ops):
    """Omitting algo is algo 0 and is still the FNV golden."""
    tokens = list(range(100, 148))
    parent = hashing.init_hash("")
    want = golden_chain("fnv-64a", parent, tokens, 16)
    for fn in (ops.tokens_to_chunk_hashes, ops.tokens_to_chunk_hashes_fast):
        assert fn(tokens, parent, 16) == want
        assert fn(tokens, parent, 16, 0) == want
    with pytest.raises(RuntimeError):
        ops.tokens_to_chunk_hashes(tokens, parent, 16, 3)


@pytest.mark.parametrize("algo", SHA_ALGOS)
def test_hash_chain_batch_ragged(ops, algo):
    rng = random.Random(5)
    bs = 16
    aid = hashing.NATIVE_ALGO_IDS[algo]
    lens = [0, 5, 15, 16, 17, 48, 80, 33, 0, 160]
    prompts = [[rng.randrange(2**32) >> rng.choice((0, 8, 16, 24, 28))
                for _ in range(n)] for n in lens]
    parents = [rng.randrange(2**64) for _ in prompts]
    flat = torch.tensor([t for p in prompts for t in p], dtype=torch.int64)
    off = [0]
    for p in prompts:
        off.append(off[-1] + len(p))
    hashes, chunk_off = ops.hash_chain_batch(
        flat, torch.tensor(off, dtype=torch.int64),
        torch.tensor([_i64(p) for p in parents], dtype=torch.int64), bs, aid)
    chunk_off = chunk_off.tolist()
    assert [chunk_off[i + 1] - chunk_off[i] for i in range(len(lens))] == \
        [n // bs for n in lens]
    for b, p in enumerate(prompts):
        got = [_u64(h) for h in
               hashes[chunk_off[b]:chunk_off[b + 1]].tolist()]
        assert got == golden_chain(algo, parents[b], p, bs), b


@pytest.mark.parametrize("algo", SHA_ALGOS)
@pytest.mark.parametrize("native", [True, False])
def test_token_processor_keys(monkeypatch, algo, native):
    from llmd_kvcache_amd.kvblock.token_processor import (
        ChunkedTokenDatabase, TokenProcessorConfig)

    tp = ChunkedTokenDatabase(TokenProcessorConfig(
        block_size=16, hash_seed="s", hash_algo=algo))
    if native:
        assert tp._native is not None
        calls = []
        real = tp._native.tokens_to_chunk_hashes

        class Spy:
            def tokens_to_chunk_hashes(self, *a):
                calls.append(a)
                return real(*a)

        monkeypatch.setattr(tp, "_native", Spy())
    else:
        monkeypatch.setattr(tp, "_native", None)
    tokens = [(i * 2654435761) % 2**32 for i in range(70)]
    keys = tp.tokens_to_kv_block_keys(None, tokens, MODEL)
    want = golden_chain(algo, hashing.CHAIN_ALGOS[algo][1]("s"), tokens, 16)
    assert [k.chunk_hash for k in keys] == want
    if native:  # the C++ op did the work, with this algo's id
        assert calls and calls[0][3] == hashing.NATIVE_ALGO_IDS[algo]


def _sha_indexers(algo="sha256-cbor-64", bs=4):
    """(native-table indexer, in-memory indexer) sharing one config."""
    from llmd_kvcache_amd.indexer import Config, Indexer
    from llmd_kvcache_amd.kvblock import InMemoryIndex
    from llmd_kvcache_amd.kvblock.gpu_index import (NativeIndex,
                                                    TableIndexConfig)
    from llmd_kvcache_amd.kvblock.token_processor import TokenProcessorConfig

    def make(index):
        cfg = Config(token_processor=TokenProcessorConfig(
            block_size=bs, hash_algo=algo))
        return Indexer(cfg, kv_block_index=index)

    return (make(NativeIndex(TableIndexConfig(capacity=1 << 12,
                                              pods_per_key=4))),
            make(InMemoryIndex()))


def _ingest(indexer, stream):
    from llmd_kvcache_amd.kvevents.pool import digest_events

    for pod, events in stream:
        digest_events(indexer.kv_block_index(), indexer.tokens_processor,
                      pod, MODEL, events)


def _event_stream(bs):
    from llmd_kvcache_amd.kvevents.events import BlockRemoved, BlockStored

    base = [(i * 7919) % 50000 for i in range(8 * bs)]
    other = [(i * 104729) % 2**32 for i in range(4 * bs)]
    stream = [
        ("pod-a", [BlockStored(list(range(100, 104)), None, base[:4 * bs],
                               bs)]),
        ("pod-a", [BlockStored(list(range(104, 108)), 103, base[4 * bs:],
                               bs)]),
        ("pod-b", [BlockStored(list(range(200, 203)), None, base[:3 * bs],
                               bs, medium="cpu")]),
        ("pod-b", [BlockStored(list(range(300, 304)), None, other, bs)]),
        ("pod-b", [BlockRemoved([302, 303])]),
    ]
    prompts = [base, base[:5 * bs + 1], other, other[:bs], base[:bs - 1],
               [], [9] * (2 * bs)]
    return stream, prompts


def test_indexer_batch_scores_match_in_memory():
    """score_tokens_batch takes the batched native route for a SHA algo
    and agrees with InMemoryIndex + the Python scorer."""
    native_ix, mem_ix = _sha_indexers()
    stream, prompts = _event_stream(4)
    _ingest(native_ix, stream)
    _ingest(mem_ix, stream)
    tp = native_ix.tokens_processor

    routed = []
    real = native_ix.score_flat_tokens

    def spy(*a, **k):
        routed.append(1)
        return real(*a, **k)

    native_ix.score_flat_tokens = spy
    got = native_ix.score_tokens_batch(prompts, MODEL, [])
    assert routed, "SHA algo fell back to the per-prompt Python chain"
    want = []
    for p in prompts:
        keys = tp.tokens_to_kv_block_keys(None, p, MODEL)
        if not keys:
            want.append({})
            continue
        want.append(mem_ix.kv_block_scorer.score(
            keys, mem_ix.kv_block_index().lookup(keys, set())))
    assert any(w for w in want)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == pytest.approx(w)
    # and it is the SHA chain that keyed the table
    keys = tp.tokens_to_kv_block_keys(None, prompts[0], MODEL)
    assert [k.chunk_hash for k in keys] == golden_chain(
        "sha256-cbor-64", hashing.sha256_init_hash(""), prompts[0], 4)


def _post_score(port, tokens):
    body = json.dumps({"model": MODEL, "tokens": tokens}).encode()
    s = socket.create_connection(("127.0.0.1", port), timeout=10)
    s.settimeout(10)
    try:
        s.sendall((f"POST /score HTTP/1.1\r\nhost: x\r\n"
                   f"content-length: {len(body)}\r\n\r\n").encode() + body)
        buf = b""
        while b"\r\n\r\n" not in buf:
            chunk = s.recv(65536)
            assert chunk, "connection closed early"
            buf += chunk
        head, rest = buf.split(b"\r\n\r\n", 1)
        clen = 0
        for line in head.split(b"\r\n")[1:]:
            k, _, v = line.partition(b":")
            if k.lower() == b"content-length":
                clen = int(v.strip())
        while len(rest) < clen:
            chunk = s.recv(65536)
            assert chunk, "connection closed mid-body"
            rest += chunk
        return int(head.split(b" ", 2)[1]), json.loads(rest[:clen])
    finally:
        s.close()


@pytest.mark.parametrize("algo", SHA_ALGOS)
def test_wirefront_serves_sha_index(algo):
    from llmd_kvcache_amd.service.wirefront import WireIndexerService

    native_ix, _ = _sha_indexers(algo)
    stream, prompts = _event_stream(4)
    _ingest(native_ix, stream)
    svc = WireIndexerService(native_ix)
    port = svc.start(port=0, n_io=1)
    try:
        hit = False
        for p in prompts[:4]:
            status, body = _post_score(port, p)
            assert status == 200
            want = native_ix.score_tokens(p, MODEL, [])
            assert body["scores"] == pytest.approx(want)
            hit = hit or bool(want)
        assert hit
    finally:
        svc.stop()


def test_wirefront_rejects_algo_without_native_id(monkeypatch):
    from llmd_kvcache_amd.indexer import Config, Indexer
    from llmd_kvcache_amd.kvblock.gpu_index import (NativeIndex,
                                                    TableIndexConfig)
    from llmd_kvcache_amd.kvblock.token_processor import TokenProcessorConfig
    from llmd_kvcache_amd.service.wirefront import WireIndexerService

    monkeypatch.setitem(
        hashing.CHAIN_ALGOS, "python-only",
        (lambda parent, tokens: (parent * 31 + sum(tokens)) % 2**64,
         lambda seed="": 1))
    cfg = Config(token_processor=TokenProcessorConfig(
        block_size=4, hash_algo="python-only"))
    indexer = Indexer(cfg, kv_block_index=NativeIndex(
        TableIndexConfig(capacity=1 << 10, pods_per_key=4)))
    # the Python chain still serves such an algo...
    assert len(indexer.tokens_processor.tokens_to_kv_block_keys(
        None, list(range(8)), MODEL)) == 2
    assert indexer.score_tokens_batch([list(range(8))], MODEL, []) == [{}]
    # ...but the native wire front refuses it
    with pytest.raises(ValueError):
        WireIndexerService(indexer)
