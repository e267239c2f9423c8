"""gfx950 sha256-cbor-64 chain kernels and the on-device event ingest
keyed by them, against the pure-Python hashlib golden
(hashing.CHAIN_ALGOS).  All tests require an MI355X."""

import random

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex, GpuIndexConfig, _to_i64, _to_u64)
from llmd_kvcache_amd.kvblock.keys import Key  # noqa: E402
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    ChunkedTokenDatabase, TokenProcessorConfig)
from llmd_kvcache_amd.kvevents.events import (  # noqa: E402
    BlockRemoved, BlockStored, EventBatch)
from llmd_kvcache_amd.utils import hashing  # noqa: E402
from tests.sha_chain_cases import (  # noqa: E402
    golden_chain, length_sweep_cases)

MODEL = "m"
SHA = "sha256-cbor-64"
SHA_LOW = "sha256-cbor-64-low"
WIDTH_SHIFTS = (0, 8, 16, 24, 28)  # token widths 5/5/3/2/1 bytes


@pytest.fixture(scope="module")
def ops():
    from llmd_kvcache_amd.ops import cpu_ext

    mod = cpu_ext.require()
    assert mod.HAS_HIP
    return mod


def _rand_tokens(rng, n):
    return [rng.randrange(2**32) >> rng.choice(WIDTH_SHIFTS)
            for _ in range(n)]


def _i64_tensor(vals):
    return torch.tensor([_to_i64(v) for v in vals], dtype=torch.int64,
                        device="cuda")


def _tokens_t(prompts, rows):
    """[rows, B] int32 (uint32 bit pattern), zero padded."""
    import numpy as np

    t = np.zeros((rows, len(prompts)), dtype=np.uint32)
    for b, p in enumerate(prompts):
        t[:len(p), b] = p
    return torch.from_numpy(t.view(np.int32)).cuda()


def test_gpu_hash_chain_sha(ops):
    rng = random.Random(11)
    B, bs = 70, 16  # more than one wave, not a multiple of 64
    prompts = [_rand_tokens(rng, (b % 6) * bs + (b % 3)) for b in range(B)]
    parents = [rng.randrange(2**64) for _ in range(B)]
    off = [0]
    for p in prompts:
        off.append(off[-1] + len(p))
    out, chunk_off = ops.gpu_hash_chain(
        torch.tensor([t for p in prompts for t in p], dtype=torch.int64,
                     device="cuda"),
        torch.tensor(off, dtype=torch.int64, device="cuda"),
        _i64_tensor(parents), bs, 1)
    out = out.cpu().tolist()
    chunk_off = chunk_off.cpu().tolist()
    for b, p in enumerate(prompts):
        got = [_to_u64(h) for h in out[chunk_off[b]:chunk_off[b + 1]]]
        assert got == golden_chain(SHA, parents[b], p, bs), b


def _run_tr(ops, algo, bs, row_major, seed):
    rng = random.Random(seed)
    B, max_chunks = 130, 3
    aid = hashing.NATIVE_ALGO_IDS[algo]
    n_chunks = [b % 4 for b in range(B)]  # ragged, zeros included
    prompts = [_rand_tokens(rng, n * bs) for n in n_chunks]
    parents = [rng.randrange(2**64) if b % 5 else rng.randrange(300)
               for b in range(B)]
    out = ops.gpu_hash_chain_tr(
        _tokens_t(prompts, max_chunks * bs), _i64_tensor(parents),
        torch.tensor(n_chunks, dtype=torch.int32, device="cuda"), bs,
        max_chunks, 0, row_major, aid).cpu()
    assert tuple(out.shape) == ((B, max_chunks) if row_major
                                else (max_chunks, B))
    for b, p in enumerate(prompts):
        want = golden_chain(algo, parents[b], p, bs)
        col = (out[b] if row_major else out[:, b]).tolist()
        assert [_to_u64(h) for h in col[:len(want)]] == want, b
        assert col[len(want):] == [0] * (max_chunks - len(want)), b


@pytest.mark.parametrize("row_major", [0, 1])
@pytest.mark.parametrize("bs", [4, 8, 16, 32, 64])
def test_gpu_hash_chain_tr_sha(ops, bs, row_major):
    _run_tr(ops, SHA, bs, row_major, seed=bs)


@pytest.mark.parametrize("row_major", [0, 1])
def test_gpu_hash_chain_tr_sha_low(ops, row_major):
    _run_tr(ops, SHA_LOW, 16, row_major, seed=99)


def test_gpu_hash_chain_tr_rejects_other_sizes(ops):
    with pytest.raises(RuntimeError):
        ops.gpu_hash_chain_tr(
            torch.zeros((17, 1), dtype=torch.int32, device="cuda"),
            torch.zeros(1, dtype=torch.int64, device="cuda"),
            torch.ones(1, dtype=torch.int32, device="cuda"), 17, 1, 0, 0, 1)


def _sweep_launch(ops, cases, algo):
    aid = hashing.NATIVE_ALGO_IDS[algo]
    link = hashing.CHAIN_ALGOS[algo][0]
    prompts = [list(c[2]) for c in cases]
    parents = [c[1] for c in cases]
    out = ops.gpu_hash_chain_tr(
        _tokens_t(prompts, 16), _i64_tensor(parents),
        torch.ones(len(cases), dtype=torch.int32, device="cuda"), 16, 1, 0,
        0, aid).cpu()[0].tolist()
    for (L, parent, tokens), h in zip(cases, out):
        assert _to_u64(h) == link(parent, tokens), (L, parent)


def test_payload_length_sweep_on_device(ops):
    """One chunk per lane, every reachable payload length 20..92 in ONE
    launch of 73 lanes with per-lane parents: each SHA padding boundary
    (55/56, 63/64) shares a wave with lanes of the other block count."""
    cases = length_sweep_cases(16, 20, 92)
    by_len = {}
    for c in cases:  # widest parent reaching each length
        by_len[c[0]] = c
    lanes = [by_len[L] for L in sorted(by_len)]
    assert len(lanes) == 72  # 91 bytes is unreachable (sha_chain_cases)
    lanes.append(cases[0])
    assert len(lanes) == 73
    _sweep_launch(ops, lanes, SHA)
    _sweep_launch(ops, lanes, SHA_LOW)
    # and every parent width of every length, shuffled across waves
    mixed = list(cases)
    random.Random(3).shuffle(mixed)
    _sweep_launch(ops, mixed, SHA)


class _OpsSpy:
    """Records which native ops a table calls; optionally drops the
    trailing algo argument of the event ops (the pre-feature call)."""

    EVENT_OPS = ("gpu_apply_events", "gpu_apply_events_split",
                 "gpu_apply_events_split_tr")

    def __init__(self, mod, drop_algo=False):
        self._mod = mod
        self._drop = drop_algo
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if name not in self.EVENT_OPS:
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*(args[:-1] if self._drop else args))

        return call


def _route_batches(bs):
    """(route op, batches) for each kernel apply_event_batches picks;
    ~8 events, 2 pods, <= 4 blocks each."""
    rng = random.Random(17)

    def toks(n_blocks):
        return _rand_tokens(rng, n_blocks * bs)

    independent = [
        ("pod-a", MODEL, [BlockStored([100, 101, 102], None, toks(3), bs)]),
        ("pod-b", MODEL, [BlockStored([110], None, toks(1), bs)]),
        ("pod-a", MODEL, [BlockStored([120, 121, 122, 123], None, toks(4),
                                      bs)]),
        ("pod-b", MODEL, [BlockStored([130, 131], None, toks(2), bs,
                                      medium="cpu")]),
    ]
    chained = [  # second event's parent is stored by the first, same batch
        ("pod-a", MODEL, [BlockStored([200, 201], None, toks(2), bs),
                          BlockStored([202, 203], 201, toks(2), bs)]),
        # parent from the earlier batch resolves via the engine map
        ("pod-b", MODEL, [BlockStored([210], 110, toks(1), bs)]),
    ]
    store_remove = [  # stores and removes engine hash 301 in one batch
        ("pod-a", MODEL, [BlockStored([300, 301, 302], 102, toks(3), bs),
                          BlockRemoved([301])]),
        ("pod-b", MODEL, [BlockRemoved([110])]),
    ]
    return [("gpu_apply_events_split_tr", independent),
            ("gpu_apply_events_split", chained),
            ("gpu_apply_events", store_remove)]


def _assert_same_state(gpu, ref, tp, batches_so_far):
    """The Python-golden request key of every stored block returns the
    same pods from both indexes, and get_request_key agrees (and is the
    golden key) for every engine hash the reference still maps - it
    forgets an engine hash once its block empties, the table keeps it."""
    algo = tp.config.hash_algo
    bs = tp.block_size
    golden = {}  # engine hash -> golden request hash, never forgotten
    live = 0
    for _, model, events in batches_so_far:
        for ev in events:
            if not isinstance(ev, BlockStored):
                continue
            parent = (tp.config.init_hash() if ev.parent_block_hash is None
                      else golden[ev.parent_block_hash])
            chain = golden_chain(algo, parent, ev.token_ids, bs)
            assert len(chain) == len(ev.block_hashes)
            golden.update(zip(ev.block_hashes, chain))
    for eh, rh in golden.items():
        ek, rk = Key(MODEL, eh), Key(MODEL, rh)
        want = ref.lookup([rk], set()).get(rk, [])
        got = gpu.lookup([rk], set()).get(rk, [])
        assert set(got) == set(want), eh
        live += bool(want)
        ref_rk = ref.get_request_key(ek)
        if ref_rk is not None:
            assert ref_rk == rk
            assert gpu.get_request_key(ek) == rk, eh
    assert live


@pytest.mark.parametrize("algo", [SHA, SHA_LOW])
def test_event_ingest_all_routes(algo):
    from llmd_kvcache_amd.kvblock import InMemoryIndex
    from llmd_kvcache_amd.kvevents.pool import digest_events

    bs = 16
    tp = ChunkedTokenDatabase(TokenProcessorConfig(block_size=bs,
                                                   hash_algo=algo))
    gpu = GpuIndex(GpuIndexConfig(capacity=1 << 14, pods_per_key=10))
    spy = gpu.table.ops = _OpsSpy(gpu.table.ops)
    ref = InMemoryIndex()
    applied = []
    for route, batches in _route_batches(bs):
        for pod, model, events in batches:
            digest_events(ref, tp, pod, model, events)
        gpu.apply_event_batches(batches, tp)
        torch.cuda.synchronize()
        assert spy.calls[-1] == route
        applied += batches
        _assert_same_state(gpu, ref, tp, applied)
    # the request keys ARE the Python-golden SHA chain
    ev = applied[0][2][0]
    want = golden_chain(algo, tp.config.init_hash(), ev.token_ids, bs)
    keys = [Key(MODEL, h) for h in want]
    assert set(gpu.lookup(keys, set())) == set(keys)
    assert gpu.get_request_key(Key(MODEL, ev.block_hashes[0])) == keys[0]


def test_fnv_wrappers_default_algo(ops):
    """algo omitted == algo 0, bit for bit, on every wrapper."""
    rng = random.Random(23)
    bs, B = 16, 70
    prompts = [_rand_tokens(rng, 2 * bs) for _ in range(B)]
    parents = _i64_tensor([rng.randrange(2**64) for _ in range(B)])
    flat = torch.tensor([t for p in prompts for t in p], dtype=torch.int64,
                        device="cuda")
    off = torch.arange(0, (B + 1) * 2 * bs, 2 * bs, dtype=torch.int64,
                       device="cuda")
    a = ops.gpu_hash_chain(flat, off, parents, bs)
    b = ops.gpu_hash_chain(flat, off, parents, bs, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    want = [golden_chain("fnv-64a", _to_u64(int(p)), t, bs)
            for p, t in zip(parents.cpu().tolist(), prompts)]
    assert [_to_u64(h) for h in a[0].cpu().tolist()] == \
        [h for w in want for h in w]
    tt = _tokens_t(prompts, 2 * bs)
    nch = torch.full((B,), 2, dtype=torch.int32, device="cuda")
    for row_major in (0, 1):
        a = ops.gpu_hash_chain_tr(tt, parents, nch, bs, 2, 0, row_major)
        b = ops.gpu_hash_chain_tr(tt, parents, nch, bs, 2, 0, row_major, 0)
        assert torch.equal(a, b)

    # the three event wrappers: same batches with and without the argument
    from llmd_kvcache_amd.kvblock import InMemoryIndex
    from llmd_kvcache_amd.kvevents.pool import digest_events

    tp = ChunkedTokenDatabase(TokenProcessorConfig(block_size=bs))
    with_arg = GpuIndex(GpuIndexConfig(capacity=1 << 14, pods_per_key=10))
    without = GpuIndex(GpuIndexConfig(capacity=1 << 14, pods_per_key=10))
    spy = without.table.ops = _OpsSpy(without.table.ops, drop_algo=True)
    ref = InMemoryIndex()
    applied = []
    for route, batches in _route_batches(bs):
        for pod, model, events in batches:
            digest_events(ref, tp, pod, model, events)
        with_arg.apply_event_batches(batches, tp)
        without.apply_event_batches(batches, tp)
        torch.cuda.synchronize()
        assert spy.calls[-1] == route
        applied += batches
    _assert_same_state(with_arg, ref, tp, applied)
    _assert_same_state(without, ref, tp, applied)


def _indexer(index, algo):
    from llmd_kvcache_amd.indexer import Config, Indexer

    cfg = Config(token_processor=TokenProcessorConfig(block_size=16,
                                                      hash_algo=algo))
    return Indexer(cfg, kv_block_index=index)


def _pump(pool, stream):
    from llmd_kvcache_amd.kvevents.pool import Message

    pool.start(with_subscriber=False)
    try:
        for seq, (pod, events) in enumerate(stream):
            pool.add_task(Message(
                topic=f"kv@{pod}@{MODEL}",
                payload=EventBatch(ts=0.0, events=events).encode(),
                seq=seq, pod_identifier=pod, model_name=MODEL))
        pool.drain()
    finally:
        pool.shutdown()


def _e2e_stream():
    rng = random.Random(31)
    bs = 16
    base = _rand_tokens(rng, 8 * bs)
    other = _rand_tokens(rng, 4 * bs)
    stream = [
        ("pod-a", [BlockStored(list(range(100, 104)), None, base[:4 * bs],
                               bs)]),
        ("pod-a", [BlockStored(list(range(104, 108)), 103, base[4 * bs:],
                               bs)]),
        ("pod-b", [BlockStored(list(range(200, 203)), None, base[:3 * bs],
                               bs, medium="cpu")]),
        ("pod-b", [BlockStored(list(range(300, 304)), None, other, bs)]),
        ("pod-b", [BlockRemoved([303])]),
    ]
    prompts = [base, base[:5 * bs + 3], other, other[:bs], base[:bs - 1],
               [], _rand_tokens(rng, 2 * bs)]
    return stream, prompts


def _e2e_scores(algo, monkeypatch=None):
    from llmd_kvcache_amd.kvblock import InMemoryIndex
    from llmd_kvcache_amd.kvevents.pool import EventsConfig, EventsPool

    stream, prompts = _e2e_stream()
    out = []
    for index in (GpuIndex(GpuIndexConfig(capacity=1 << 14,
                                          pods_per_key=10)),
                  InMemoryIndex()):
        ix = _indexer(index, algo)
        _pump(EventsPool(EventsConfig(concurrency=1), index,
                         ix.tokens_processor), stream)
        out.append(ix.score_tokens_batch(prompts, MODEL, []))
    return out


def test_pool_to_gpu_index_to_batch_scores():
    """kvevents.Pool -> GpuIndex (on-device ingest) -> batched scoring
    agrees with the InMemoryIndex indexer on the same stream.  Before
    the kernels honoured hash_algo the GPU side scored all zeros."""
    got, want = _e2e_scores(SHA)
    assert want[0] and want[1] and want[2]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == pytest.approx(w)


def test_algo_without_native_id_falls_back_to_per_event_path(monkeypatch):
    """Such an algo must not reach the kernels: apply_event_batches
    raises and the pool's per-event Python path applies the burst."""
    monkeypatch.setitem(
        hashing.CHAIN_ALGOS, "python-only",
        (lambda parent, tokens: (parent * 31 + sum(tokens) + 1) % 2**64,
         lambda seed="": 1))
    tp = ChunkedTokenDatabase(TokenProcessorConfig(block_size=16,
                                                   hash_algo="python-only"))
    gpu = GpuIndex(GpuIndexConfig(capacity=1 << 14, pods_per_key=10))
    with pytest.raises(ValueError):
        gpu.apply_event_batches(
            [("pod-a", MODEL, [BlockStored([1], None, list(range(16)),
                                           16)])], tp)
    got, want = _e2e_scores("python-only")
    assert want[0] and want[2]
    for g, w in zip(got, want):
        assert g == pytest.approx(w)
