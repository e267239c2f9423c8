"""The read path with the chain on the device, on MI355X, piece by piece
and whole, every comparison exact:

 - gpu_stage_ragged_tokens against the transposed int32 image built in
   numpy (lengths at the chunk edges and at the edges of the kernel's
   64-position tile, prompt counts at the edges of its 64-prompt tile,
   token values at the edges of the 32-bit narrowing);
 - gpu_hash_chain_tr on the staged image against hash_chain_batch on the
   same flat tokens, every chunk of every prompt, zeros past the end;
 - gpu_fused_score_rows on padded rows against gpu_fused_score on the
   compacted hashes, the padding filled with a key the table holds so
   that a walk past n_keys[b] changes the score;
 - Indexer.score_flat_tokens and wire_score_flat with the device route on
   against the CPU-chain route, including the batches that must fall
   back (masks too large for LDS, image over the cap, block size 24).
"""

import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.indexer import Config, Indexer  # noqa: E402
from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex,
    GpuIndexConfig,
    KvTable,
    TableIndexConfig,
    _to_i64,
)
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    ChunkedTokenDatabase,
    TokenProcessorConfig,
)
from llmd_kvcache_amd.kvevents.events import BlockStored  # noqa: E402
from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402
from llmd_kvcache_amd.utils import hashing  # noqa: E402

LENS = [0, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1040]
SPECIAL = [0, 2**31 - 1, 2**31, 2**32 - 1, 2**32 + 5, 2**63 - 1, -1]
ALGOS = sorted(hashing.NATIVE_ALGO_IDS)


def _ops():
    return cpu_ext.require()


def _ragged(B, seed=0):
    """-> flat int64 tokens (numpy), int64 offsets [B+1] (numpy).  The
    lengths cycle through LENS, shifted so that the first and (for
    B > 1) the last prompt are empty; B == 1 is one 1040-token prompt."""
    if B == 1:
        lens = [1040]
    else:
        lens = [0] + [LENS[(i + 1) % len(LENS)] for i in range(B - 2)] + [0]
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    rng = np.random.default_rng(seed + B)
    flat = rng.integers(-2**63, 2**63 - 1, size=int(off[-1]), dtype=np.int64)
    # the special values, all over: at every 5th slot, so that they land
    # at the starts and ends of chunks and tiles as well
    for i in range(0, flat.size, 5):
        flat[i] = SPECIAL[(i // 5) % len(SPECIAL)]
    return flat, off


def _np_image(flat, off, bs):
    lens = off[1:] - off[:-1]
    nc = (lens // bs).astype(np.int32)
    max_k = int(nc.max()) if nc.size else 0
    img = np.zeros((max_k * bs, nc.size), dtype=np.int32)
    low = (flat & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    for b in range(nc.size):
        n = int(nc[b]) * bs
        img[:n, b] = low[off[b]:off[b] + n]
    return img, nc


STAGE_CASES = [(16, B) for B in (1, 63, 64, 65, 130)] + [(4, 65), (64, 65)]


@pytest.mark.parametrize("bs,B", STAGE_CASES)
@pytest.mark.parametrize("src", ["host_i64", "dev_i64", "dev_i32"])
def test_stage_matches_numpy_image(bs, B, src):
    flat, off = _ragged(B)
    want, want_nc = _np_image(flat, off, bs)
    tok = torch.from_numpy(flat)
    if src == "dev_i64":
        tok = tok.cuda()
    elif src == "dev_i32":
        low = (flat & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        tok = torch.from_numpy(low).cuda()
    img, nc = _ops().gpu_stage_ragged_tokens(tok, torch.from_numpy(off), bs)
    assert img.is_cuda and img.dtype == torch.int32
    assert nc.is_cuda and nc.dtype == torch.int32
    assert tuple(img.shape) == want.shape
    assert np.array_equal(nc.cpu().numpy(), want_nc)
    assert np.array_equal(img.cpu().numpy(), want)
    if B > 1:
        assert want.any() and not want[:, 0].any() and not want[:, -1].any()


def test_stage_rejects_offsets_outside_the_tokens():
    tok = torch.zeros(32, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        _ops().gpu_stage_ragged_tokens(
            tok, torch.tensor([0, 16, 48], dtype=torch.int64), 16)
    with pytest.raises(RuntimeError):
        _ops().gpu_stage_ragged_tokens(
            tok, torch.tensor([0, 16, 8], dtype=torch.int64), 16)


@pytest.mark.parametrize("bs", [16, 64])
@pytest.mark.parametrize("algo", ALGOS)
def test_chain_on_staged_image_matches_cpu_chain(algo, bs):
    ops = _ops()
    B = 130
    flat, off = _ragged(B, seed=7)
    tok, off_t = torch.from_numpy(flat), torch.from_numpy(off)
    algo_id = hashing.NATIVE_ALGO_IDS[algo]
    init = _to_i64(TokenProcessorConfig(hash_algo=algo).init_hash())
    parents = torch.full((B,), init, dtype=torch.int64)
    want, chunk_off = ops.hash_chain_batch(tok, off_t, parents, bs, algo_id)
    want, chunk_off = want.numpy(), chunk_off.numpy()

    img, nc = ops.gpu_stage_ragged_tokens(tok, off_t, bs)
    max_k = img.shape[0] // bs
    rows = ops.gpu_hash_chain_tr(img, parents.cuda(), nc, bs, max_k, 0, 1,
                                 algo_id).cpu().numpy()
    assert rows.shape == (B, max_k) and max_k == 1040 // bs
    nc = nc.cpu().numpy()
    assert np.array_equal(nc, chunk_off[1:] - chunk_off[:-1])
    live = np.arange(max_k)[None, :] < nc[:, None]
    assert np.array_equal(rows[live], want)  # row-major order = flat order
    assert not rows[~live].any()
    assert live.sum() == want.size > 0


# --- gpu_fused_score_rows -------------------------------------------------
# The table builder of tests/test_fused_score_walk_gpu.py, copied.

MODEL = 3
KS = [0, 1, 63, 64, 65, 129, 512, 0]
DROPS = [0, 63, 64, 65, None]  # key at which a pod leaves; None = stays
WEIGHTS = [1.0, 0.8, 0.3, 1.0]
CALL_EPOCH = 1_000_000


def _i64(h):
    return h - (1 << 64) if h >= (1 << 63) else h


def _entry(pod, tier):
    return (tier << 24) | (pod + 1)


def _build(num_pods, n_tiers, ppk, seed):
    """-> table, prompts (lists of int64 hashes), hashes stored in it."""
    rng = random.Random(seed)
    table = KvTable(TableIndexConfig(capacity=1 << 12, pods_per_key=ppk,
                                     device="cuda:0"))
    used = set()

    def fresh():
        while True:
            h = rng.randrange(1, 2**64)
            if h not in used:
                used.add(h)
                return h

    prompts = []
    by_row = {}  # tuple of pod entries -> hashes that carry that row
    for pi, K in enumerate(KS):
        keys = [fresh() for _ in range(K)]
        prompts.append(keys)
        # up to ppk member pods, spread over the pod words; each leaves
        # at its own key
        members = []
        for j in range(min(ppk, num_pods)):
            pod = (pi * 7 + j * 37) % num_pods
            if pod not in [m[0] for m in members]:
                members.append((pod, DROPS[(pi + j) % len(DROPS)]))
        if K == 512:
            members[0] = (members[0][0], None)  # all 512 keys hit
        missing = set()
        if K == 129:
            missing.add(0)    # miss at key 0: every score is 0
        if K == 65:
            missing.add(2)    # hit-miss-hit: stops at the miss
        empty_row = {40} if K == 64 else set()  # present, no pods
        for k, h in enumerate(keys):
            if k in missing:
                continue
            row = []
            if k not in empty_row:
                for pod, drop in members:
                    if drop is None or k < drop:
                        row.append(_entry(pod, (pod + k) % n_tiers))
                # one pod on two tiers at once, where the row has room
                if row and len(row) < ppk and n_tiers > 1 and k % 5 == 0:
                    pod = members[-1][0]
                    row.append(_entry(pod, (pod + k + 1) % n_tiers))
            by_row.setdefault(tuple(row), []).append(h)
    for row, hs in by_row.items():
        ht = torch.tensor([_i64(h) for h in hs], dtype=torch.int64,
                          device="cuda")
        table.insert(ht, ht, MODEL,
                     torch.tensor(row, dtype=torch.int32, device="cuda"))
    stored = [h for hs in by_row.values() for h in hs]
    return table, prompts, stored


@pytest.mark.parametrize("num_pods,n_tiers,ppk", [(64, 1, 10), (200, 3, 16)])
def test_fused_score_rows_matches_flat(num_pods, n_tiers, ppk):
    table, prompts, stored = _build(num_pods, n_tiers, ppk,
                                    seed=num_pods * 100 + n_tiers * 10 + ppk)
    ops = table.ops
    W = (num_pods + 63) // 64
    max_k = max(KS)
    flat = [h for p in prompts for h in p]
    hashes = torch.tensor([_i64(h) for h in flat], dtype=torch.int64,
                          device="cuda")
    counts = torch.tensor([len(p) for p in prompts], dtype=torch.int32)
    offsets = torch.zeros(len(prompts) + 1, dtype=torch.int32)
    offsets[1:] = torch.cumsum(counts, 0)
    # padded rows; the padding is a key that is in the table with pods on
    # it (key 0 of the all-hit prompt), not zero
    pad = prompts[6][0]
    assert pad in stored
    rows = torch.full((len(prompts), max_k), _i64(pad), dtype=torch.int64)
    for b, p in enumerate(prompts):
        rows[b, :len(p)] = torch.tensor([_i64(h) for h in p],
                                        dtype=torch.int64)
    rows = rows.cuda()
    weights = torch.tensor(WEIGHTS, dtype=torch.float32, device="cuda")
    allow = [0] * W
    for p in range(num_pods):
        if p % 3 != 1:
            allow[p // 64] |= 1 << (p % 64)
    filters = [torch.zeros(0, dtype=torch.int64, device="cuda"),
               torch.tensor([_i64(a) for a in allow], dtype=torch.int64,
                            device="cuda")]
    for call, filt in enumerate(filters):
        epoch = CALL_EPOCH + call
        want = ops.gpu_fused_score(*table._t(), hashes, offsets.cuda(), MODEL,
                                   filt, weights, num_pods, epoch, max_k,
                                   n_tiers)
        got = ops.gpu_fused_score_rows(*table._t(), rows, counts.cuda(),
                                       MODEL, filt, weights, num_pods, epoch,
                                       max_k, n_tiers)
        assert tuple(got.shape) == (len(prompts), num_pods)
        assert torch.equal(got, want)
        if call == 0:
            got = got.cpu()
            assert got[6].max().item() > 500 * min(WEIGHTS[:n_tiers])
            # the padding key alone would score: rows 0 and 7 hold nothing
            # else, and must score nothing
            assert got[0].abs().sum().item() == 0
            assert got[7].abs().sum().item() == 0
            assert got[1].max().item() <= 1.0


# --- the whole route --------------------------------------------------------

class _SpyOps:
    """The ops module with a count of gpu_score_flat_tokens calls."""

    def __init__(self, real):
        self._real = real
        self.device_calls = 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name != "gpu_score_flat_tokens":
            return fn

        def counted(*a, **kw):
            self.device_calls += 1
            return fn(*a, **kw)

        return counted


def _world(algo="fnv-64a", bs=16, n_pods=6, tiers=None, lens=None, seed=1,
           **cfg_kw):
    """One GpuIndex filled through apply_event_batches, an "off" and an
    "on" Indexer over it, and a batch (flat tokens, offsets) whose
    prompts share prefixes of different depth with what the pods hold."""
    rng = random.Random(seed)
    tpc = TokenProcessorConfig(block_size=bs, hash_algo=algo)
    icfg = GpuIndexConfig(capacity=1 << 14, pods_per_key=10)
    if tiers:
        icfg.tier_names = list(tiers)
    gpu = GpuIndex(icfg)
    for i in range(n_pods):
        gpu.registry.pod_id(f"pod-{i}")
    tp = ChunkedTokenDatabase(tpc)
    lens = lens or [0, bs * 3 + 1, bs * 40, bs - 1, bs * 7 + 5, 1040, 0]
    prompts = [[rng.randrange(0, 1 << 31) for _ in range(n)] for n in lens]
    tiers = list(tiers or ["gpu", "cpu"])
    batches = []
    hid = 1000
    for j, p in enumerate(prompts):
        k = len(p) // bs
        if k == 0:
            continue
        for m in range(3):  # three pods hold prefixes of different depth
            depth = max(1, k * (m + 1) // 3)
            pod = f"pod-{(j * 3 + m * 5) * 43 % n_pods}"
            ev = BlockStored(list(range(hid, hid + depth)), None,
                             p[:depth * bs], bs,
                             medium=tiers[(j + m) % len(tiers)])
            hid += depth
            batches.append((pod, "m", [ev]))
    gpu.apply_event_batches(batches, tp)
    torch.cuda.synchronize()
    spy = _SpyOps(gpu.table.ops)
    gpu.table.ops = spy
    ixs = {mode: Indexer(Config(token_processor=TokenProcessorConfig(
        block_size=bs, hash_algo=algo), device_chain=mode, **cfg_kw),
        kv_block_index=gpu) for mode in ("off", "on")}
    off = np.zeros(len(prompts) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in prompts])
    flat = np.asarray([t for p in prompts for t in p], dtype=np.int64)
    return gpu, spy, ixs, torch.from_numpy(flat), torch.from_numpy(off)


def _both(spy, ixs, flat, off, pods=()):
    before = spy.device_calls
    want = ixs["off"].score_flat_tokens(flat, off, "m", list(pods))
    assert spy.device_calls == before
    got = ixs["on"].score_flat_tokens(flat, off, "m", list(pods))
    return got, want, spy.device_calls - before


@pytest.mark.parametrize("algo", ALGOS)
def test_route_on_equals_off(algo):
    gpu, spy, ixs, flat, off = _world(algo=algo)
    got, want, calls = _both(spy, ixs, flat, off)
    assert calls == 1 and got.is_cuda
    assert torch.equal(got, want)
    want = want.cpu()
    assert tuple(want.shape) == (7, gpu._num_pods_padded())
    # the 1040-token prompt hits on all 65 keys (0.8 is not exact in
    # float32, so its sum of 65 is a little under 52)
    assert want[5].max().item() >= 65 * 0.79
    assert want[0].abs().sum().item() == 0
    # and with a pod filter
    got, want, calls = _both(spy, ixs, flat, off, pods=["pod-0", "pod-3"])
    assert calls == 1
    assert torch.equal(got, want)
    assert want.cpu()[:, [1, 2, 4, 5]].abs().sum().item() == 0


def test_route_lds_overflow_fallback():
    # 1100 chunks x 4 tiers x 5 pod words x 8 B > 64 KB of masks
    gpu, spy, ixs, flat, off = _world(
        bs=4, n_pods=260, tiers=["gpu", "cpu", "disk", "remote"],
        lens=[0, 4400, 13, 4 * 200, 0])
    assert gpu._num_pods_padded() == 320
    assert len(gpu.registry.id_to_tier) == 4
    got, want, calls = _both(spy, ixs, flat, off)
    assert calls == 1
    assert torch.equal(got, want)
    assert want.cpu()[1].max().item() >= 1100 * 0.3


def test_route_image_over_cap_takes_cpu_chain():
    gpu, spy, ixs, flat, off = _world(device_chain_max_image_bytes=1024)
    got, want, calls = _both(spy, ixs, flat, off)
    assert calls == 0
    assert torch.equal(got, want)


def test_route_block_size_24_takes_cpu_chain():
    gpu, spy, ixs, flat, off = _world(bs=24, lens=[0, 24 * 5 + 3, 23, 24, 0])
    got, want, calls = _both(spy, ixs, flat, off)
    assert calls == 0
    assert torch.equal(got, want)
    assert want.cpu()[1].max().item() > 0


def test_route_empty_batches():
    gpu, spy, ixs, flat, off = _world()
    P = gpu._num_pods_padded()
    none = torch.zeros(0, dtype=torch.int64)
    for ix in ixs.values():
        s = ix.score_flat_tokens(none, torch.zeros(1, dtype=torch.int64),
                                 "m", [])
        assert tuple(s.shape) == (0, P)
        # all prompts shorter than a chunk (or empty)
        s = ix.score_flat_tokens(torch.arange(20, dtype=torch.int64),
                                 torch.tensor([0, 0, 15, 20, 20]), "m", [])
        assert tuple(s.shape) == (4, P) and s.abs().sum().item() == 0
    # the op itself, called directly
    ops = gpu.table.ops
    w = gpu.tier_weights()
    f = gpu._filter_tensor(set(), P)
    for toks, offs, B in ((none, [0], 0),
                          (torch.arange(20, dtype=torch.int64),
                           [0, 0, 15, 20, 20], 4)):
        s = ops.gpu_score_flat_tokens(
            *gpu.table._t(), toks, torch.tensor(offs, dtype=torch.int64), 0,
            f, w, P, gpu.table.next_epoch(), 0, 16, 2, 0)
        assert s.is_cuda and tuple(s.shape) == (B, P)
        assert s.abs().sum().item() == 0


def test_wire_service_passes_the_route_per_batch():
    """The wire front's batch callback (no sockets opened) hands
    wire_score_flat the route of plan_read_route."""
    from llmd_kvcache_amd.service.wirefront import WireIndexerService

    gpu, spy, ixs, flat, off = _world()
    out = {}
    for mode in ("off", "on"):
        svc = WireIndexerService(ixs[mode])
        before = spy.device_calls
        assert svc._device_chain(gpu, off, 16) == (1 if mode == "on" else 0)
        scores, pods = svc._score_tokens_cb("m", ["pod-1", "pod-2"], flat,
                                            off)
        assert spy.device_calls == before  # the op is called from C++
        assert pods == [f"pod-{i}" for i in range(6)]
        out[mode] = scores
    assert out["off"].abs().sum().item() > 0
    assert torch.equal(out["on"], out["off"])


@pytest.mark.parametrize("algo", ALGOS)
def test_wire_score_flat_device_chain(algo):
    gpu, spy, ixs, flat, off = _world(algo=algo)
    tp = ixs["on"].tokens_processor
    P = gpu._num_pods_padded()
    args = (flat, off, gpu.registry.model_id("m"),
            gpu._filter_tensor({"pod-1", "pod-4"}, P), gpu.tier_weights(), P)
    tail = (_to_i64(tp.config.init_hash()), 16,
            len(gpu.registry.id_to_tier), hashing.NATIVE_ALGO_IDS[algo])
    ops = gpu.table.ops
    want = ops.wire_score_flat(*gpu.table._t(), *args,
                               gpu.table.next_epoch(), *tail)
    same = ops.wire_score_flat(*gpu.table._t(), *args,
                               gpu.table.next_epoch(), *tail, 0)
    got = ops.wire_score_flat(*gpu.table._t(), *args,
                              gpu.table.next_epoch(), *tail, device_chain=1)
    assert not got.is_cuda and not want.is_cuda
    assert want.abs().sum().item() > 0
    assert torch.equal(same, want)
    assert torch.equal(got, want)
