"""gpu_tiled_score[_rows] on MI355X, exactly, against cpu_fused_score on a
CPU copy of the table tensors, gpu_lookup + gpu_score_from_masks, and a
plain Python longest-prefix model in float64.

KT = tiled_score_tile_keys(n_tiers, W); prompts of 0, 1, KT-1, KT, KT+1,
2KT+1, 3KT and 0 keys.  Pods leave at keys 0, KT-1, KT, KT+1, 2KT or never,
in words that move with the prompt so that every wave walks a live word.
Prompt 2 has a stored key with an empty pod row, 3 is hit-miss-hit, 4 misses
at key 0, 5 loses its last pod inside tile 0 while its later keys are stored
under another pod (the touch-only tail), 6 hits on all 3KT keys; where a row
has room one pod sits on two tiers at once."""

import functools
import random

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.kvblock.gpu_index import KvTable, TableIndexConfig  # noqa: E402,E501

MODEL = 3
WEIGHTS = [1.0, 0.8, 0.3, 1.0]
DYADIC = [1.0, 0.5, 0.25, 1.0]
SHAPES = [(64, 1, 10), (200, 2, 10), (320, 4, 10), (1088, 2, 10),
          (2050, 1, 4), (4096, 4, 16)]


def _i64(h):
    return h - (1 << 64) if h >= (1 << 63) else h


@functools.lru_cache(maxsize=None)
def _build(num_pods, n_tiers, ppk):
    """-> table, KT, prompts (lists of hashes), content {hash: [(pod, tier)]}
    of every stored key, pad (a stored key with pods that no prompt holds)."""
    rng = random.Random(num_pods * 100 + n_tiers * 10 + ppk)
    table = KvTable(TableIndexConfig(capacity=1 << 13, pods_per_key=ppk,
                                     device="cuda:0"))
    W = (num_pods + 63) // 64
    KT = table.ops.tiled_score_tile_keys(n_tiers, W)
    drops = [0, KT - 1, KT, KT + 1, 2 * KT, None]
    prompts, content = [], {}
    for pi, K in enumerate([0, 1, KT - 1, KT, KT + 1, 2 * KT + 1, 3 * KT, 0]):
        keys = [rng.randrange(1, 2**64) for _ in range(K)]
        prompts.append(keys)
        m = min(ppk, num_pods)
        members = {}  # pod -> key at which it leaves
        for j in range(m):
            word = (j * W // m + j + pi) % W
            pod = min(word * 64 + (pi * 7 + j * 11) % 64, num_pods - 1)
            if pi % 2 and j == m - 1:
                pod = num_pods - 1  # the last bit of a partial word
            drop = drops[(pi + j) % len(drops)]
            members.setdefault(pod, [0, KT - 1][j % 2] if pi == 5 else drop)
        if pi == 6:
            members[next(iter(members))] = None
        late = next(p for p in range(num_pods) if p not in members)
        for k, h in enumerate(keys):
            if (pi, k) in ((3, 2), (4, 0)):
                continue  # not stored
            row = [(pod, (pod + k) % n_tiers) for pod, drop in members.items()
                   if (drop is None or k < drop) and (pi, k) != (2, 5)]
            if row and len(row) < ppk and n_tiers > 1 and k % 5 == 0:
                row.append((row[-1][0], (row[-1][1] + 1) % n_tiers))
            if pi == 5 and k >= KT:
                row.append((late, 0))
            content[h] = row
    pad = rng.randrange(1, 2**64)
    content[pad] = [(0, 0), (num_pods - 1, 0)]
    by_row = {}
    for h, row in content.items():
        by_row.setdefault(tuple((t << 24) | (p + 1) for p, t in row),
                          []).append(_i64(h))
    for row, hs in by_row.items():
        ht = torch.tensor(hs, dtype=torch.int64, device="cuda")
        table.insert(ht, ht, MODEL,
                     torch.tensor(row, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    return table, KT, prompts, content, pad


def _cpu_copy(table):
    return [t.cpu().clone() if torch.is_tensor(t) else t for t in table._t()]


def _batch(num_pods, prompts, pad):
    """-> flat hashes, offsets, counts, padded rows, [no filter, filter]."""
    flat = torch.tensor([_i64(h) for p in prompts for h in p],
                        dtype=torch.int64)
    counts = torch.tensor([len(p) for p in prompts], dtype=torch.int32)
    offsets = torch.zeros(len(prompts) + 1, dtype=torch.int32)
    offsets[1:] = torch.cumsum(counts, 0)
    rows = torch.full((len(prompts), max(counts).item() + 3), _i64(pad))
    for b, p in enumerate(prompts):
        rows[b, :len(p)] = flat[offsets[b]:offsets[b + 1]]
    allow = [0] * ((num_pods + 63) // 64)
    for p in range(num_pods):
        if p % 3 != 1:
            allow[p // 64] |= 1 << (p % 64)
    filters = [torch.zeros(0, dtype=torch.int64),
               torch.tensor([_i64(a) for a in allow], dtype=torch.int64)]
    return flat, offsets, counts, rows, filters


@pytest.mark.parametrize("num_pods,n_tiers,ppk", SHAPES)
def test_tiled_score_matches_cpu_and_mask_walk(num_pods, n_tiers, ppk):
    table, KT, prompts, content, pad = _build(num_pods, n_tiers, ppk)
    ops = table.ops
    flat, offsets, counts, rows, filters = _batch(num_pods, prompts, pad)
    weights = torch.tensor(WEIGHTS)
    cpu_t = _cpu_copy(table)
    slot_of = {k: i for i, k in enumerate(cpu_t[0].tolist()) if k != 0}
    hit = torch.tensor(sorted(slot_of[h] for h in set(flat.tolist())
                              if h in slot_of and h != _i64(pad)))
    assert len(hit) == len(flat) - 2  # all but the two keys not stored
    epoch = table.next_epoch() + 1_000_000
    for filt in filters:
        tail = (MODEL, filt.cuda(), weights.cuda(), num_pods)
        for rows_op in (False, True):
            epoch += 1
            expect = table.stamp.cpu().clone()
            expect[hit] = epoch
            if rows_op:
                got = ops.gpu_tiled_score_rows(
                    *table._t(), rows.cuda(), counts.cuda(), *tail, epoch,
                    3 * KT, n_tiers).cpu()
            else:
                got = ops.gpu_tiled_score(
                    *table._t(), flat.cuda(), offsets.cuda(), *tail, epoch,
                    3 * KT, n_tiers).cpu()
            # every stored key that was probed carries the call's epoch,
            # those behind the break too; the padding was never read
            assert torch.equal(table.stamp.cpu(), expect)
            want = ops.cpu_fused_score(*cpu_t, flat, counts, MODEL, filt,
                                       weights, num_pods, epoch)
            _, masks = ops.gpu_lookup(*table._t(), flat.cuda(), *tail[:2],
                                      num_pods, epoch, 0, 1, n_tiers)
            walk = ops.gpu_score_from_masks(masks.contiguous(), offsets.cuda(),
                                            weights.cuda(), num_pods)
            assert tuple(got.shape) == (len(prompts), num_pods)
            assert torch.equal(got, want)
            assert torch.equal(got, walk.cpu())
        if filt.numel() == 0:  # the cases are really in there
            assert got[6].max().item() > (3 * KT - 1) * min(WEIGHTS[:n_tiers])
            assert got[[0, 4, 7]].abs().sum().item() == 0
            assert 0 < got[3].max().item() <= 2.0
            assert 0 < got[2].max().item() <= 5.0
            assert 0 < got[5].max().item() <= KT - 1


@pytest.mark.parametrize("num_pods,n_tiers,ppk", SHAPES)
def test_tiled_score_matches_python_model(num_pods, n_tiers, ppk):
    """Dyadic weights: every sum is exact in float32 and in float64."""
    table, KT, prompts, content, pad = _build(num_pods, n_tiers, ppk)
    flat, offsets, counts, rows, filters = _batch(num_pods, prompts, pad)
    for filt in filters:
        got = table.ops.gpu_tiled_score(
            *table._t(), flat.cuda(), offsets.cuda(), MODEL, filt.cuda(),
            torch.tensor(DYADIC).cuda(), num_pods, table.next_epoch(), 3 * KT,
            n_tiers).cpu().double()
        want = torch.zeros(len(prompts), num_pods, dtype=torch.float64)
        for b, keys in enumerate(prompts):
            active = None
            for h in keys:
                best = {}  # pod -> its best tier weight at this key
                for pod, tier in content.get(h, []):
                    if filt.numel() == 0 or pod % 3 != 1:
                        best[pod] = max(best.get(pod, 0.0), DYADIC[tier])
                active = set(best) if active is None else active & set(best)
                if not active:
                    break
                for pod in active:
                    want[b, pod] += best[pod]
        assert torch.equal(got, want)
