"""gpu_fused_score on MI355X, exactly (torch.equal), against the two other
implementations of the same scoring: cpu_fused_score on a CPU copy of the
table tensors (sequential per-key adds in key order) and gpu_lookup +
gpu_score_from_masks.

One batch mixes prompts of 0, 1, 63, 64, 65, 129 and 512 keys - lengths
around the 64 lanes of the wave that walks a prompt's keys and around
the 256 threads that probe them - with an empty prompt first and last.
Inside the prompts: pods that drop out at keys 0, 63, 64 and 65 and pods
that never do (all keys hit), a
miss at key 0, hit-miss-hit, a key that is present with an empty pod row,
tiers that change from key to key and one pod on two tiers at once (the
per-key maximum over tier weights 1.0 / 0.8 / 0.3, none of whose sums is
exact in binary)."""

import random

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    KvTable,
    TableIndexConfig,
)

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


@pytest.mark.parametrize("num_pods,n_tiers,ppk", [
    (64, 1, 10),   # the benchmark's shape
    (1, 1, 1),
    (64, 2, 4),
    (65, 3, 16),
    (200, 2, 10),
    (200, 3, 16),
    (65, 1, 4),
    (200, 1, 1),
])
def test_fused_score_matches_cpu_and_mask_walk(num_pods, n_tiers, ppk):
    table, prompts, stored = _build(num_pods, n_tiers, ppk,
                                    seed=num_pods * 100 + n_tiers * 10 + ppk)
    ops = table.ops
    W = (num_pods + 63) // 64
    flat = [h for p in prompts for h in p]
    hashes = torch.tensor([_i64(h) for h in flat], dtype=torch.int64,
                          device="cuda")
    counts = torch.tensor([len(p) for p in prompts], dtype=torch.int32)
    offsets = torch.zeros(len(prompts) + 1, dtype=torch.int32)
    offsets[1:] = torch.cumsum(counts, 0)
    offsets = offsets.cuda()
    weights = torch.tensor(WEIGHTS, dtype=torch.float32, device="cuda")
    allow = [0] * W
    for p in range(num_pods):
        if p % 3 != 1:
            allow[p // 64] |= 1 << (p % 64)
    filters = [torch.zeros(0, dtype=torch.int64, device="cuda"),
               torch.tensor([_i64(a) for a in allow], dtype=torch.int64,
                            device="cuda")]
    torch.cuda.synchronize()
    cpu_t = [t.cpu().clone() if torch.is_tensor(t) else t
             for t in table._t()]
    stamp_before = table.stamp.cpu().clone()

    for call, filt in enumerate(filters):
        epoch = CALL_EPOCH + call
        got = ops.gpu_fused_score(*table._t(), hashes, offsets, MODEL, filt,
                                  weights, num_pods, epoch, max(KS), n_tiers)
        want_cpu = ops.cpu_fused_score(*cpu_t, hashes.cpu(), counts, MODEL,
                                       filt.cpu(), weights.cpu(), num_pods,
                                       epoch)
        found, masks = ops.gpu_lookup(*table._t(), hashes, MODEL, filt,
                                      num_pods, epoch, 0, 1, n_tiers)
        want_walk = ops.gpu_score_from_masks(masks.contiguous(), offsets,
                                             weights, num_pods)
        got = got.cpu()
        assert tuple(got.shape) == (len(prompts), num_pods)
        assert torch.equal(got, want_cpu)
        assert torch.equal(got, want_walk.cpu())
        # the cases are really in there: something scores, the all-hit
        # prompt scores every key, the empty and miss-at-0 prompts nothing
        if call == 0:
            assert got[6].max().item() > 500 * min(WEIGHTS[:n_tiers])
            assert got[0].abs().sum().item() == 0
            assert got[5].abs().sum().item() == 0
            assert got[7].abs().sum().item() == 0
            assert 0 < got[4].max().item() <= 2.0

    # every slot that was hit carries the (last) call's epoch, no other
    # slot changed
    keys_cpu = cpu_t[0].tolist()
    slot_of = {k: i for i, k in enumerate(keys_cpu) if k != 0}
    probed = set(flat)
    hit_slots = sorted(slot_of[_i64(h)] for h in stored if h in probed)
    assert len(hit_slots) == len([h for h in stored if h in probed])
    stamp_after = table.stamp.cpu()
    expect = stamp_before.clone()
    expect[torch.tensor(hit_slots, dtype=torch.int64)] = CALL_EPOCH + 1
    assert torch.equal(stamp_after, expect)
