"""Shared material of the purge-by-pod tests (CPU and GPU files): the
hand-built 64-slot tables with one row per case, a pure-Python model of
the sweep that says what they must look like afterwards, and a builder
of larger random tables for the CPU<->GPU differential."""

import random

import torch

from llmd_kvcache_amd.kvblock.gpu_index import (
    KvTable,
    TableIndexConfig,
    _to_i64,
)

OCC = 0x80000000
TOMB = 0x40000000
TENSORS = ("keys", "meta", "stamp", "pods", "e_keys", "e_meta", "e_vals")

PURGED = (0, 63, 64, 127, 4095)          # word edges and the last id
SURVIVORS = (5, 62, 65, 128, 4094)       # their neighbours stay
HAND_PODS_PER_KEY = (1, 3, 10, 16)


def entry(pid, tier):
    return (tier << 24) | (pid + 1)


def i32(v):
    return v - (1 << 32) if v >= (1 << 31) else v


def purge_words(ids, n_words=None):
    """int64 [W] bitmap tensor selecting these pod ids."""
    W = n_words or (max(ids) // 64 + 1 if ids else 1)
    words = [0] * W
    for pid in ids:
        words[pid // 64] |= 1 << (pid % 64)
    return torch.tensor([_to_i64(w) for w in words], dtype=torch.int64)


def py_purge(meta, pods, P, ids, model_id):
    """The sweep on plain lists of unsigned ints.  Returns (meta, pods,
    entries_cleared, keys_tombstoned)."""
    ids = set(ids)
    meta, pods = list(meta), list(pods)
    entries = keys = 0
    for i, m in enumerate(meta):
        if not m & OCC:
            continue
        if model_id >= 0 and (m & 0xFFFF) != model_id:
            continue
        cleared = left = 0
        for k in range(P):
            e = pods[i * P + k]
            if e and ((e & 0xFFFFFF) - 1) in ids:
                pods[i * P + k] = 0
                cleared += 1
            elif e:
                left += 1
        entries += cleared
        if cleared and not left and not m & TOMB:
            meta[i] = m | TOMB
            keys += 1
    return meta, pods, entries, keys


def hand_rows(P):
    """{slot: (meta, [entries])} - one row per case of the issue; cases
    that need more slots than P has are left out for that P."""
    rows = {}
    # held only by purged pods, tiers 0 and 3 alternating
    rows[0] = (OCC, [entry(p, 3 * (j & 1))
                     for j, p in enumerate(PURGED[:min(P, 5)])])
    if P >= 3:
        # two purged pods in non-adjacent slots and nothing else
        rows[7] = (OCC, [entry(63, 3), 0, entry(64, 0)])
        # one survivor (last slot, tier 3) next to a purged pod
        rows[31] = (OCC, [entry(0, 3)] + [0] * (P - 2) + [entry(5, 3)])
    # already tombstoned, still holding a stale matching entry
    rows[32] = (OCC | TOMB, [entry(127, 0)])
    # another model's row
    rows[40] = (OCC | 1, [entry(4095, 3)])
    # never published (no OCC): not touched whatever it holds
    rows[13] = (0, [entry(0, 0)])
    # survivors only; ids next to every purged bit
    rows[63] = (OCC, [entry(p, 3 * (j & 1))
                      for j, p in enumerate(SURVIVORS[:min(P, 5)])])
    return rows


def hand_table(P, device="cpu"):
    """A 64-slot KvTable holding hand_rows(P)."""
    t = KvTable(TableIndexConfig(capacity=64, pods_per_key=P, device=device))
    meta = [0] * 64
    pods = [0] * (64 * P)
    keys = [0] * 64
    for slot, (m, ents) in hand_rows(P).items():
        meta[slot] = m
        keys[slot] = 1000 + slot
        for k, e in enumerate(ents):
            pods[slot * P + k] = e
    t.keys.copy_(torch.tensor(keys, dtype=torch.int64))
    t.meta.copy_(torch.tensor([i32(m) for m in meta], dtype=torch.int32))
    t.pods.copy_(torch.tensor([i32(e) for e in pods], dtype=torch.int32))
    t.stamp.fill_(7)
    return t


def table_lists(t):
    """(meta, pods) of a table as lists of unsigned ints."""
    meta = [m & 0xFFFFFFFF for m in t.meta.cpu().tolist()]
    pods = [e & 0xFFFFFFFF for e in t.pods.cpu().tolist()]
    return meta, pods


def snapshot(t):
    return {n: getattr(t, n).cpu().clone() for n in TENSORS}


def assert_tables_equal(a, b, what=""):
    for n in TENSORS:
        assert torch.equal(a[n], b[n]), f"{what}: tensor {n} differs"


def check_hand_table(t, ids, model_id):
    """Run purge_pods on a hand table and hold it against py_purge;
    returns (entries, keys) for further assertions."""
    P = t.cfg.pods_per_key
    before = snapshot(t)
    meta, pods = table_lists(t)
    want_meta, want_pods, want_e, want_k = py_purge(meta, pods, P, ids,
                                                    model_id)
    got_e, got_k = t.purge_pods(purge_words(ids), model_id)
    got_meta, got_pods = table_lists(t)
    assert (got_e, got_k) == (want_e, want_k)
    assert got_meta == want_meta
    assert got_pods == want_pods
    after = snapshot(t)
    for n in ("keys", "stamp", "e_keys", "e_meta", "e_vals"):
        assert torch.equal(before[n], after[n]), f"{n} must stay untouched"
    return got_e, got_k


def random_table(capacity, P, n_keys=300, n_pods=130, seed=0):
    """CPU KvTable filled through the insert / evict ops: n_keys keys of
    2 models held by up to min(P, 4) of n_pods pods at tiers 0..3, some
    evicted again so that tombstones (a few with pods nobody cleared)
    exist.  Returns the table."""
    rng = random.Random(seed)
    t = KvTable(TableIndexConfig(capacity=capacity, pods_per_key=P))
    for i in range(n_keys):
        model = i & 1
        h = torch.tensor([_to_i64(rng.getrandbits(64) | 1)],
                         dtype=torch.int64)
        n = rng.randint(1, min(P, 4))
        pids = rng.sample(range(n_pods), n)
        if i % 5 == 0:
            pids[0] = rng.choice((63, 64))
        ents = torch.tensor([i32(entry(p, rng.randrange(4))) for p in pids],
                            dtype=torch.int32)
        t.insert(h, h, model, ents)
        if i % 7 == 0:  # evict everything: tombstone
            t.evict(h, model, ents)
        elif i % 11 == 0:  # evict one pod
            t.evict(h, model, ents[:1])
    # stale entries inside tombstoned rows (what a raced add leaves)
    meta = t.meta.tolist()
    tombs = [i for i, m in enumerate(meta) if (m & 0xFFFFFFFF) & TOMB]
    for i in tombs[::2]:
        t.pods[i * P] = i32(entry(rng.choice((63, 64, 3)), 3))
    return t
