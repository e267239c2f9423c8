"""Shared material of the pod-id remap tests (CPU and GPU files): a
pure-Python model of the sweep, the maps over the purge cases' word-edge
ids, and the hand-table check."""

import random

import torch

from . import pod_purge_cases as pc

N_ALL = 4096
PURGED, SURVIVORS = pc.PURGED, pc.SURVIVORS


def py_remap(meta, pods, P, remap):
    """The sweep on plain lists of unsigned ints.  Returns (meta, pods,
    entries_moved, entries_cleared, keys_tombstoned)."""
    meta, pods = list(meta), list(pods)
    n = len(remap)
    moved = cleared_all = keys = 0
    for i, m in enumerate(meta):
        if not m & pc.OCC:
            continue
        cleared = left = 0
        for k in range(P):
            e = pods[i * P + k]
            if not e:
                continue
            pid = (e & 0xFFFFFF) - 1
            if pid >= n or remap[pid] == pid:
                left += 1
            elif remap[pid] < 0:
                pods[i * P + k] = 0
                cleared += 1
            else:
                pods[i * P + k] = (e & 0xFF000000) | (remap[pid] + 1)
                moved += 1
                left += 1
        cleared_all += cleared
        if cleared and not left and not m & pc.TOMB:
            meta[i] = m | pc.TOMB
            keys += 1
    return meta, pods, moved, cleared_all, keys


def identity(n=N_ALL):
    return list(range(n))


def drop_only(ids=PURGED, n=N_ALL):
    m = identity(n)
    for pid in ids:
        m[pid] = -1
    return m


def compaction(keep=SURVIVORS, n=N_ALL):
    """keep -> 0.. in ascending order, everything else dropped."""
    m = [-1] * n
    for new, old in enumerate(sorted(keep)):
        m[old] = new
    return m


def swap(a=5, b=4094, n=N_ALL):
    m = identity(n)
    m[a], m[b] = b, a
    return m


def cycle3(ids=(5, 65, 4094), n=N_ALL):
    m = identity(n)
    a, b, c = ids
    m[a], m[b], m[c] = b, c, a
    return m


# n = 1: only id 0 is spoken for; it moves to 7 (an id no hand row holds)
N1_MOVE = [7]
N1_DROP = [-1]

HAND_MAPS = {
    "identity": identity(),
    "drop_only": drop_only(),
    "compaction": compaction(),
    "swap": swap(),
    "cycle3": cycle3(),
    "n1_move": N1_MOVE,
    "n1_drop": N1_DROP,
}


def random_injective(n, drop_frac=1 / 3, seed=0):
    """A random injective map over n ids with about drop_frac drops."""
    rng = random.Random(seed)
    targets = list(range(n))
    rng.shuffle(targets)
    return [-1 if rng.random() < drop_frac else targets[i] for i in range(n)]


def hand_table(P, device="cpu"):
    """pod_purge_cases.hand_table plus one row that holds a dropped
    (PURGED) and a moved (SURVIVORS) pod side by side."""
    t = pc.hand_table(P, device)
    if P >= 2:
        slot = 20
        t.meta[slot] = pc.i32(pc.OCC)
        t.keys[slot] = 1000 + slot
        t.pods[slot * P] = pc.i32(pc.entry(63, 2))
        t.pods[slot * P + 1] = pc.i32(pc.entry(62, 1))
    return t


def check_hand_table_remap(t, remap):
    """Run remap_pods on a table and hold it against py_remap; returns
    (moved, cleared, tombstoned)."""
    P = t.cfg.pods_per_key
    before = pc.snapshot(t)
    meta, pods = pc.table_lists(t)
    want_meta, want_pods, *want = py_remap(meta, pods, P, remap)
    got = t.remap_pods(remap)
    got_meta, got_pods = pc.table_lists(t)
    assert got == tuple(want)
    assert got_meta == want_meta
    assert got_pods == want_pods
    after = pc.snapshot(t)
    for n in ("keys", "stamp", "e_keys", "e_meta", "e_vals"):
        assert torch.equal(before[n], after[n]), f"{n} must stay untouched"
    return got
