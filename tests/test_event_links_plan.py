"""The host side of the linked wave ingest, without a GPU: the link plan
against a dict model, the per-level wave plan, plan_write_route under the
"linked" layout and TableIndexConfig.event_link_max_levels."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.config import index_config_from_dict  # noqa: E402
from llmd_kvcache_amd.kvblock.event_batch import (  # noqa: E402
    WriteRoute, flatten_event_batches, plan_write_route)
from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    NativeIndex, Registry, TableIndexConfig)
from llmd_kvcache_amd.kvevents.events import (  # noqa: E402
    BlockRemoved, BlockStored)
from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402

BS = 2
LINKED, WAVES, SPLIT = ("gpu_apply_events_split" + s
                        for s in ("_linked", "_waves", ""))


def _store(hashes, parent, chunks=None):
    n = len(hashes) if chunks is None else chunks
    return BlockStored(hashes, parent, list(range(n * BS + 1)), BS)


def _flat(batches):
    return flatten_event_batches(batches, Registry(["gpu", "cpu"]))


def _burst():
    """Blocks are numbered in event order: event 0 owns 0..2, 1 owns 3..4."""
    a = [
        _store([10, 11, 12], None),   # 0: blocks 0 1 2
        _store([20, 21], 12),         # 1: its parent's last block (2)
        _store([30], 11),             # 2: a middle block (1)
        _store([31], 12),             # 3: second child of block 2
        _store([11, 40], None),       # 4: 11 again, block 7
        _store([41], 11),             # 5: the latest 11: block 7, not 1
        _store([50], 70),             # 6: 70 only in pod-b's group
        _store([51], 60),             # 7: 60 only later in this group
        _store([60], None),           # 8
        _store([61, 62], None, 1),    # 9: dropped, one chunk for two hashes
        _store([63], 61),             # 10: parent in the dropped store
        BlockRemoved([64]),           # 11
        _store([65], 64),             # 12: parent in the removal
        _store([80], 21),             # 13: level 2
        _store([81], 80),             # 14: level 3
        _store([82], 81),             # 15: level 4
    ]
    b = [_store([70, 12], None), _store([71], 12)]  # 16, 17: its own 12
    c = [_store([1000 + 4 * i + j for j in range(1 + i % 3)], None)
         for i in range(70)]  # 18..87: level 0 takes two waves
    return _flat([("pod-a", "m", a), ("pod-b", "m", b), ("pod-c", "m", c)])


def _links(f, bs=BS):
    link, level, n_levels = cpu_ext.require().plan_event_links(
        *(torch.from_numpy(getattr(f, name)) for name in (
            "ehashes", "eh_off", "tok_off", "ev_type", "parents",
            "has_parent", "grp_off")), bs)
    return link, level, int(n_levels)


def _model(f, bs):
    E = len(f.ev_type)
    link, level = [-1] * E, [0] * E
    for g in range(len(f.grp_off) - 1):
        seen = {}  # engine hash -> (its latest block, that block's event)
        for e in range(f.grp_off[g], f.grp_off[g + 1]):
            blocks = range(f.eh_off[e], f.eh_off[e + 1])
            if f.ev_type[e] or (f.tok_off[e + 1] - f.tok_off[e]) // bs != \
                    len(blocks):
                continue
            if f.has_parent[e] and f.parents[e] in seen:
                link[e], src = seen[f.parents[e]]
                level[e] = level[src] + 1
            seen.update((f.ehashes[bi], (bi, e)) for bi in blocks)
    return link, level


def test_plan_event_links_matches_model():
    f = _burst()
    link, level, n_levels = _links(f)
    want_link, want_level = _model(f, BS)
    assert link.tolist() == want_link and level.tolist() == want_level
    assert want_link == [-1, 2, 1, 2, -1, 7, -1, -1, -1, -1, -1, -1, -1,
                         4, 18, 19, -1, 22] + [-1] * 70  # by hand
    assert n_levels == 5 and max(want_level) == want_level[15] == 4


def test_plan_linked_event_waves_properties():
    f = _burst()
    link, level, n_levels = _links(f)
    tok_off, eh_off, ev_type = (torch.from_numpy(getattr(f, n))
                                for n in ("tok_off", "eh_off", "ev_type"))
    ops = cpu_ext.require()
    perm, wave_k, img_off, tile_start, h_off, n_chunks, level_wave, plink = (
        t.numpy() for t in ops.plan_linked_event_waves(
            tok_off, eh_off, ev_type, link, level, BS))
    assert np.array_equal(h_off, f.eh_off) and np.array_equal(plink, link)
    assert sorted(perm[perm >= 0]) == list(np.flatnonzero(n_chunks > 0))
    assert level_wave.tolist() == [0, 2, 3, 4, 5, 6] and len(wave_k) == 6
    for l in range(n_levels):
        seg = perm[64 * level_wave[l]:64 * level_wave[l + 1]]
        lanes = seg[seg >= 0]
        assert len(lanes) and (level.numpy()[lanes] == l).all()
        assert (np.diff(n_chunks[lanes]) <= 0).all()
        assert (seg[len(lanes):] == -1).all()  # padding only at the end
    assert np.array_equal(np.diff(img_off), wave_k * BS * 64)
    bad = link.clone()
    bad[1] = int(f.eh_off[1])
    with pytest.raises(RuntimeError, match="at or past its own event"):
        ops.plan_linked_event_waves(tok_off, eh_off, ev_type, bad, level, BS)


def test_write_route_and_config_linked():
    f = _burst()
    links = _links(f)
    assert plan_write_route(f, BS, "linked", links, link_max_levels=5) == \
        WriteRoute(LINKED, 0, True)
    assert plan_write_route(f, BS, "linked", links, 4).op == SPLIT  # the cap
    assert plan_write_route(f, 65536, "linked", links, 5).op == SPLIT
    # as at the parent commit: without links, and under the other layouts
    assert plan_write_route(f, BS, "linked").op == SPLIT
    for layout in ("rect", "waves"):
        assert plan_write_route(f, BS, layout, links, 5).op == SPLIT
        assert plan_write_route(f, BS, layout) == \
            plan_write_route(f, BS, layout, links, 5)
    plain = _flat([("pod-a", "m", [_store([1, 2], None), _store([3], 77)])])
    assert plan_write_route(plain, BS, "linked", _links(plain), 5).op == WAVES
    both = _flat([("pod-a", "m", [_store([1, 2], None), _store([3], 2),
                                  BlockRemoved([2])])])
    assert plan_write_route(both, BS, "linked", _links(both), 5).op == \
        "gpu_apply_events"
    # the config fields
    assert TableIndexConfig().event_link_max_levels >= 1
    cfg = index_config_from_dict({"native": {
        "event_chain_layout": "linked", "event_link_max_levels": 3}})
    assert cfg.native.event_chain_layout == "linked"
    assert NativeIndex(cfg.native).cfg.event_link_max_levels == 3
