"""The host side of the wave-tiled ingest chain, without a GPU: the event
plan (ops.plan_event_waves) against numpy, plan_write_route under the
"waves" layout, and TableIndexConfig.event_chain_layout."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.config import index_config_from_dict  # noqa: E402
from llmd_kvcache_amd.kvblock.event_batch import (  # noqa: E402
    flatten_event_batches, plan_write_route)
from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    NativeIndex, Registry, TableIndexConfig)
from llmd_kvcache_amd.kvevents.events import (  # noqa: E402
    BlockRemoved, BlockStored)
from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402

WAVES = "gpu_apply_events_split_waves"


@pytest.mark.parametrize("bs", [4, 128])
def test_plan_event_waves_matches_numpy(bs):
    """70 events: stores of 0..5 chunks (some with spare tokens), a removal
    at 20 and a store with one engine hash too many at 41."""
    E = 70
    chunks = np.arange(E) % 6
    n_tok = chunks * bs + np.arange(E) % 3
    n_eh = np.maximum(chunks, 1)  # a store of no chunk still names a hash
    ev_type = np.zeros(E, dtype=np.uint8)
    ev_type[20], n_tok[20], n_eh[20] = 1, 0, 3
    n_eh[41] = chunks[41] + 1
    tok_off = np.concatenate([[0], np.cumsum(n_tok)]).astype(np.int32)
    eh_off = np.concatenate([[0], np.cumsum(n_eh)]).astype(np.int32)
    perm, wave_k, img_off, tile_start, h_off, n_chunks = (
        t.numpy() for t in cpu_ext.require().plan_event_waves(
            torch.from_numpy(tok_off), torch.from_numpy(eh_off),
            torch.from_numpy(ev_type), bs))
    nc = np.where((ev_type == 0) & (n_tok // bs == n_eh), n_tok // bs, 0)
    assert nc[20] == 0 and nc[41] == 0 and nc[5] == 5
    assert n_chunks.dtype == np.int32 and np.array_equal(n_chunks, nc)
    assert h_off.dtype == np.int32 and np.array_equal(h_off, eh_off)
    live = int((nc > 0).sum())
    G = (live + 63) // 64
    assert G == 1 and live < 64  # the zero-chunk events made no second wave
    order = np.argsort(-nc, kind="stable")
    want_perm = np.full(64 * G, -1, dtype=np.int32)
    want_perm[:min(E, 64 * G)] = order[:64 * G]
    want_k = nc[order[:64 * G:64]]
    assert np.array_equal(perm, want_perm)
    assert np.array_equal(wave_k, want_k)
    zero = np.zeros(1, dtype=np.int64)
    assert img_off.dtype == np.int64 and np.array_equal(
        img_off, np.concatenate([zero, np.cumsum(want_k * bs * 64)]))
    assert np.array_equal(
        tile_start, np.concatenate([zero, np.cumsum((want_k * bs + 63) // 64)]))


def _flat(batches):
    return flatten_event_batches(batches, Registry(["gpu", "cpu"]))


def _store(hashes, parent, bs):
    return BlockStored(hashes, parent, list(range(len(hashes) * bs)), bs)


@pytest.mark.parametrize("bs", [1, 4, 64, 128])
def test_plan_write_route_waves(bs):
    plain = _flat([("pod-a", "m", [_store([1, 2], None, bs),
                                   _store([3], 77, bs), BlockRemoved([9])])])
    route = plan_write_route(plain, bs, layout="waves")
    assert (route.op, route.max_tokens, route.tokens_int32) == (WAVES, 0, True)
    # the default layout routes as ever
    today = plan_write_route(plain, bs)
    assert today == plan_write_route(plain, bs, layout="rect")
    assert today.op == ("gpu_apply_events_split_tr" if bs <= 64
                        else "gpu_apply_events_split")
    assert today.max_tokens == (2 * bs if bs <= 64 else 0)
    # a batch-local parent and a store+remove conflict keep their kernels
    local = _flat([("pod-a", "m", [_store([1, 2], None, bs),
                                   _store([3], 2, bs)])])
    both = _flat([("pod-a", "m", [_store([1, 2], None, bs),
                                  BlockRemoved([2])])])
    for layout in ("rect", "waves"):
        assert plan_write_route(local, bs, layout).op == \
            "gpu_apply_events_split"
        assert plan_write_route(both, bs, layout).op == "gpu_apply_events"
    # past the stream kernels' block sizes nothing changes either
    assert plan_write_route(plain, 65536, layout="waves").op == \
        "gpu_apply_events_split"


def test_event_chain_layout_config():
    assert TableIndexConfig().event_chain_layout == "rect"
    cfg = index_config_from_dict({"native": {"event_chain_layout": "waves"}})
    assert cfg.native.event_chain_layout == "waves"
    assert NativeIndex(cfg.native).cfg.event_chain_layout == "waves"
    with pytest.raises(ValueError):
        TableIndexConfig(event_chain_layout="ragged")
    bad = index_config_from_dict({"native": {"event_chain_layout": "tr"}})
    with pytest.raises(ValueError):
        NativeIndex(bad.native)
    with pytest.raises(ValueError):
        plan_write_route(_flat([("p", "m", [_store([1], None, 4)])]), 4,
                         layout="tr")
