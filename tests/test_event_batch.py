"""The write path's host half (kvblock/event_batch.py) and the read
path's staging helpers, without a GPU: what a burst of events flattens
to, which apply kernel a burst is planned for, how token lists pack, and
what TableIndex.score_args stages."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.indexer import pack_token_lists  # noqa: E402
from llmd_kvcache_amd.kvblock.event_batch import (  # noqa: E402
    FIELDS,
    flatten_event_batches,
    plan_write_route,
)
from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    NativeIndex,
    Registry,
    TableIndexConfig,
)
from llmd_kvcache_amd.kvevents.events import (  # noqa: E402
    AllBlocksCleared,
    BlockRemoved,
    BlockStored,
)
from llmd_kvcache_amd.scorer import KVCacheBackendConfig  # noqa: E402
from tests.test_sha_chain_gpu import _route_batches  # noqa: E402
from tests.test_write_path_parity_gpu import route_batches  # noqa: E402

SERIAL = "gpu_apply_events"
SPLIT = "gpu_apply_events_split"
SPLIT_TR = "gpu_apply_events_split_tr"

DTYPES = dict(tokens=np.int64, tok_off=np.int32, ehashes=np.int64,
              eh_off=np.int32, parents=np.int64, has_parent=np.uint8,
              ev_type=np.uint8, pod_entry=np.int32, grp_off=np.int32,
              model_of=np.int32)


def _hand_burst():
    """Two pods, two models, pod-a's two batches merging into one group.
    The registry starts with the tiers gpu (0) and cpu (1)."""
    # 9 bytes: the last 8 count, and they have the top bit set
    wide = b"\xff" + (2**63 + 5).to_bytes(8, "big")
    return [
        ("pod-a", "m1", [
            BlockStored([10, 11], None, list(range(1, 9)), 4),
            AllBlocksCleared(),                                  # skipped
        ]),
        ("pod-b", "m2", [
            BlockStored([20], b"", [1, 2, 3, 4], 4),   # malformed parent
            BlockRemoved([10, 11], medium="disk"),     # fourth tier name
        ]),
        ("pod-a", "m1", [
            BlockStored([12], 11, [9, 10, 11, 12], 4, medium="CPU"),
            BlockStored([], None, [5, 6, 7, 8], 4),    # no hashes
            # bytes among the hashes: the per-element coercion, which
            # also passes over what it cannot read; third tier name
            BlockStored([wide, None, 14], 2**64 - 1, list(range(13, 21)),
                        4, medium="nvme"),
        ]),
        ("pod-b", "m2", [
            BlockRemoved([30], medium="tape"),         # a fifth tier name
            BlockRemoved([12]),                        # default tier
        ]),
    ]


def test_hand_burst_flattens_to_exactly_these_arrays():
    reg = Registry()
    assert reg.id_to_tier == ["gpu", "cpu"]
    flat = flatten_event_batches(_hand_burst(), reg)
    want = dict(
        tokens=list(range(1, 21)),
        tok_off=[0, 8, 12, 20, 20, 20],
        ehashes=[10, 11, 12, -(2**63) + 5, 14, 10, 11, 12],
        eh_off=[0, 2, 3, 5, 7, 8],
        parents=[0, 11, -1, 0, 0],
        has_parent=[0, 1, 1, 0, 0],
        ev_type=[0, 0, 0, 1, 1],
        # (tier << 24) | (pod id + 1)
        pod_entry=[1, (1 << 24) | 1, (2 << 24) | 1, (3 << 24) | 2, 2],
        grp_off=[0, 3, 5],
        model_of=[0, 0, 0, 1, 1],
    )
    assert set(want) == set(FIELDS)
    for name in FIELDS:
        got = getattr(flat, name)
        assert got.dtype == DTYPES[name], name
        assert got.ndim == 1 and got.flags.c_contiguous, name
        assert got.tolist() == want[name], name
    assert flat.ev_of is None
    ev_of = flat.event_of_hash()
    assert ev_of.dtype == np.int32
    assert ev_of.tolist() == [0, 0, 1, 2, 2, 3, 3, 4]
    # groups in first-seen order, and tiers interned group by group
    assert reg.id_to_pod == ["pod-a", "pod-b"]
    assert reg.id_to_model == ["m1", "m2"]
    assert reg.id_to_tier == ["gpu", "cpu", "nvme", "disk"]
    # it stores and removes 10, 11 and 12
    assert plan_write_route(flat, 4).op == SERIAL


def test_burst_with_nothing_left_is_none():
    reg = Registry(["gpu", "cpu", "disk", "nvme"])
    burst = [("pod-a", "m", [AllBlocksCleared(),
                             BlockStored([], None, [1, 2, 3, 4], 4),
                             BlockStored([1], b"", [1, 2, 3, 4], 4)]),
             ("pod-b", "m", [BlockRemoved([1], medium="tape"),
                             BlockRemoved([None])])]
    assert flatten_event_batches(burst, reg) is None
    assert flatten_event_batches([], reg) is None


def _plans(route_list, block_size):
    reg = Registry()
    return [(route, plan_write_route(flatten_event_batches(batches, reg),
                                     block_size))
            for route, batches in route_list]


def test_plans_the_ops_the_gpu_route_tests_assert():
    plans = _plans(_route_batches(16), 16)
    assert [r for r, _ in plans] == [SPLIT_TR, SPLIT, SERIAL]
    plans += _plans(route_batches()[1:], 4)
    for route, plan in plans:
        assert plan.op == route
        assert plan.tokens_int32 == (route == SPLIT_TR)
    # longest event: 4 blocks of 16 tokens, 2 blocks of 4
    assert [p.max_tokens for _, p in plans] == [64, 0, 0, 8, 0, 0]
    seed = _plans(route_batches()[:1], 4)[0][1]
    assert (seed.op, seed.max_tokens) == (SPLIT_TR, 12)


def test_block_size_128_never_plans_the_transposed_route():
    independent = _route_batches(128)[0][1]
    reg = Registry()
    flat = flatten_event_batches(independent, reg)
    assert plan_write_route(flat, 64).op == SPLIT_TR
    plan = plan_write_route(flat, 128)
    assert (plan.op, plan.max_tokens, plan.tokens_int32) == (SPLIT, 0, False)


def test_parent_stored_in_the_same_burst_leaves_the_transposed_route():
    toks = list(range(8))
    own = [("pod-a", "m", [BlockStored([1, 2], None, toks, 4)]),
           ("pod-b", "m", [BlockStored([3, 4], 2, toks, 4)])]
    other = [("pod-a", "m", [BlockStored([1, 2], None, toks, 4)]),
             ("pod-b", "m", [BlockStored([3, 4], 99, toks, 4)])]
    reg = Registry()
    assert plan_write_route(flatten_event_batches(own, reg), 4).op == SPLIT
    assert plan_write_route(flatten_event_batches(other, reg),
                            4).op == SPLIT_TR


def test_store_and_remove_of_one_hash_plans_the_serial_op():
    toks = list(range(8))
    reg = Registry()
    both = [("pod-a", "m", [BlockStored([1, 2], None, toks, 4)]),
            ("pod-b", "m", [BlockRemoved([2])])]
    apart = [("pod-a", "m", [BlockStored([1, 2], None, toks, 4)]),
             ("pod-b", "m", [BlockRemoved([7])])]
    plan = plan_write_route(flatten_event_batches(both, reg), 4)
    assert (plan.op, plan.max_tokens, plan.tokens_int32) == (SERIAL, 0, False)
    assert plan_write_route(flatten_event_batches(apart, reg),
                            4).op == SPLIT_TR


def test_pack_token_lists():
    flat, off = pack_token_lists([])
    assert flat.dtype == off.dtype == torch.int64
    assert (flat.tolist(), off.tolist()) == ([], [0])
    flat, off = pack_token_lists([[7, 8, 9]])
    assert (flat.tolist(), off.tolist()) == ([7, 8, 9], [0, 3])
    flat, off = pack_token_lists([[1, 2], [], (3,), np.arange(4, 8)])
    assert flat.dtype == off.dtype == torch.int64
    assert flat.tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert off.tolist() == [0, 2, 2, 3, 7]


def test_score_args_stages_what_the_call_sites_computed():
    idx = NativeIndex(TableIndexConfig(capacity=1 << 10))
    reg = idx.registry
    for i in range(70):
        reg.pod_id(f"pod-{i}")
    reg.tier_id("disk")
    reg.model_id("other")
    backends = [KVCacheBackendConfig("gpu", 1.0),
                KVCacheBackendConfig("cpu", 0.25),
                KVCacheBackendConfig("disk", 0.125)]
    pods = ["pod-3", "pod-65", "nobody"]

    a = idx.score_args("m", pods, backends)
    assert a.model_id == reg.model_id("m") == 1
    assert a.num_pods == idx._num_pods_padded() == 128
    assert torch.equal(a.filter_words, idx._filter_tensor(set(pods), 128))
    assert a.filter_words.tolist() == [1 << 3, 1 << 1]
    assert torch.equal(a.weights, idx.tier_weights(
        {b.name: b.weight for b in backends}))
    assert a.weights.tolist() == [1.0, 0.25, 0.125, 1.0]
    assert a.n_tiers == max(1, len(reg.id_to_tier)) == 3
    assert tuple(a) == (a.model_id, a.num_pods, a.filter_words, a.weights,
                        a.n_tiers)

    # no backend configs: the default weights; no pods: no filter
    d = idx.score_args("m", set())
    assert torch.equal(d.weights, idx.tier_weights())
    assert d.filter_words.numel() == 0
    # a weight tensor is passed through
    w = torch.ones(4)
    assert idx.score_args("m", pods, weights=w).weights is w
