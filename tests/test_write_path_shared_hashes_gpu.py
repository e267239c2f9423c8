"""GPU write path with engine hashes shared across pods and models: the
scenarios of write_path_cases.py through GpuIndex.apply_event_batches
against the sequential model, and the engine map's (hash, model) scoping
through the direct ops (k_insert, k_get_request_keys, k_evict,
k_compact_emap).  All tests require an MI355X."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex, GpuIndexConfig)
from llmd_kvcache_amd.kvblock.keys import Key, PodEntry  # noqa: E402
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    ChunkedTokenDatabase, TokenProcessorConfig)
from tests.test_sha_chain_gpu import _OpsSpy  # noqa: E402
from tests.write_path_cases import (  # noqa: E402
    BS, CAPACITY, MODEL_A, MODEL_B, PODS_PER_KEY, SCENARIO_IDS, SCENARIOS,
    SequentialModel, assert_index_matches)

POD_A, POD_B = PodEntry("pod-a", "gpu"), PodEntry("pod-b", "gpu")
ORDERS = {"a-then-b": ((MODEL_A, 70, POD_A), (MODEL_B, 71, POD_B)),
          "b-then-a": ((MODEL_B, 71, POD_B), (MODEL_A, 70, POD_A))}
orders = pytest.mark.parametrize("order", list(ORDERS))


def new_index():
    return GpuIndex(GpuIndexConfig(capacity=CAPACITY,
                                   pods_per_key=PODS_PER_KEY))


@pytest.mark.parametrize("scenario", SCENARIOS, ids=SCENARIO_IDS)
def test_scenario_matches_sequential_model(scenario):
    tp = ChunkedTokenDatabase(TokenProcessorConfig(block_size=BS,
                                                   hash_algo=scenario.algo))
    gpu = new_index()
    spy = gpu.table.ops = _OpsSpy(gpu.table.ops)
    model = SequentialModel(scenario.algo, tp.config.init_hash())
    for b, burst in enumerate(scenario.bursts):
        gpu.apply_event_batches(burst.groups, tp)
        torch.cuda.synchronize()
        assert spy.calls[-1] == burst.route, (scenario.name, b)
        model.apply_burst(burst.groups)
        assert_index_matches(gpu, model, f"{scenario.name} burst {b}")


def add_hash_7_under_both_models(gpu, order):
    """Engine hash 7 -> request key 70 under model-a (pod-a) and -> 71
    under model-b (pod-b), one add each."""
    for model, rh, pod in ORDERS[order]:
        gpu.add([Key(model, 7)], [Key(model, rh)], [pod])
    torch.cuda.synchronize()


def assert_both_models_hold_hash_7(gpu, where):
    for model, rh, pod in ORDERS["a-then-b"]:
        assert gpu.get_request_key(Key(model, 7)) == Key(model, rh), (
            f"{where}: engine hash 7 under {model}")
        rk = Key(model, rh)
        assert gpu.lookup([rk], set()) == {rk: [pod]}, (
            f"{where}: pods of ({model}, {rh})")


@orders
def test_engine_hash_maps_per_model(order):
    gpu = new_index()
    add_hash_7_under_both_models(gpu, order)
    assert_both_models_hold_hash_7(gpu, order)
    gpu.evict(Key(MODEL_B, 7), [POD_B])
    torch.cuda.synchronize()
    rk_a, rk_b = Key(MODEL_A, 70), Key(MODEL_B, 71)
    assert not gpu.lookup([rk_b], set()).get(rk_b), "(model-b, 71) emptied"
    assert gpu.lookup([rk_a], set()) == {rk_a: [POD_A]}, "model-a untouched"
    # neither request key exists under the other model
    assert not gpu.lookup([Key(MODEL_A, 71)], set())
    assert not gpu.lookup([Key(MODEL_B, 70)], set())
    # removals retain both mappings
    assert gpu.get_request_key(Key(MODEL_A, 7)) == rk_a
    assert gpu.get_request_key(Key(MODEL_B, 7)) == rk_b


@orders
def test_compaction_keeps_both_models_mappings(order):
    gpu = new_index()
    add_hash_7_under_both_models(gpu, order)
    gpu.compact()
    torch.cuda.synchronize()
    assert gpu.table.keys.numel() == CAPACITY
    assert_both_models_hold_hash_7(gpu, f"{order}, same capacity")
    gpu.compact(new_capacity=1 << 11)
    torch.cuda.synchronize()
    assert gpu.table.keys.numel() == 1 << 11
    assert_both_models_hold_hash_7(gpu, f"{order}, grown")


def test_duplicate_inserts_converge_per_model():
    """2048 identical (7 -> 70) inserts in one launch under model-a, then
    2048 identical (7 -> 71) under model-b: racers of one (hash, model)
    still end on one slot, and the second launch takes a slot of its own.
    Says nothing about two models racing inside one launch."""
    gpu = new_index()
    n = 2048
    eh = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    for model, rh, pod in ORDERS["a-then-b"]:
        gpu.table.insert(eh, torch.full_like(eh, rh),
                         gpu.registry.model_id(model),
                         gpu._entries_tensor([pod]))
    torch.cuda.synchronize()
    assert_both_models_hold_hash_7(gpu, "2048 duplicates per model")
    e_keys = gpu.table.e_keys.cpu()
    e_meta = gpu.table.e_meta.cpu()
    assert int((e_keys == 7).sum()) == 2, "one engine-map slot per model"
    models = sorted(int(m) & 0xFFFF for m in e_meta[e_keys == 7].tolist())
    assert models == sorted(gpu.registry.model_id(m)
                            for m in (MODEL_A, MODEL_B))
    assert int((gpu.table.keys.cpu() != 0).sum()) == 2
