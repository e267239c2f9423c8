"""The write-path scenarios of write_path_cases.py on the CPU: the
scenarios themselves (order independence, the route the planner picks),
the CPU table fed through digest_events against the sequential model, and
InMemoryIndex where the two stances on a removed block's engine mapping
cannot tell them apart."""

import pytest

from llmd_kvcache_amd.kvblock import InMemoryIndex
from llmd_kvcache_amd.kvblock.event_batch import (
    flatten_event_batches, plan_write_route)
from llmd_kvcache_amd.kvblock.gpu_index import (
    NativeIndex, Registry, TableIndexConfig)
from llmd_kvcache_amd.kvblock.token_processor import (
    ChunkedTokenDatabase, TokenProcessorConfig)
from llmd_kvcache_amd.kvevents.pool import digest_events
from tests.write_path_cases import (
    BS, CAPACITY, PODS_PER_KEY, SCENARIO_IDS, SCENARIOS, SequentialModel,
    assert_index_matches, assert_order_independent)

scenarios = pytest.mark.parametrize("scenario", SCENARIOS, ids=SCENARIO_IDS)


def token_processor(scenario):
    return ChunkedTokenDatabase(TokenProcessorConfig(
        block_size=BS, hash_algo=scenario.algo))


def digest_and_compare(index, scenario, retains):
    tp = token_processor(scenario)
    model = SequentialModel(scenario.algo, tp.config.init_hash())
    for b, burst in enumerate(scenario.bursts):
        for pod, model_name, events in burst.groups:
            digest_events(index, tp, pod, model_name, events)
        model.apply_burst(burst.groups)
        assert_index_matches(index, model, f"{scenario.name} burst {b}",
                             retains=retains)


@scenarios
def test_scenario_is_order_independent(scenario):
    assert_order_independent(scenario,
                             token_processor(scenario).config.init_hash())


def test_shapes_stay_small():
    for s in SCENARIOS:
        for burst in s.bursts:
            assert 1 <= len(burst.groups) <= 4
            for _, _, events in burst.groups:
                assert all(len(ev.block_hashes) <= 3 for ev in events)


@scenarios
def test_planner_picks_the_route_the_scenario_names(scenario):
    """A later change of the planner must not move a scenario off the
    kernel it was written for."""
    registry = Registry()
    for b, burst in enumerate(scenario.bursts):
        flat = flatten_event_batches(burst.groups, registry)
        assert flat is not None
        assert len(flat.grp_off) - 1 == len(burst.groups)
        assert plan_write_route(flat, BS).op == burst.route, (scenario.name, b)


@scenarios
def test_cpu_table_matches_model(scenario):
    index = NativeIndex(TableIndexConfig(capacity=CAPACITY,
                                         pods_per_key=PODS_PER_KEY))
    digest_and_compare(index, scenario, retains=True)


@pytest.mark.parametrize(
    "scenario", [s for s in SCENARIOS if s.inmemory_comparable],
    ids=[s.name for s in SCENARIOS if s.inmemory_comparable])
def test_in_memory_index_matches_model(scenario):
    """Only S1, S2, S3 (and S7, S1 again): InMemoryIndex forgets an engine
    hash when its block empties, the model and the table retain it.  In
    these scenarios no event follows a removal, so no parent can name a
    forgotten hash and the difference never reaches a request key or a
    pod set; a forgotten hash may answer None (retains=False), everything
    else must agree.  S4 to S6 remove and go on storing: they are held
    against the backends that share the model's stance."""
    digest_and_compare(InMemoryIndex(), scenario, retains=False)
