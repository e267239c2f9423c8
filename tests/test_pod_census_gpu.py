"""Pod census on the GPU: k_pod_census + k_census_reduce against the plain
torch count of the same tensors (exact equality, the cases and reference
of test_pod_census), and GpuIndex.pod_census against NativeIndex fed the
same events."""

import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(cpu_ext.maybe_load() is None,
                       reason="native extension not built"),
]

from llmd_kvcache_amd.kvblock.gpu_index import (  # noqa: E402
    GpuIndex,
    GpuIndexConfig,
    NativeIndex,
    TableIndexConfig,
)
from llmd_kvcache_amd.kvblock.token_processor import (  # noqa: E402
    ChunkedTokenDatabase,
    TokenProcessorConfig,
)
from llmd_kvcache_amd.kvevents.events import (  # noqa: E402
    BlockRemoved,
    BlockStored,
)
from llmd_kvcache_amd.kvevents.pool import digest_events  # noqa: E402

from .test_pod_census import CASES, check_case  # noqa: E402


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_gpu_op_equals_plain_count(case):
    check_case("cuda:0", *case)


def test_gpu_index_census_equals_native():
    tp = ChunkedTokenDatabase(TokenProcessorConfig(block_size=4))
    cfg = dict(capacity=1 << 12, pods_per_key=10, tier_names=["gpu", "cpu"])
    gpu = GpuIndex(GpuIndexConfig(**cfg))
    cpu = NativeIndex(TableIndexConfig(**cfg))
    toks = lambda base, n: list(range(base, base + 4 * n))  # noqa: E731
    # pod i: chain c = i % 3 (engine hashes 100 * (c + 1) + ...), 1 + i % 5
    # blocks of it
    batches = [
        (f"p{i}", ("m", "other")[i % 2],
         [BlockStored([100 * (i % 3 + 1) + j for j in range(1 + i % 5)],
                      None, toks(1000 * (i % 3), 1 + i % 5), 4,
                      medium=("gpu", "cpu")[i % 3 == 0])])
        for i in range(12)]
    # p7 alone holds the third block of chain 1 under "other": a tombstone
    batches.append(("p7", "other", [BlockRemoved([202], medium="gpu")]))
    for idx in (gpu, cpu):
        idx.registry.pod_id("idle")
    gpu.apply_event_batches(batches, tp)
    for pod, model, events in batches:
        digest_events(cpu, tp, pod, model, events)
    for model in (None, "m", "other", "nobody"):
        got, want = gpu.pod_census(model), cpu.pod_census(model)
        print(model, got)
        assert got == want
    assert got["pods"]["idle"] == {"gpu": 0, "cpu": 0}
    assert want["tables"][0]["keys_live"] == 0  # "nobody"
    everything = gpu.pod_census()
    assert everything["tables"][0]["entries"] == sum(
        n for tiers in everything["pods"].values() for n in tiers.values()) > 0
    assert everything["tables"][0]["keys_tombstoned"] > 0
