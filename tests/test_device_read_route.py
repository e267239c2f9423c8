"""The read path's route decision (indexer.plan_read_route) and its config
fields, without a GPU: which batches of score_flat_tokens chain on the
device, which stay on the CPU chain, and what the function reports about
a batch (whole chunks per prompt, the longest prompt, the padded image).
"""

import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.config import (  # noqa: E402
    config_from_json,
    config_to_dict,
)
from llmd_kvcache_amd.indexer import (  # noqa: E402
    Config,
    Indexer,
    plan_read_route,
)
from llmd_kvcache_amd.utils import hashing  # noqa: E402

# 4 prompts of 64 tokens = 4 chunks each at block size 16
OFFSETS = [0, 64, 128, 192, 256]


def _cfg(**kw):
    cfg = Config()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_config_fields_and_json_overlay():
    cfg = Config()
    assert cfg.device_chain == "auto"
    assert cfg.device_chain_min_chunks == 8192
    assert cfg.device_chain_max_image_bytes == 1 << 30
    d = config_to_dict(cfg)
    assert {"device_chain", "device_chain_min_chunks",
            "device_chain_max_image_bytes"} <= set(d)
    over = config_from_json(
        '{"device_chain": "on", "device_chain_min_chunks": 4096,'
        ' "device_chain_max_image_bytes": 1048576}')
    assert over.device_chain == "on"
    assert over.device_chain_min_chunks == 4096
    assert over.device_chain_max_image_bytes == 1 << 20


def test_cpu_table_stays_on_cpu_chain_under_on():
    r = plan_read_route(OFFSETS, 16, "fnv-64a", False, _cfg(device_chain="on"))
    assert not r.device


def test_block_size_24_stays_on_cpu_chain():
    off = [0, 48, 96]
    r = plan_read_route(off, 24, "fnv-64a", True, _cfg(device_chain="on"))
    assert not r.device
    assert r.n_chunks == [2, 2] and r.max_k == 2


def test_algo_without_native_id_stays_on_cpu_chain():
    assert "python-only-hash" not in hashing.NATIVE_ALGO_IDS
    r = plan_read_route(OFFSETS, 16, "python-only-hash", True,
                        _cfg(device_chain="on"))
    assert not r.device


def test_image_over_cap_stays_on_cpu_chain():
    # image = 4 prompts * 4 chunks * 16 tokens * 4 bytes = 1024
    on_cap = plan_read_route(OFFSETS, 16, "fnv-64a", True,
                             _cfg(device_chain="on",
                                  device_chain_max_image_bytes=1024))
    assert on_cap.image_bytes == 1024 and on_cap.device
    over = plan_read_route(OFFSETS, 16, "fnv-64a", True,
                           _cfg(device_chain="on",
                                device_chain_max_image_bytes=1023))
    assert over.image_bytes == 1024 and not over.device


def test_auto_threshold():
    below = plan_read_route(OFFSETS, 16, "fnv-64a", True,
                            _cfg(device_chain="auto",
                                 device_chain_min_chunks=17))
    assert not below.device
    at = plan_read_route(OFFSETS, 16, "fnv-64a", True,
                         _cfg(device_chain="auto",
                              device_chain_min_chunks=16))
    assert at.device


@pytest.mark.parametrize("algo", sorted(hashing.NATIVE_ALGO_IDS))
def test_auto_default_threshold(algo):
    cfg = Config()
    floor = cfg.device_chain_min_chunks
    assert floor > 0 and floor & (floor - 1) == 0  # a power of two
    below = plan_read_route([0, (floor - 1) * 16], 16, algo, True, cfg)
    at = plan_read_route([0, 7, floor * 16 + 7], 16, algo, True, cfg)
    assert not below.device and at.device


def test_off_never_and_on_whenever_eligible():
    for algo in hashing.NATIVE_ALGO_IDS:
        for bs in (4, 8, 16, 32, 64):
            on = plan_read_route(OFFSETS, bs, algo, True,
                                 _cfg(device_chain="on"))
            off = plan_read_route(OFFSETS, bs, algo, True,
                                  _cfg(device_chain="off"))
            assert on.device and not off.device
    odd = plan_read_route(OFFSETS, 16, "fnv-64a", True,
                          _cfg(device_chain="sometimes"))
    assert not odd.device


def test_chunk_counts_with_empty_prompts_and_remainders():
    # lengths 0, 15, 16, 17, 0, 100, 0
    lens = [0, 15, 16, 17, 0, 100, 0]
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    for src in (off, torch.tensor(off, dtype=torch.int64)):
        r = plan_read_route(src, 16, "fnv-64a", True, _cfg(device_chain="on"))
        assert r.n_chunks == [0, 0, 1, 1, 0, 6, 0]
        assert r.max_k == 6
        assert r.image_bytes == 7 * 6 * 16 * 4
    empty = plan_read_route([0], 16, "fnv-64a", True, _cfg(device_chain="on"))
    assert empty.n_chunks == [] and empty.max_k == 0
    assert empty.image_bytes == 0


def test_native_index_scores_equal_under_on_and_off():
    from llmd_kvcache_amd.kvblock.gpu_index import (
        NativeIndex,
        TableIndexConfig,
    )
    from llmd_kvcache_amd.kvblock.keys import PodEntry
    from llmd_kvcache_amd.kvblock.token_processor import (
        ChunkedTokenDatabase,
        TokenProcessorConfig,
    )

    def run(mode):
        cfg = Config(token_processor=TokenProcessorConfig(block_size=4),
                     device_chain=mode)
        idx = NativeIndex(TableIndexConfig(capacity=1 << 12, pods_per_key=4))
        indexer = Indexer(cfg, kv_block_index=idx)
        tp = ChunkedTokenDatabase(cfg.token_processor)
        a = list(range(40))
        b = list(range(100, 123))
        idx.add(*[tp.tokens_to_kv_block_keys(None, a, "m")] * 2,
                [PodEntry("pod-a", "gpu")])
        idx.add(*[tp.tokens_to_kv_block_keys(None, b[:12], "m")] * 2,
                [PodEntry("pod-b", "gpu")])
        flat = torch.tensor(a + b + [7, 8], dtype=torch.int64)
        off = torch.tensor([0, 40, 40, 63, 65], dtype=torch.int64)
        return indexer.score_flat_tokens(flat, off, "m", [])

    off, on = run("off"), run("on")
    assert tuple(off.shape)[0] == 4
    assert off[0].max().item() == 10.0 and off[2].max().item() == 3.0
    assert off[1].abs().sum().item() == 0
    assert torch.equal(on, off)
