"""The host side of the ragged device chain, without a GPU: the wave plan
(ops.plan_ragged_waves) against numpy, and Config.device_chain_layout
through indexer.plan_read_route.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from llmd_kvcache_amd.config import (  # noqa: E402
    config_from_json,
    config_to_dict,
)
from llmd_kvcache_amd.indexer import Config, plan_read_route  # noqa: E402
from llmd_kvcache_amd.ops import cpu_ext  # noqa: E402

BS = 16
# zero-chunk prompts first, in the middle and last; ties; one long prompt
LENS = [0, 15, 16, 700, 17, 0, 64, 65, 16, 5, 129, 0]
SHAPES = {
    "mixed": lambda B: [LENS[i % len(LENS)] for i in range(B)],
    "equal": lambda B: [48] * B,
    "empty": lambda B: [i % BS for i in range(B)],
}


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_plan_ragged_waves_matches_numpy(shape, B):
    lens = np.asarray(SHAPES[shape](B), dtype=np.int64)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    perm, wave_k, img_off, tile_start, h_off = (
        t.numpy() for t in cpu_ext.require().plan_ragged_waves(
            torch.zeros(int(off[-1]), dtype=torch.int64),
            torch.from_numpy(off), BS))
    nc = lens // BS
    G = (int((nc > 0).sum()) + 63) // 64
    if shape != "mixed":
        assert G == (0 if shape == "empty" else (B + 63) // 64)
    order = np.argsort(-nc, kind="stable")
    want_perm = np.full(64 * G, -1, dtype=np.int32)
    n = min(B, 64 * G)
    want_perm[:n] = order[:n]
    want_k = nc[order[:64 * G:64]]
    assert perm.dtype == np.int32 and np.array_equal(perm, want_perm)
    assert wave_k.dtype == np.int32 and np.array_equal(wave_k, want_k)
    assert (wave_k > 0).all()
    zero = np.zeros(1, dtype=np.int64)
    assert img_off.dtype == np.int64 and np.array_equal(
        img_off, np.concatenate([zero, np.cumsum(want_k * BS * 64)]))
    assert tile_start.dtype == np.int32 and np.array_equal(
        tile_start, np.concatenate([zero, np.cumsum((want_k * BS + 63) // 64)]))
    assert h_off.dtype == np.int32 and np.array_equal(
        h_off, np.concatenate([zero, np.cumsum(nc)]))


# 4 prompts of 4 chunks at block size 16: a padded image of 1024 bytes
OFFSETS = [0, 64, 128, 192, 256]


@pytest.mark.parametrize("layout,cap,mode,device,ragged", [
    ("padded", 1024, "on", True, False),
    ("padded", 1023, "on", False, False),
    ("padded", 1024, "off", False, False),
    ("over_cap", 1024, "on", True, False),
    ("over_cap", 1023, "on", True, True),
    ("over_cap", 1023, "off", False, False),
    ("ragged", 1024, "on", True, True),
    ("ragged", 1023, "on", True, True),
    ("ragged", 1023, "off", False, False),
])
def test_plan_read_route_layouts(layout, cap, mode, device, ragged):
    cfg = Config(device_chain=mode, device_chain_layout=layout,
                 device_chain_max_image_bytes=cap)
    r = plan_read_route(OFFSETS, 16, "fnv-64a", True, cfg)
    assert (r.device, r.ragged, r.image_bytes) == (device, ragged, 1024)
    # what no layout changes: a CPU table, a block size without a kernel,
    # the "auto" threshold
    assert not plan_read_route(OFFSETS, 16, "fnv-64a", False, cfg).device
    assert not plan_read_route([0, 48, 96], 24, "fnv-64a", True, cfg).device
    cfg.device_chain = "auto"
    auto = plan_read_route(OFFSETS, 16, "fnv-64a", True, cfg)
    assert not auto.device and not auto.ragged


def test_layout_field_default_and_json():
    assert Config().device_chain_layout == "padded"
    assert config_to_dict(Config())["device_chain_layout"] == "padded"
    over = config_from_json('{"device_chain_layout": "over_cap"}')
    assert over.device_chain_layout == "over_cap"
