"""select_sort_kernel's two sort keys (option "sort_key"): one exact 32-bit word per entry where a tile's depth range fits it
and no two entries share a depth ("narrow" = "auto"), the 64-bit (depth bits, id) key otherwise and under "wide". Both build the
same lists, so frames and every gradient are equal BIT FOR BIT, and the counter sort_wide_tiles says which path a tile took.

Scenes are built by hand: a 64 x 64 image, the camera at the origin looking down +z (the view depth IS the z that was set, bit for
bit), K small isotropic Gaussians whose centres -- and whole footprints -- lie inside one 8 x 8 tile, opacities near 0.5 and
distinct colours, so an entry out of order changes bits of the frame."""
import math

import numpy as np
import pytest
import torch

from sfgs.camera import fovy_from_fovx, make_frame
from sfgs.synth import upstream_grads
from test_gpu_raster import run_hip

pytestmark = pytest.mark.gpu

W = H = 64
FOVX = math.radians(60.0)
SIGMA_PX = 0.45     # 3 sigma (+ the 0.1 px^2 mip filter) < 1.5 px: centres 2.5 px inside a tile keep the footprint inside it


def _frame():
    return make_frame(np.eye(3), np.zeros(3), FOVX, fovy_from_fovx(FOVX, W, H), W, H)


def _scene(groups, seed=3):
    """groups: [((tile x, tile y), depths)]; Gaussian ids follow the order given."""
    frame = _frame()
    rng = np.random.default_rng(seed)
    tiles = np.concatenate([np.tile(np.asarray(t, np.float64), (len(z), 1)) for t, z in groups])
    z = np.concatenate([np.asarray(z, np.float32) for _, z in groups]).astype(np.float32)
    n = len(z)
    pix = tiles * 8.0 + 2.5 + 3.0 * rng.random((n, 2))            # centre, in pixels: inside the tile's inner 3 x 3
    focal = W / (2.0 * frame["tanfovx"])
    zd = z.astype(np.float64)
    x = ((2.0 * pix[:, 0] + 1.0) / W - 1.0) * frame["tanfovx"] * zd
    y = ((2.0 * pix[:, 1] + 1.0) / H - 1.0) * frame["tanfovy"] * zd
    means = np.stack([x, y, zd], 1).astype(np.float32)
    means[:, 2] = z                                                # the depth bits exactly as asked for
    s = (SIGMA_PX * zd / focal).astype(np.float32)
    g = dict(means3D=torch.from_numpy(means), scales=torch.from_numpy(np.repeat(s[:, None], 3, 1).copy()),
             rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1).contiguous(),
             opacities=torch.from_numpy((0.45 + 0.1 * rng.random((n, 1))).astype(np.float32)),
             colors_precomp=torch.from_numpy(rng.random((n, 3)).astype(np.float32)), shs=None)
    return frame, g


def _distinct_depths(k, lo=250.0, hi=350.0, seed=1):
    z = np.linspace(lo, hi, k, dtype=np.float32) if k > 1 else np.asarray([lo], np.float32)
    assert len(np.unique(z.view(np.uint32))) == k
    return np.random.default_rng(seed).permutation(z)


def _wide_vs_narrow(frame, g, sfgs_option, sort="fused"):
    gc, gd = upstream_grads(W, H, 2)
    sfgs_option("sort", sort)
    sfgs_option("sort_key", "wide")
    a = run_hip(frame, g, gc, gd)
    sfgs_option("sort_key", "narrow")
    b = run_hip(frame, g, gc, gd)
    for k in ("color", "depth", "alpha", "radii"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["grads"].keys() == b["grads"].keys()
    for k in a["grads"]:
        np.testing.assert_array_equal(a["grads"][k], b["grads"][k], err_msg=k)
    assert a["counters"]["max_tile_list"] == b["counters"]["max_tile_list"]
    assert (a["color"] > 0).any()
    return a["counters"], b["counters"]


@pytest.mark.parametrize("K", [1, 63, 64, 65, 128, 129, 255, 256, 257, 511, 512])
def test_network_sizes_and_padding(K, sfgs_option):
    """every network size, full and partial last lanes, lists that end on and next to a size boundary"""
    frame, g = _scene([((3, 2), _distinct_depths(K))])
    wide, narrow = _wide_vs_narrow(frame, g, sfgs_option)
    assert narrow["max_tile_list"] == K
    assert narrow["sort_wide_tiles"] == 0
    assert wide["sort_wide_tiles"] == 1      # "wide" sorts the scene's one tile on the 64-bit key


def test_list_beyond_the_kernel_goes_to_the_long_list_kernels(sfgs_option):
    frame, g = _scene([((3, 2), _distinct_depths(513))])
    wide, narrow = _wide_vs_narrow(frame, g, sfgs_option, sort="fused")
    assert narrow["max_tile_list"] == 513
    assert narrow["sort_wide_tiles"] == 0 and wide["sort_wide_tiles"] == 0    # not sorted inside select_sort at all


@pytest.mark.parametrize("K", [700, 1000])
@pytest.mark.parametrize("sort", ["fused768", "fused1024"])
def test_ten_position_bits(sort, K, sfgs_option):
    """the 768- and 1 024-entry forms of the kernel: 10 position bits, the 16-key network beyond 512 entries (1 000 entries go
    to the long-list kernels under fused768)"""
    frame, g = _scene([((3, 2), _distinct_depths(K))])
    wide, narrow = _wide_vs_narrow(frame, g, sfgs_option, sort=sort)
    assert narrow["max_tile_list"] == K
    assert narrow["sort_wide_tiles"] == 0
    assert wide["sort_wide_tiles"] == (1 if K <= int(sort[5:]) else 0)


@pytest.mark.parametrize("first", [0, 3, 2], ids=["in_lane_0_1", "across_lanes_3_4", "triple_2_3_4"])
@pytest.mark.parametrize("others", [100, 200], ids=["net128", "net256"])
def test_equal_depths_fall_back_to_depth_id_order(others, first, sfgs_option):
    """two (three) Gaussians of identical z, different ids and colours, at the sorted positions first, first + 1 (, + 2) -- the
    nearest entries of the tile, so all of them are composited: neighbours inside one lane's registers (positions 0 / 1) or on
    both sides of a lane boundary (3 / 4: lanes hold 2 entries each in the 128-entry network, 4 in the 256-entry one)"""
    n_tied = 3 if first == 2 else 2
    z = _distinct_depths(others + 1)                  # one value more: the tied depth
    z_sorted = np.sort(z)
    tied = z_sorted[first]
    rest = np.delete(z_sorted, first)
    rest = np.random.default_rng(4).permutation(rest)
    # the tied Gaussians far apart in id order, the later id first in nothing: only (depth, id) decides
    depths = np.concatenate([[tied], rest[: others // 2], [tied] * (n_tied - 1), rest[others // 2:]]).astype(np.float32)
    assert (np.sort(depths)[first:first + n_tied] == tied).all() and len(np.unique(depths)) == others + 1
    frame, g = _scene([((3, 2), depths)])
    wide, narrow = _wide_vs_narrow(frame, g, sfgs_option)
    assert narrow["max_tile_list"] == others + n_tied
    assert narrow["sort_wide_tiles"] >= 1


def _limit_depths(extra_ulps, k=100):
    """k depths whose bit patterns span exactly (the 9-position-bit key's largest range) + extra_ulps"""
    limit = (1 << 23) - 2
    lo = int(np.asarray([2.0], np.float32).view(np.uint32)[0])
    bits = lo + np.linspace(0, limit + extra_ulps, k).astype(np.int64)
    bits[-1] = lo + limit + extra_ulps
    assert len(np.unique(bits)) == k
    z = bits.astype(np.uint32).view(np.float32)
    return np.random.default_rng(2).permutation(z)


@pytest.mark.parametrize("extra_ulps,expect_wide", [(-1, False), (0, False), (1, True)], ids=["below", "at", "above"])
def test_depth_range_at_the_key_limit(extra_ulps, expect_wide, sfgs_option):
    frame, g = _scene([((3, 2), _limit_depths(extra_ulps))])
    wide, narrow = _wide_vs_narrow(frame, g, sfgs_option)
    assert narrow["max_tile_list"] == 100
    if expect_wide:
        assert narrow["sort_wide_tiles"] >= 1
    else:
        assert narrow["sort_wide_tiles"] == 0


def test_depth_range_beyond_the_key(sfgs_option):
    """z from 1 to 300 in one tile: eight binades"""
    z = np.random.default_rng(6).permutation(np.geomspace(1.0, 300.0, 120).astype(np.float32))
    frame, g = _scene([((3, 2), z)])
    wide, narrow = _wide_vs_narrow(frame, g, sfgs_option)
    assert narrow["max_tile_list"] == 120
    assert narrow["sort_wide_tiles"] >= 1


@pytest.mark.parametrize("K", [2, 150])
def test_all_depths_equal(K, sfgs_option):
    frame, g = _scene([((3, 2), np.full(K, 300.0, np.float32))])
    wide, narrow = _wide_vs_narrow(frame, g, sfgs_option)
    assert narrow["max_tile_list"] == K
    assert narrow["sort_wide_tiles"] >= 1


def test_fallback_is_per_tile(sfgs_option):
    """2 x 2 tiles of one coarse bin (each row of two = waves of one workgroup), distinct depths everywhere except ONE pair of
    equal depths in one tile: that tile alone is sorted on the 64-bit key"""
    z = _distinct_depths(4 * 40 - 1)
    groups = [((0, 0), z[:40]), ((1, 0), np.concatenate([z[40:79], z[40:41]])), ((0, 1), z[79:119]), ((1, 1), z[119:159])]
    frame, g = _scene(groups)
    wide, narrow = _wide_vs_narrow(frame, g, sfgs_option)
    assert narrow["max_tile_list"] == 40
    assert narrow["sort_wide_tiles"] == 1
    assert wide["sort_wide_tiles"] == 4
