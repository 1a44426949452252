"""GPU tests of sfgs.ortho (csrc/ortho.hip): rendered views -> the true orthophoto on the DSM's grid. The reference is the numpy
restatement tests/ortho_np.py (held to independent spellings by tests/test_ortho_host.py). Nothing here reads the reference tree.

Bounds. Every comparison is exact (assert_array_equal; the NaN pattern of `height` included): the kernels perform the
restatement's float64 operations in its order, nothing contracted, round once to float32 and take integer maxima, so there is
nothing to tolerate."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import geometry_np as gnp
import ortho_np as onp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("rgb", "height", "source", "state", "coverage")


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))          # a copy: the shared scenes are read-only
    return (t if dtype is None else t.to(dtype)).to(DEV)


def dsm_grid(grid):
    from sfgs.geometry import DsmGrid
    return DsmGrid(*grid)


def accumulate(views, grid, origin=None, implicit_tags=False):
    from sfgs.ortho import OrthoAccumulator
    o = OrthoAccumulator(dsm_grid(grid), device=DEV)
    for v in views:
        o.add_view(dev(v.depth), dev(v.image), v.camera, origin=origin, mask=None if v.mask is None else dev(v.mask),
                   tag=None if implicit_tags else v.tag)
    return o


def host(res):
    assert all(getattr(res, f).device == torch.device(DEV) for f in FIELDS)
    return onp.Result(*(getattr(res, f).cpu().numpy() for f in FIELDS))


def assert_same(got, want, grid):
    _, _, xsize, ysize, _ = grid
    assert got.rgb.dtype == np.uint8 and got.rgb.shape == (ysize, xsize, 3)
    assert got.height.dtype == np.float32 and got.height.shape == (ysize, xsize)
    assert got.source.dtype == np.uint8 and got.state.dtype == np.uint8 and got.source.shape == got.state.shape == (ysize, xsize)
    assert got.coverage.dtype == np.int64 and got.coverage.shape == (256,) and got.coverage.sum() == xsize * ysize
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f)
    empty = want.state == 0
    np.testing.assert_array_equal(got.height.view(np.uint32)[empty], np.uint32(0x7fc00000))


def check_against_restatement(views, grid, origin, fills=(0, 1, 2, 3)):
    acc, n = onp.keys(views, grid, origin)
    o = accumulate(views, grid, origin)
    assert o.num_points.dtype == torch.int64 and o.num_points.is_cuda and int(o.num_points) == n
    for fill in fills:
        assert_same(host(o.result(fill=fill)), onp.resolve(acc, fill), grid)
    return o, acc


@functools.lru_cache(maxsize=None)
def base_views():
    """The base scene with a mask on view 1 -> (grid, views, origin)"""
    grid, cams, depths, images, origin = onp.base_scene()
    mask = np.random.default_rng(3).random((40, 48)) > 0.3
    views = tuple(onp.View(d, i, c, mask if k == 1 else None, k + 1) for k, (d, i, c) in enumerate(zip(depths, images, cams)))
    return grid, views, origin


# ---- 1. all five outputs against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("altitude", [20.0, -30.0, -12.0])
def test_all_outputs_equal_the_restatement_at_every_fill(altitude):
    """+20: the scene's own origin, every height positive; -30 (the issue's) : every height negative, the other branch of K32;
    -12: heights on both sides of zero in ONE accumulator."""
    grid, views, origin = base_views()
    assert all(v.camera.cx != 0 or v.camera.cy != 0 for v in views[1:]) and views[1].mask is not None
    origin = np.array([origin[0], origin[1], altitude])
    o, acc = check_against_restatement(views, grid, origin)
    h = onp.resolve(acc, 0).height
    assert {20.0: np.nanmin(h) > 0, -30.0: np.nanmax(h) < 0, -12.0: np.nanmin(h) < 0 < np.nanmax(h)}[altitude]
    if altitude == 20.0:                                   # without the mask: the figures the scene was chosen for
        plain = [v._replace(mask=None) for v in views]
        acc, n = onp.keys(plain, grid, origin)
        assert (n, int((acc != 0).sum())) == (5294, 487)
        assert [(int((r.state == 0).sum()), int((r.state == 2).sum())) for r in (onp.resolve(acc, f) for f in range(4))] == \
            [(89, 0), (32, 57), (10, 79), (0, 89)]
        check_against_restatement(plain, grid, origin)


# ---- 2. order independence -------------------------------------------------------------------------------------------------------
def test_any_view_order_and_any_run_give_the_same_bits():
    grid, views, origin = base_views()
    acc, _ = onp.keys(views, grid, origin)
    want = {fill: onp.resolve(acc, fill) for fill in (0, 2)}
    orders = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0), (0, 1, 2)]      # all six, the first one twice
    for order in orders:
        o = accumulate([views[k] for k in order], grid, origin)
        np.testing.assert_array_equal(o._acc.cpu().numpy().view(np.uint64), acc)
        for fill, w in want.items():
            assert_same(host(o.result(fill=fill)), w, grid)


# ---- 3. the DSM's cells and heights ----------------------------------------------------------------------------------------------
def test_heights_are_float32_of_the_dsm_maximum_cell_for_cell():
    from sfgs.geometry import DsmAccumulator
    grid, views, origin = base_views()
    o = accumulate(views, grid, origin)
    dsm = DsmAccumulator(dsm_grid(grid), mode="max", device=DEV)
    for v in views:
        dsm.add_view(dev(v.depth), v.camera, origin=origin, mask=None if v.mask is None else dev(v.mask))
    want, got = dsm.result().to(torch.float32).cpu().numpy(), o.result().height.cpu().numpy()
    assert np.isnan(want).any() and not np.isnan(want).all()
    np.testing.assert_array_equal(got, want)               # equal values and the same NaN cells
    assert int(o.num_points) == int(dsm.num_points) > 0


# ---- 4. float32 ties -------------------------------------------------------------------------------------------------------------
def nadir_case():
    R = np.diag([1.0, -1.0, -1.0])
    C = np.array([16.0, 14.0, 70.0])
    cam = types.SimpleNamespace(R=R, T=-R @ C, focal_x=37.5, focal_y=37.5, cx=0.0, cy=0.0)
    d60 = np.float32(60.0)
    depth = np.where(np.add.outer(np.arange(12), np.arange(20)) % 2 == 0, d60, np.nextafter(d60, np.float32(61.0))).astype(np.float32)
    return cam, depth, (0.0, 24.0, 8, 6, 4.0), np.array([0.0, 0.0, 4096.0])


def test_heights_that_tie_in_float32_are_decided_by_colour_then_by_tag():
    cam, depth, grid, origin = nadir_case()
    pts = onp.unproject(depth, cam, origin)
    h64 = np.unique(pts[:, 2])
    assert len(h64) == 2 and 3.7e-6 < h64[1] - h64[0] < 3.9e-6 and np.spacing(np.float32(h64[1])) > 4.8e-4
    assert len(np.unique(pts[:, 2].astype(np.float32))) == 1          # float64 heights differ, their float32 values do not
    image = onp.seeded_images([depth], 5)[0]
    view = onp.View(depth, image, cam, None, 1)
    o, acc = check_against_restatement([view], grid, origin, fills=(0, 1))
    res = host(o.result())
    gx, gy, inside = gnp.cells(pts, grid)
    assert inside.all()
    counts = np.zeros((6, 8), dtype=np.int64)
    np.add.at(counts, (gy, gx), 1)
    assert (counts[:5] >= 2).all() and counts.max() == 9 and (counts[5] == 0).all() and (res.state[5] == 0).all()
    col = onp.quantize(image).reshape(3, -1).T
    for y in range(5):
        for x in range(8):
            here = (gy == y) & (gx == x)
            assert tuple(res.rgb[y, x]) == max(tuple(int(c) for c in row) for row in col[here])     # not the higher float64 point's
    lower = pts[:, 2] == h64[0]
    winners = {tuple(int(c) for c in res.rgb[y, x]) for y in range(5) for x in range(8)}
    assert winners & {tuple(int(c) for c in row) for row in col[lower]}, "no cell was won by a point that is lower in float64"
    # the same view twice: equal height and colour, the larger tag wins everywhere
    for tags in ((1, 2), (2, 1)):
        twice = accumulate([view._replace(tag=t) for t in tags], grid, origin)
        r2 = host(twice.result())
        np.testing.assert_array_equal(r2.source, np.where(res.state != 0, 2, 0))
        np.testing.assert_array_equal(r2.rgb, res.rgb)
        assert int(twice.num_points) == 2 * int(o.num_points) == 480 and r2.coverage[2] == 40 and r2.coverage[1] == 0


# ---- 5. a grid smaller than the footprint ----------------------------------------------------------------------------------------
def test_points_outside_on_all_four_sides_are_dropped_and_the_band_below_zero_lands_in_cell_zero():
    grid, views, origin = base_views()
    views = [v._replace(mask=None) for v in views]
    small = (grid[0] + 3, grid[1] - 2.5, 10, 9, grid[4])
    pts = np.vstack([onp.unproject(v.depth, v.camera, origin) for v in views])
    qx, qy = gnp.cell_coords(pts, small)
    assert [int(s.sum()) for s in (qx < 0, qx >= 10, qy < 0, qy >= 9)] == [1103, 1494, 1224, 2303]
    assert (int(((qx > -1) & (qx < 0)).sum()), int(((qy > -1) & (qy < 0)).sum())) == (202, 204)       # truncation: cell 0
    o, acc = check_against_restatement(views, small, origin)
    inside = (np.trunc(qx) >= 0) & (qx < 10) & (np.trunc(qy) >= 0) & (qy < 9)
    assert 0 < int(o.num_points) == int(inside.sum()) < len(pts)
    band = inside & ((qx < 0) | (qy < 0))                  # landed through truncation: in column 0 or row 0
    gx, gy = np.trunc(qx[band]).astype(int), np.trunc(qy[band]).astype(int)
    assert band.sum() > 50 and ((gx == 0) | (gy == 0)).all() and (acc[gy, gx] != 0).all()


# ---- 6. extremes -----------------------------------------------------------------------------------------------------------------
def test_one_cell_takes_every_atomic():
    grid, views, origin = base_views()
    one = (grid[0] - 100.0, grid[1] + 100.0, 1, 1, 400.0)
    o, acc = check_against_restatement(views, one, origin, fills=(0, 3))
    assert int(o.num_points) == sum(int(onp.used_pixels(v.depth, v.mask).sum()) for v in views) and acc[0, 0] != 0
    assert host(o.result()).coverage[0] == 0


def test_a_view_smaller_than_one_wave():
    cam, _, grid, origin = nadir_case()
    depth = np.random.default_rng(2).uniform(55.0, 65.0, (5, 7)).astype(np.float32)
    depth[2, 3] = 0.0
    view = onp.View(depth, onp.seeded_images([depth], 8)[0], cam, None, 255)
    o, _ = check_against_restatement([view], grid, origin)
    assert int(o.num_points) == 34 and int(o.result().source.max()) == 255


def test_an_all_zero_depth_map_leaves_everything_empty():
    grid, views, origin = base_views()
    o = accumulate([views[0]._replace(depth=np.zeros((40, 48), dtype=np.float32))], grid, origin)
    for fill in (0, 3):
        r = host(o.result(fill=fill))
        assert int(o.num_points) == 0 and r.coverage[0] == 576 and (r.coverage[1:] == 0).all()
        assert not r.rgb.any() and not r.source.any() and not r.state.any()
        np.testing.assert_array_equal(r.height.view(np.uint32), np.uint32(0x7fc00000))


def test_colours_outside_the_unit_interval_and_nan_are_clipped():
    cam, depth, grid, origin = nadir_case()
    image = np.empty((3, 12, 20), dtype=np.float32)
    image[0], image[1], image[2] = np.nan, -1.0, 2.0
    view = onp.View(depth, image, cam, None, 9)
    o, _ = check_against_restatement([view], grid, origin, fills=(0,))
    r = host(o.result())
    filled = r.state == 1
    assert filled.sum() == 40 and (r.rgb[filled] == np.array([0, 0, 255], dtype=np.uint8)).all()


# ---- 7. size ---------------------------------------------------------------------------------------------------------------------
def wavy_view(H, W, tag):
    cam = gnp.look_down_camera(np.array([24.0, 24.0, 12.0]), 64.0, 23.0, 96.0, focal=900.0, cx=0.02, cy=-0.01)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (96.0 + 6.0 * np.sin(xx / 37.0) * np.cos(yy / 53.0) + np.random.default_rng(7).uniform(-2, 2, (H, W))).astype(np.float32)
    mask = np.random.default_rng(8).random((H, W)) > 0.1
    return onp.View(depth, onp.seeded_images([depth], 9)[0], cam, mask, tag), np.array([4.0e5, 3.3e6, 20.0])


def test_a_512_square_view_onto_96_square_cells():
    view, origin = wavy_view(512, 512, 3)
    grid = (4.0e5, 3.3e6 + 48.0, 96, 96, 0.5)
    o, acc = check_against_restatement([view], grid, origin, fills=(0, 3))
    assert int(o.num_points) > 150000 and 8000 < int((acc != 0).sum()) < 96 * 96      # ~ 20 points per filled cell, some cells empty


def test_more_pixels_and_cells_than_one_pass_of_the_capped_grids():
    """Both kernels stride once their capped grid is full: the accumulate kernel beyond 1024 workgroups (2^18 pixels), the
    resolve kernel beyond 512 (2^17 cells). 520 x 512 pixels onto 384 x 352 cells: the last pass of each is a partial one."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "skyfall-gs_amd", "csrc", "ortho.hip")).read()
    threads, acc_cap, res_cap = (int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1))
                                 for n in ("ORTHO_THREADS", "ORTHO_ACC_MAX_BLOCKS", "ORTHO_RESOLVE_MAX_BLOCKS"))
    assert threads * acc_cap < 520 * 512 < 2 * threads * acc_cap and threads * res_cap < 384 * 352 < 2 * threads * res_cap
    view, origin = wavy_view(520, 512, 200)
    grid = (4.0e5, 3.3e6 + 46.0, 384, 352, 0.125)
    o, acc = check_against_restatement([view], grid, origin, fills=(0, 2))
    filled = int((acc != 0).sum())
    assert int(o.num_points) > 100000 and 50000 < filled < 384 * 352 and (acc[-1] != 0).any()      # empty cells: the gather runs


# ---- 8. wiring -------------------------------------------------------------------------------------------------------------------
def test_evaluate_dsm_with_an_ortho_reports_the_same_and_fills_it():
    from sfgs.geometry import evaluate_dsm
    from sfgs.ortho import OrthoAccumulator
    grid, views, origin = base_views()
    g = dsm_grid(grid)
    rng = np.random.default_rng(1)
    terrain = gnp.city_views(0, 40, 48, seed=1, cells=24)[1]
    gt = dev(terrain + origin[2] + rng.normal(0, 0.05, terrain.shape))
    depths, cams, images = [dev(v.depth) for v in views], [v.camera for v in views], [dev(v.image) for v in views]
    masks = [None if v.mask is None else dev(v.mask) for v in views]
    plain = evaluate_dsm(depths, cams, g, gt, origin=origin, view_masks=masks)
    o = OrthoAccumulator(g, device=DEV)
    with_ortho = evaluate_dsm(depths, cams, g, gt, origin=origin, view_masks=masks, ortho=o, images=images)
    assert with_ortho == plain and plain["valid_pixels"] > 300 and plain["total_points"] == int(o.num_points)
    alone = accumulate(views, grid, origin, implicit_tags=True)
    assert o.num_views == alone.num_views == 3
    for fill in (0, 1):
        assert_same(host(o.result(fill=fill)), host(alone.result(fill=fill)), grid)
    assert_same(host(o.result()), onp.resolve(onp.keys(views, grid, origin)[0], 0), grid)
    with pytest.raises(ValueError, match="images"):
        evaluate_dsm(depths, cams, g, gt, origin=origin, ortho=o)
    with pytest.raises(ValueError, match="images"):
        evaluate_dsm(depths, cams, g, gt, origin=origin, ortho=o, images=images[:2])
    # reset() empties
    assert int(o.reset().num_points) == 0 and o.num_views == 0
    r = host(o.result(fill=3))
    assert r.coverage[0] == 576 and not r.state.any() and np.isnan(r.height).all()
    o.add_view(depths[0], images[0], cams[0], origin=origin)
    assert int(o.result().source.max()) == 1               # implicit tags start again


def test_wrong_arguments_raise_value_error():
    from sfgs.ortho import OrthoAccumulator
    grid, views, origin = base_views()
    v = views[0]
    o = OrthoAccumulator(dsm_grid(grid), device=DEV)
    d, img = dev(v.depth), dev(v.image)
    for depth, image in ((d.cpu(), img), (d, img.cpu()), (d, img[:2]), (d, img[:, :39]), (d, img.double()), (d[:39], img), (d, None)):
        with pytest.raises(ValueError):
            o.add_view(depth, image, v.camera, origin=origin)
    with pytest.raises(ValueError):
        o.add_view(d, img, v.camera, origin=origin, mask=dev(np.ones((40, 48), dtype=bool)).cpu())
    for tag in (0, 256, 2.0):
        with pytest.raises(ValueError, match="tag"):
            o.add_view(d, img, v.camera, origin=origin, tag=tag)
    assert o.num_views == 0 and int(o.num_points) == 0
    tiny = OrthoAccumulator(dsm_grid((-2.0, 2.0, 1, 1, 4.0)), device=DEV)           # the one point, (-0.5, -0.5, 1), is inside
    one, rgb = torch.ones((1, 1), device=DEV), torch.ones((3, 1, 1), device=DEV)
    cam = types.SimpleNamespace(R=np.eye(3), T=np.zeros(3), focal_x=1.0, focal_y=1.0)
    for _ in range(255):
        tiny.add_view(one, rgb, cam)
    with pytest.raises(ValueError, match="255"):           # the 256th implicit tag
        tiny.add_view(one, rgb, cam)
    tiny.add_view(one, rgb, cam, tag=255)                  # an explicit one is still welcome
    assert tiny.num_views == 256 and int(tiny.num_points) == 256 and int(tiny.result().source[0, 0]) == 255


# ---- 9. save_png -----------------------------------------------------------------------------------------------------------------
def test_save_png_round_trips_and_writes_the_world_file(tmp_path):
    from PIL import Image
    grid, views, origin = base_views()
    o = accumulate(views, grid, origin)
    for fill in (0, 2):
        path = str(tmp_path / "sub" / f"ortho_{fill}.png")
        o.save_png(path, fill=fill)
        res = host(o.result(fill=fill))
        with Image.open(path) as im:
            assert im.mode == "RGBA" and im.size == (24, 24)
            px = np.asarray(im)
        np.testing.assert_array_equal(px[..., :3], res.rgb)
        np.testing.assert_array_equal(px[..., 3], np.where(res.state != 0, 255, 0))
        lines = open(os.path.splitext(path)[0] + ".pgw").read().split("\n")
        xoff, yoff_top, _, _, r = grid
        assert lines == [repr(r), "0.0", "0.0", repr(-r), repr(xoff + r / 2), repr(yoff_top - r / 2), ""]
        assert [float(s) for s in lines[:6]] == [r, 0.0, 0.0, -r, xoff + r / 2, yoff_top - r / 2]
