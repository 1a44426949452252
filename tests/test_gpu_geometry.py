"""GPU tests of sfgs.geometry (csrc/geometry.hip): depth -> DSM accumulation, dsmr registration, shift + compare. Every case
runs against the reference's own run where the golden has one (tests/golden/make_golden_geometry.py) and against the numpy
restatement (tests/geometry_np.py, held to the golden by tests/test_geometry_host.py) otherwise. Nothing here reads the
reference tree.

Bounds. Max mode: NaN pattern identical, heights within 1e-10 m (8 roundings x 1e3 m x 2^-53 ~ 1e-12). Mean mode: every
point is rounded to the fixed-point unit 2^-20 m (error <= half a unit each, so the mean's error <= half a unit), the
restatement's float64 sum of `count` heights below 2^10 m errs by <= count x 2^-43 m, and the final division rounds once:
bound = 2^-20 x (1 + count x 2^-23) m per cell, derived below from the unit. Registration: (dx, dy) exact; mu, sigma, xcorr, a, b
within 1e-10 relative (<= 5e4 float64 terms: worst case n 2^-53 ~ 6e-12). Metrics: counts and completeness exact, mae / rmse
1e-10 relative. apply_shift: the same bits."""
import os
import types

import numpy as np
import pytest
import torch

import geometry_np as gnp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_geometry.npz"))
REG_TAGS = sorted(k[len("reg_"):-len("_shift")] for k in G.files if k.startswith("reg_") and k.endswith("_shift"))
REL = 1e-10


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def f64(a):
    return np.asarray(a).astype(np.float64)


def cam_of(R, T, intr):
    return types.SimpleNamespace(R=R, T=T, focal_x=intr[0], focal_y=intr[1], cx=intr[2], cy=intr[3])


def accumulate(grid, views, mode="max", radius=1, origin=None):
    """views: [(depth, camera, mask)] -> (result float64 numpy, num_points int)"""
    from sfgs.geometry import DsmAccumulator, DsmGrid
    acc = DsmAccumulator(DsmGrid(*grid), mode=mode, radius=radius, device=DEV)
    for k, (depth, cam, mask) in enumerate(views):
        d = dev(depth)
        acc.add_view(d[None] if k % 2 else d, cam, origin=origin, mask=None if mask is None else dev(mask))
    out = acc.result()
    assert out.dtype == torch.float64 and tuple(out.shape) == (grid[3], grid[2]) and out.device == torch.device(DEV)
    return out.cpu().numpy(), int(acc.num_points)


def cloud_of(views, origin):
    return np.vstack([gnp.unproject(d, c.R, c.T, c.focal_x, c.focal_y, c.cx, c.cy, origin=origin, mask=m) for d, c, m in views])


def assert_max_equal(got, want):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)


def mean_bound(count):
    from sfgs.geometry import FIXED_POINT_UNIT
    return FIXED_POINT_UNIT * (1.0 + count * 2.0 ** -23)


# ---- accumulate ------------------------------------------------------------------------------------------------------------------
def golden_city():
    from sfgs.geometry import DsmGrid
    grid = tuple(DsmGrid.from_metadata(G["city_meta"]))
    views = [(d, cam_of(R, T, i), None) for d, R, T, i in zip(G["city_depths"], G["city_R"], G["city_T"], G["city_intr"])]
    return grid, views, G["city_origin"]


def test_three_views_at_utm_magnitude_equal_the_reference_dsm():
    grid, views, origin = golden_city()
    assert origin[0] == 4.0e5 and origin[1] == 3.3e6 and views[0][0].shape == (70, 130)
    got, n = accumulate(grid, views, origin=origin)
    assert_max_equal(got, G["city_dsm"])
    want, landed = gnp.dsm_max(cloud_of(views, origin), grid)
    assert_max_equal(got, want)
    assert n == landed
    one, _ = accumulate(grid, views[:1], origin=origin)
    assert_max_equal(one, G["city_dsm_view0"])


def test_planted_depths_with_and_without_mask_equal_the_reference_points():
    fx, fy, cx, cy = G["pc_intr"]
    cam, grid, origin = cam_of(G["pc_R"], G["pc_T"], G["pc_intr"]), tuple(G["pc_grid"]), G["pc_origin"]
    grid = (grid[0], grid[1], int(grid[2]), int(grid[3]), grid[4])
    depth = G["pc_depth"]
    assert depth.shape == (37, 53) and np.isposinf(depth).any() and np.isnan(depth).any() and (depth < 0).any()
    for mask, pts in ((None, G["pc_points"]), (G["pc_mask"], G["pc_points_masked"]), (G["pc_mask"].astype(np.uint8) * 5, G["pc_points_masked"])):
        want, landed = gnp.dsm_max(pts, grid)                      # the reference's points, flattened by the restatement
        got, n = accumulate(grid, [(depth, cam, mask)], origin=origin)
        assert_max_equal(got, want)
        assert n == landed > 0


@pytest.mark.parametrize("H,W", [(1, 1), (2, 1), (37, 53), (70, 130)])
@pytest.mark.parametrize("cells", [1, (7, 5), 64, 65])
def test_depth_and_grid_sizes(H, W, cells):
    xsize, ysize = (cells, cells) if isinstance(cells, int) else cells
    _, terrain, cams, depths, origin = gnp.city_views(2, H, W, 77 + H, cells=32)
    side = 16.0
    grid = (origin[0] + 1.0, origin[1] + side - 1.0, xsize, ysize, (side - 2.0) / max(xsize, ysize))
    views = [(d, c, None) for d, c in zip(depths, cams)]
    assert any((d > 0).any() for d in depths)
    cloud = cloud_of(views, origin)
    got, n = accumulate(grid, views, origin=origin)
    want, landed = gnp.dsm_max(cloud, grid)
    assert_max_equal(got, want)
    assert n == landed
    got, n = accumulate(grid, views, mode="mean", radius=1, origin=origin)
    total, count, landed = gnp.dsm_mean_sums(cloud, grid, 1)
    assert n == landed
    np.testing.assert_array_equal(np.isnan(got), count == 0)
    ok = count > 0
    assert (np.abs(got[ok] - total[ok] / count[ok]) <= mean_bound(count[ok])).all()


def test_one_cell_takes_a_whole_view_and_a_view_outside_leaves_nothing():
    _, _, cams, depths, origin = gnp.city_views(1, 64, 64, 5, cells=32)
    views = [(depths[0], cams[0], None)]
    cloud = cloud_of(views, None)
    assert len(cloud) > 3000
    big = (-1000.0, 1000.0, 1, 1, 2000.0)                      # every point in ONE cell: maximum contention
    got, n = accumulate(big, views)
    assert n == len(cloud) and got.shape == (1, 1) and abs(got[0, 0] - cloud[:, 2].max()) <= 1e-10
    got, n = accumulate(big, views, mode="mean", radius=3)
    assert n == len(cloud) and abs(got[0, 0] - cloud[:, 2].mean()) <= mean_bound(len(cloud))
    for mode in ("max", "mean"):
        got, n = accumulate((5000.0, 6000.0, 8, 8, 1.0), views, mode=mode)
        assert n == 0 and np.isnan(got).all()


def test_the_band_left_of_and_above_the_grid_lands_in_row_and_column_zero():
    """A nadir camera over a plane: pixel (u, v) at depth z lands at (u - cx) z / f east, -(v - cy) z / f north."""
    H = W = 16
    A = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])     # x east, y south, z down
    C = np.array([0.0, 0.0, 100.0])
    cam = types.SimpleNamespace(R=A, T=-A @ C, focal_x=100.0, focal_y=100.0, cx=0.0, cy=0.0)
    depth = np.full((H, W), 100.0, dtype=np.float32)           # points at (u - 8, 8 - v, 0): a 16 x 16 lattice, 1 m apart
    grid = (-5.5, 5.5, 4, 4, 2.0)                              # x from -5.5: the points at -7, -6 are in (-1, 0) cells
    pts = gnp.unproject(depth, cam.R, cam.T, 100.0, 100.0)
    qx, qy = gnp.cell_coords(pts, grid)
    band = ((qx > -1) & (qx < 0) & (qy > -1) & (qy < 4)) | ((qy > -1) & (qy < 0) & (qx > -1) & (qx < 4))
    assert band.sum() >= 8 and (qx <= -1).any() and (qy >= 4).any()
    got, n = accumulate(grid, [(depth, cam, None)], mode="mean", radius=0)
    total, count, landed = gnp.dsm_mean_sums(pts, grid, 0)
    assert n == landed == int(((qx > -1) & (qx < 4) & (qy > -1) & (qy < 4)).sum())
    assert count[0, 0] > count[1, 1]                           # row / column 0 took the band as well
    from sfgs.geometry import DsmAccumulator, DsmGrid
    acc = DsmAccumulator(DsmGrid(*grid), mode="mean", radius=0, device=DEV)
    acc.add_view(dev(depth), cam)
    np.testing.assert_array_equal(acc._count.cpu().numpy(), count)
    np.testing.assert_array_equal(np.isnan(got), count == 0)


@pytest.mark.parametrize("radius", [0, 1, 3])
def test_mean_mode_is_deterministic_and_within_the_fixed_point_bound(radius):
    grid, views, origin = golden_city()
    mask = np.random.default_rng(radius).random(views[1][0].shape) > 0.25
    views = [views[0], (views[1][0], views[1][1], mask), views[2]]
    a, n = accumulate(grid, views, mode="mean", radius=radius, origin=origin)
    b, _ = accumulate(grid, views, mode="mean", radius=radius, origin=origin)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    total, count, landed = gnp.dsm_mean_sums(cloud_of(views, origin), grid, radius)
    assert n == landed
    np.testing.assert_array_equal(np.isnan(a), count == 0)
    ok = count > 0
    err = np.abs(a[ok] - total[ok] / count[ok])
    assert (err <= mean_bound(count[ok])).all(), (err.max(), count.max())


# ---- registration ----------------------------------------------------------------------------------------------------------------
def run_register(ref, sec, irange=5, scaling=False, init=(0, 0), dtype=torch.float64):
    from sfgs.geometry import register
    s = register(dev(ref, dtype), dev(sec, dtype), irange=irange, scaling=scaling, init=init)
    assert s.shift.dtype == torch.int32 and s.ab.dtype == torch.float64 and s.shift.device == torch.device(DEV)
    return s


def assert_shift_equals(s, dx, dy, a, b, stats):
    got = s.cpu()
    assert got[:2] == (dx, dy), (got, dx, dy)
    np.testing.assert_allclose(got[2:], [a, b], rtol=REL, atol=1e-12)
    np.testing.assert_allclose(s.stats.cpu().numpy()[2:7], stats, rtol=REL, atol=0)


@pytest.mark.parametrize("tag", REG_TAGS)
def test_registration_equals_the_reference(tag):
    irange, scaling, ix, iy = (int(v) for v in G[f"reg_{tag}_params"])
    ref, sec = f64(G[f"reg_{tag}_ref"]), f64(G[f"reg_{tag}_sec"])
    for dtype in (torch.float64, torch.float32):               # the rasters are float16-exact: float32 input, the same result
        s = run_register(ref, sec, irange, bool(scaling), (ix, iy), dtype)
        assert_shift_equals(s, *G[f"reg_{tag}_shift"], *G[f"reg_{tag}_ab"], G[f"reg_{tag}_stats"])
    t = run_register(ref, sec, irange, bool(scaling), (ix, iy))
    assert torch.equal(s.shift, t.shift) and torch.equal(s.stats.view(torch.int64), t.stats.view(torch.int64))
    best = G[f"reg_{tag}_margins"][-1, 0]
    np.testing.assert_allclose(float(s.stats[7]), best, rtol=1e-9)


def test_expected_shift_of_the_differently_shaped_pair():
    s = run_register(f64(G["reg_110x130_shapes_ref"]), f64(G["reg_110x130_shapes_sec"]))
    assert s.cpu()[:2] == (7, -3)


def test_skipped_shifts_on_the_device():
    one = np.array([[3.0]])
    for scaling in (False, True):
        dx, dy, a, b = run_register(one, one, scaling=scaling).cpu()
        assert (dx, dy) == (0, 0) and np.isnan(b) and (np.isnan(a) if scaling else a == 1.0)
    ref, _ = gnp.shifted_pair(30, 40, 3, 0, 0, 0.0)
    dx, dy, a, b = run_register(ref, np.full((30, 40), np.nan), init=(2, -1)).cpu()
    assert (dx, dy, a) == (2, -1, 1.0) and np.isnan(b)
    ref, _ = gnp.shifted_pair(120, 130, 4, 0, 0, 0.0)          # one pyramid level, every shift of both levels skipped
    dx, dy, a, b = run_register(ref, np.full((50, 60), np.nan), init=(-3, 5)).cpu()
    assert (dx, dy) == (-4, 4) and np.isnan(b)                 # -3 // 2 * 2, 5 // 2 * 2
    flat = np.full((20, 20), 7.0)
    assert run_register(flat, ref[:20, :20]).cpu()[:2] == (0, 0)


def test_infinite_pixels_are_skipped_and_restatement_agrees_on_a_fresh_pair():
    ref, sec = gnp.shifted_pair(103, 131, 21, -3, 6, 0.5, sec_shape=(90, 140))
    ref.reshape(-1)[[4, 44, 444]] = [np.inf, -np.inf, np.inf]
    sec.reshape(-1)[[5, 55, 555]] = [-np.inf, np.inf, np.inf]
    margins = []
    dx, dy, a, b, stats = gnp.compute_shift(ref, sec, 5, True, (0, 0), margins)
    assert (dx, dy) == (-3, 6) and all(m[0] - m[1] >= 1e-6 for m in margins)
    assert_shift_equals(run_register(ref, sec, scaling=True), dx, dy, a, b, stats)


# ---- compare ---------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """float64 arrays equal bit for bit, any NaN equal to any NaN"""
    canon = lambda v: np.where(np.isnan(v), np.uint64(0x7ff8000000000000), np.ascontiguousarray(v).view(np.uint64))
    return a.shape == b.shape and np.array_equal(canon(a), canon(b))


def test_apply_shift_is_bit_identical_to_the_restatement():
    from sfgs.geometry import apply_shift
    sec = f64(G["ms_sec"])
    dx, dy, a, b = G["as_params"]
    found = run_register(f64(G["ms_ref"]), sec)
    given = found._replace(shift=dev(np.array([dx, dy], dtype=np.int32)), ab=dev(np.array([a, b])))
    for shift, dtype in ((given, torch.float64), (found, torch.float64), (given, torch.float32)):
        got = apply_shift(dev(sec, dtype), shift)
        assert got.dtype == torch.float64 and tuple(got.shape) == sec.shape
        assert same_bits(got.cpu().numpy(), gnp.apply_shift(sec, *shift.cpu()))
    assert same_bits(apply_shift(dev(sec), given).cpu().numpy(), G["as_out"])
    zero = given._replace(ab=dev(np.array([1.0, 0.0])))
    got = apply_shift(dev(np.array([[-0.0, 1.0], [2.0, -3.0]])), zero._replace(shift=dev(np.zeros(2, dtype=np.int32))))
    assert same_bits(got.cpu().numpy(), np.array([[0.0, 1.0], [2.0, -3.0]]))     # the reference's zero terms turn -0 into +0


def assert_metrics(got, want):
    host = {k: v.cpu().item() for k, v in got.items()}
    assert got["valid_pixels"].dtype == torch.int64 and got["mae"].dtype == torch.float64
    assert host["valid_pixels"] == want["valid_pixels"] and host["completeness"] == want["completeness"]
    if want["valid_pixels"] == 0:
        assert np.isnan(host["mae"]) and np.isnan(host["rmse"])
    else:
        np.testing.assert_allclose([host["mae"], host["rmse"]], [want["mae"], want["rmse"]], rtol=REL, atol=0)


def test_metrics_with_and_without_shift_and_mask():
    from sfgs.geometry import dsm_metrics, register, register_simple
    pred, gt, keep = f64(G["met_pred"]), f64(G["met_gt"]), G["met_keep"]
    for tag, mask in (("plain", None), ("masked", keep)):
        got = dsm_metrics(dev(pred), dev(gt), mask=None if mask is None else dev(mask))
        want = G[f"met_{tag}"]
        assert_metrics(got, {"mae": want[0], "rmse": want[1], "valid_pixels": want[2], "completeness": want[3]})
    inf = dsm_metrics(dev(f64(G["met_pred_inf"])), dev(gt))      # an infinite height is valid (`~isnan`): counted, mae = inf
    assert inf["valid_pixels"].item() == G["met_inf"][2] and inf["completeness"].item() == G["met_inf"][3]
    assert np.isinf(inf["mae"].item()) and np.isinf(inf["rmse"].item())
    shift = register(dev(gt), dev(pred))
    for mask in (None, keep):
        for dtype in (torch.float64, torch.float32):
            got = dsm_metrics(dev(pred, dtype), dev(gt, dtype), shift=shift, mask=None if mask is None else dev(mask))
            assert_metrics(got, gnp.dsm_metrics(pred, gt, mask, shift=shift.cpu()))
    nan = np.full_like(pred, np.nan)
    assert_metrics(dsm_metrics(dev(nan), dev(gt)), gnp.dsm_metrics(nan, gt))                  # no valid pixel
    assert_metrics(dsm_metrics(dev(pred), dev(nan)), gnp.dsm_metrics(pred, nan))              # valid_gt == 0
    assert_metrics(dsm_metrics(dev(pred), dev(gt), mask=dev(np.zeros_like(keep))), gnp.dsm_metrics(pred, gt, np.zeros_like(keep)))
    np.testing.assert_allclose(register_simple(dev(pred), dev(gt)).item(), G["met_dz"], rtol=REL, atol=0)
    assert register_simple(dev(nan), dev(gt)).item() == 0.0
    big_p, big_g = gnp.shifted_pair(300, 517, 8, 0, 0, 0.4)          # more than one workgroup per partial, odd size
    assert_metrics(dsm_metrics(dev(big_p), dev(big_g)), gnp.dsm_metrics(big_p, big_g))
    a, b = dsm_metrics(dev(big_p), dev(big_g)), dsm_metrics(dev(big_p), dev(big_g))
    assert all(torch.equal(a[k], b[k]) or (torch.isnan(a[k]) and torch.isnan(b[k])) for k in a)


def city_case(n_views=6):
    grid, terrain, cams, depths, origin = gnp.city_views(n_views, 70, 130, 4242)
    rng = np.random.default_rng(1)
    gt = np.roll(terrain, (2, -3), axis=(0, 1)) + 0.8 + rng.normal(0, 0.05, terrain.shape)
    keep = rng.random(terrain.shape) > 0.1
    return grid, cams, depths, origin, gt, keep


def test_evaluate_dsm_equals_the_staged_calls():
    from sfgs.geometry import DsmAccumulator, DsmGrid, dsm_metrics, evaluate_dsm, register
    grid, cams, depths, origin, gt, keep = city_case()
    g = DsmGrid(*grid)
    d = [dev(x) for x in depths]
    report = evaluate_dsm(d, cams, g, dev(gt), origin=origin, keep_mask=dev(keep))
    acc = DsmAccumulator(g, device=DEV)
    for x, cam in zip(d, cams):
        acc.add_view(x, cam, origin=origin)
    pred = torch.where(dev(keep), acc.result(), torch.full_like(acc.result(), float("nan")))
    shift = register(dev(gt), pred)
    m = dsm_metrics(pred, dev(gt), shift=shift, mask=dev(keep))
    dx, dy, a, b = shift.cpu()
    assert report == {"mae": m["mae"].item(), "rmse": m["rmse"].item(), "valid_pixels": m["valid_pixels"].item(),
                      "completeness": m["completeness"].item(), "dx_offset": dx, "dy_offset": dy, "dz_offset": b,
                      "total_points": int(acc.num_points)}
    assert all(type(v) in (int, float) for v in report.values()) and report["valid_pixels"] > 1000 and report["total_points"] > 10000
    # and the whole chain in numpy
    cloud = np.vstack([gnp.unproject(x, c.R, c.T, c.focal_x, c.focal_y, c.cx, c.cy, origin=origin) for x, c in zip(depths, cams)])
    want_pred = np.where(keep, gnp.dsm_max(cloud, grid)[0], np.nan)
    wdx, wdy, wa, wb, _ = gnp.compute_shift(gt, want_pred)
    want = gnp.dsm_metrics(want_pred, gt, keep, shift=(wdx, wdy, wa, wb))
    assert (dx, dy) == (wdx, wdy) and report["valid_pixels"] == want["valid_pixels"] and report["completeness"] == want["completeness"]
    np.testing.assert_allclose([report["mae"], report["rmse"], report["dz_offset"]], [want["mae"], want["rmse"], wb], rtol=REL)


def test_whole_module_runs_on_a_non_default_stream():
    from sfgs.geometry import DsmGrid, apply_shift, evaluate_dsm, register
    grid, cams, depths, origin, gt, keep = city_case(2)
    g = DsmGrid(*grid)
    d, gt_d, keep_d = [dev(x) for x in depths], dev(gt), dev(keep)
    want = evaluate_dsm(d, cams, g, gt_d, origin=origin, keep_mask=keep_d, mode="mean")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(DEV) == side and side.cuda_stream != 0
        got = evaluate_dsm(d, cams, g, gt_d, origin=origin, keep_mask=keep_d, mode="mean")
        s = register(gt_d, gt_d, irange=2)
        moved = apply_shift(gt_d, s)
    side.synchronize()
    assert got == want or all(got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])) for k in got)
    assert s.cpu()[:2] == (0, 0) and torch.equal(moved, gt_d + 0.0)
