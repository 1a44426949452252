#!/usr/bin/env python
"""Golden vectors of the geometry evaluation: the reference's OWN functions, imported from evaluate_gs_geometry.py and dsmr.py
and run on CPU arrays.

Runs only in the authoring container (it imports /root/reference read-only). Third-party modules the container lacks
(rasterio, cv2, sklearn, utm, pyproj, open3d, osgeo, plyflatten, ...) are replaced by empty stand-ins, `mean_absolute_error`
by its one-line definition, and `numba.jit` by the identity: dsmr.py then runs as plain Python (about two minutes for the
cases below). dsmr's rasters are passed as float64 [1,H,W]: that is the precision numba's typing gives the reference's
accumulators whatever the raster's dtype. No reference text is copied.

Recorded (tests/test_geometry_host.py describes how each is used):
  pc_*    depth_to_point_cloud (enu_origin=None; the origin is added here the way enu_to_utm_coordinates adds it) on a small
          view with NaN / +-inf / 0 / negative depths planted (+inf scrubbed to 0 for the reference, as its caller does) and a
          masked one (the reference's caller multiplies the depth by the mask)
  city_*  three 70 x 130 views of the synthetic city at UTM magnitude -> create_dsm_manual_satnerf_style on the stacked cloud
  ds_*    dsmr.downsample2x;  ms_*  dsmr.mean_std;  as_*  dsmr.apply_shift_
  reg_*   dsmr.recursive_ncc + the (a, b) of dsmr.compute_shift, with the score of every shift at every level
  met_*   compute_dsm_metrics (plain, masked, no valid pixel, and with two infinite heights, which `~isnan` counts as valid),
          register_dsms_simple
and the two CONDITIONS, asserted here and again by the host test on the recorded values:
  *_cell_margin   every golden point's cell coordinate is at least 1e-6 cells from an integer (no cell can flip under a
                  re-ordered float64 evaluation, whose error is ~3e-9 m)
  reg_*_margins   at every pyramid level the best score exceeds the runner-up by at least 1e-6
Registration rasters are multiples of 1/16 m below 128 m and stored as float16 (exact); the seeds are re-drawn until the
conditions hold.

usage: python tests/golden/make_golden_geometry.py [--check]     (--check: regenerate and compare with the committed file)
"""
import importlib.machinery
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "reference_geometry.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_np as gnp  # noqa: E402

CELL_MARGIN = 1e-6
SCORE_MARGIN = 1e-6


class _Anything(types.ModuleType):
    """a module whose every attribute is another stand-in (callable, usable as a decorator)"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        child = _Anything(f"{self.__name__}.{name}")
        setattr(self, name, child)
        return child

    def __call__(self, *a, **k):
        return a[0] if len(a) == 1 and callable(a[0]) and not k else self


def import_reference():
    def stand_in(name):
        if name not in sys.modules:
            m = _Anything(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            sys.modules[name] = m
        return sys.modules[name]
    for name in ("rasterio", "cv2", "sklearn", "sklearn.metrics", "utm", "pyproj", "open3d", "osgeo", "tqdm", "torchvision",
                 "scene", "gaussian_renderer", "utils", "utils.general_utils", "utils.system_utils", "arguments", "numba",
                 "matplotlib", "matplotlib.pyplot", "matplotlib.colors", "scipy", "plyflatten"):
        try:
            if name in ("scipy", "matplotlib", "matplotlib.pyplot", "matplotlib.colors", "tqdm", "torchvision"):
                __import__(name)
                continue
        except ImportError:
            pass
        stand_in(name)
    sys.modules["sklearn.metrics"].mean_absolute_error = lambda a, b: np.mean(np.abs(np.asarray(a) - np.asarray(b)))
    sys.modules["numba"].jit = lambda *a, **k: a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f)
    sys.path.insert(0, REF)
    import dsmr
    import evaluate_gs_geometry as egg
    return egg, dsmr


def registration_cases():
    """tag -> dict(ref, sec, irange, scaling, init): rasters float64"""
    out = {}

    def pair(tag, rows, cols, dx, dy, dz, irange=5, scaling=False, init=(0, 0), seed=0, **kw):
        ref, sec = gnp.shifted_pair(rows, cols, 9000 + seed, dx, dy, dz, **kw)
        out[tag] = dict(ref=ref, sec=sec, irange=irange, scaling=scaling, init=init)
    pair("9x7", 7, 9, 1, -1, 0.5, seed=1, nan_fraction=0.0)
    pair("100x101", 100, 101, 2, 3, -1.25, seed=2)
    pair("101x102", 101, 102, -4, 2, 2.0, seed=3)
    pair("110x130_shapes", 110, 130, 7, -3, 1.5, seed=4, sec_shape=(121, 117))
    pair("205x210", 205, 210, 9, -14, 0.75, seed=5)
    pair("101x102_negodd_init", 101, 102, -5, 3, 0.0, seed=6, init=(-3, 3))
    pair("40x50_irange1", 40, 50, 1, -1, 0.25, irange=1, seed=7)
    pair("40x50_irange7", 40, 50, -6, 7, 0.25, irange=7, seed=8)
    pair("40x50_scaling", 40, 50, 2, 1, 3.0, scaling=True, seed=9, scale=1.3)
    return out


def run_registration(dsmr, case):
    """-> dx, dy, a, b, stats[5], margins [levels, 2] (coarsest first) from the reference's functions"""
    u, v = case["ref"][None], case["sec"][None]
    log = []
    plain = dsmr.ncc

    def logged(a, b, x=0, y=0):
        c = plain(a, b, x, y)
        log.append(c)
        return c
    dsmr.ncc = logged
    try:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            dx, dy = dsmr.recursive_ncc(u, v, case["irange"], *case["init"])
            stats = [float(t) for t in dsmr.mean_std(u, v, dx, dy)]
    finally:
        dsmr.ncc = plain
    a = stats[2] / stats[3] if case["scaling"] else 1.0          # compute_shift's last three statements
    b = stats[0] - stats[1] * a
    n = (2 * case["irange"] + 1) ** 2
    assert len(log) % n == 0
    margins = []
    for k in range(0, len(log), n):
        sc = np.sort(np.asarray([c for c in log[k:k + n] if np.isfinite(c)], dtype=np.float64))
        margins.append((sc[-1], sc[-2]))
    return int(dx), int(dy), a, b, np.asarray(stats), np.asarray(margins)


def planted_depth(H, W, seed):
    grid, terrain, cams, depths, origin = gnp.city_views(1, H, W, seed, cells=24)
    d = depths[0].copy()
    flat = d.reshape(-1)
    flat[[3, 10, 17, 24, 31, 38]] = [np.nan, np.inf, -np.inf, 0.0, -2.5, -0.0]
    return grid, cams[0], d, origin


def cell_margin(points, grid):
    qx, qy = gnp.cell_coords(points, grid)
    q = np.concatenate([qx, qy])
    return float(np.abs(q - np.rint(q)).min())


def generate():
    egg, dsmr = import_reference()
    out = {}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        # ---- stage 1 ---------------------------------------------------------------------------------------------------------
        import contextlib
        import io
        quiet = contextlib.redirect_stdout(io.StringIO())      # the reference prints per call
        for seed in range(100):
            grid, cam, depth, origin = planted_depth(37, 53, 1000 + seed)
            mask = np.random.default_rng(seed).random(depth.shape) > 0.3
            scrubbed = np.where(np.isposinf(depth), np.float32(0), depth)
            with quiet:
                pts = egg.depth_to_point_cloud(scrubbed, cam, None) + origin
                pts_m = egg.depth_to_point_cloud(scrubbed * mask, cam, None) + origin
            if min(cell_margin(pts, grid), cell_margin(pts_m, grid)) >= CELL_MARGIN:
                break
        else:
            raise AssertionError("no seed meets the cell condition")
        out.update(pc_depth=depth, pc_mask=mask, pc_R=cam.R, pc_T=cam.T, pc_intr=np.array([cam.focal_x, cam.focal_y, cam.cx, cam.cy]),
                   pc_origin=origin, pc_grid=np.asarray(grid, dtype=np.float64), pc_points=pts, pc_points_masked=pts_m,
                   pc_cell_margin=np.float64(min(cell_margin(pts, grid), cell_margin(pts_m, grid))))
        for seed in range(100):
            grid, terrain, cams, depths, origin = gnp.city_views(3, 70, 130, 2000 + seed)
            with quiet:
                cloud = np.vstack([egg.depth_to_point_cloud(d, c, None) + origin for d, c in zip(depths, cams)])
            if cell_margin(cloud, grid) >= CELL_MARGIN:
                break
        else:
            raise AssertionError("no seed meets the cell condition")
        meta = np.array([grid[0], grid[1] - grid[3] * grid[4], grid[2], grid[4]])
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "city_DSM.txt")
            np.savetxt(path, meta, fmt="%.17g")
            dsm = egg.create_dsm_manual_satnerf_style(cloud, path)
            with quiet:
                one = egg.create_dsm_manual_satnerf_style(egg.depth_to_point_cloud(depths[0], cams[0], None) + origin, path)
        out.update(city_depths=np.stack(depths), city_R=np.stack([c.R for c in cams]), city_T=np.stack([c.T for c in cams]),
                   city_intr=np.array([[c.focal_x, c.focal_y, c.cx, c.cy] for c in cams]), city_origin=origin, city_meta=meta,
                   city_dsm=dsm, city_dsm_view0=one, city_num_points=np.int64(len(cloud)),
                   city_cell_margin=np.float64(cell_margin(cloud, grid)))
        # ---- stage 2 ---------------------------------------------------------------------------------------------------------
        small = np.arange(35, dtype=np.float64).reshape(5, 7)
        out["ds_5x7_in"], out["ds_5x7_out"] = small, dsmr.downsample2x(small[None])[0]
        holes = gnp.make_terrain(101, 102, 31, nan_fraction=0.1)
        holes.reshape(-1)[[5, 500, 5000]] = [np.inf, -np.inf, np.inf]
        out["ds_holes_in"], out["ds_holes_out"] = holes, dsmr.downsample2x(holes[None])[0]
        ref, sec = gnp.shifted_pair(37, 53, 41, 3, -2, 1.0, sec_shape=(40, 49))
        sec.reshape(-1)[[7, 70]] = [np.inf, -np.inf]
        out["ms_ref"], out["ms_sec"] = ref.astype(np.float16), sec.astype(np.float16)
        assert np.array_equal(out["ms_ref"].astype(np.float64), ref, equal_nan=True)
        out["ms_shifts"] = np.array([[0, 0], [3, -2], [-5, 4], [30, 0]])
        out["ms_stats"] = np.array([[float(t) for t in dsmr.mean_std(ref[None], sec[None], int(x), int(y))]
                                    for x, y in out["ms_shifts"]])
        out["as_params"] = np.array([3.0, -2.0, 1.5, 0.25])
        out["as_out"] = dsmr.apply_shift_(sec[None], np.zeros_like(sec[None]), 3, -2, 1.5, 0.25, 0, 0)[0]
        for tag, case in registration_cases().items():
            for name in ("ref", "sec"):
                half = case[name].astype(np.float16)
                assert np.array_equal(half.astype(np.float64), case[name], equal_nan=True), (tag, name)
                out[f"reg_{tag}_{name}"] = half
            dx, dy, a, b, stats, margins = run_registration(dsmr, case)
            assert (margins[:, 0] - margins[:, 1] >= SCORE_MARGIN).all(), (tag, margins)
            out[f"reg_{tag}_params"] = np.array([case["irange"], int(case["scaling"]), *case["init"]])
            out[f"reg_{tag}_shift"] = np.array([dx, dy])
            out[f"reg_{tag}_ab"] = np.array([a, b])
            out[f"reg_{tag}_stats"] = stats
            out[f"reg_{tag}_margins"] = margins
            print(f"reg_{tag}: shift ({dx}, {dy}) a {a:.6g} b {b:.6g} margins {margins.tolist()}", flush=True)
        # ---- stage 3 ---------------------------------------------------------------------------------------------------------
        pred_inf, gt = sec[:37, :49].copy(), ref[:, :49].copy()
        assert np.isinf(pred_inf).sum() == 2
        pred = np.where(np.isinf(pred_inf), np.nan, pred_inf)
        keep = np.random.default_rng(5).random(pred.shape) > 0.2
        r = egg.compute_dsm_metrics(pred_inf, gt, None)           # an infinite height is "valid" (~isnan): it counts
        out["met_inf"] = np.array([r["mae"], r["rmse"], r["valid_pixels"], r["completeness"]], dtype=np.float64)
        out["met_pred_inf"] = pred_inf.astype(np.float16)
        for tag, m in (("plain", None), ("masked", keep)):
            r = egg.compute_dsm_metrics(pred, gt, m)
            out[f"met_{tag}"] = np.array([r["mae"], r["rmse"], r["valid_pixels"], r["completeness"]], dtype=np.float64)
        r = egg.compute_dsm_metrics(np.full_like(pred, np.nan), gt, None)
        out["met_none"] = np.array([r["mae"], r["rmse"], r["valid_pixels"], r["completeness"]], dtype=np.float64)
        out["met_pred"], out["met_gt"], out["met_keep"] = pred.astype(np.float16), gt.astype(np.float16), keep
        out["met_dz"] = np.float64(egg.register_dsms_simple(pred, gt)[1])
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert set(old.files) == set(out), set(old.files) ^ set(out)
        for k in out:
            np.testing.assert_array_equal(old[k], out[k], err_msg=k)
        print("reference_geometry.npz reproduced exactly")
        return
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
