#!/usr/bin/env python
"""Geometry evaluation alone: the device chain of sfgs.geometry (depth maps -> DSM -> dsmr registration -> metrics, ONE host
read) against the host spelling of the same chain, at the evaluation's own size: 24 depth maps of 1024 x 1024 scattered into
a grid of 1024 x 1024 cells of 0.5 m, registered against a synthetic truth (the terrain the depth maps were rendered from,
moved by a known shift and offset, with holes).

The host spelling is the vectorised numpy restatement of tests/geometry_np.py, fed the way the reference feeds its own
functions: every depth map is downloaded, unprojected in float64, the clouds are stacked and flattened, then registered and
compared. Two facts about this baseline, printed with the result:
  * the reference's own dsmr.py needs numba, which is not installed here; run as plain Python it takes seconds for a
    110 x 130 pair, so it is not timed;
  * the reference's fallback flattening is a per-point Python loop; the vectorised np.maximum.at used here is faster than
    that loop, so the baseline is not the reference's slowest path either.
Both sides run in one process, alternating, ROUNDS times after a warm-up; the device time is the host clock around the whole
chain INCLUDING its single host read. Each stage is also timed on its own (device: host clock with a synchronise around the
stage). The tool checks that both sides find the same shift and the same valid-pixel count, and exits with status 1 unless
the device chain is faster than the host spelling in every round.

usage: python tools/bench_geometry.py [--out FILE]      env: ROUNDS=3 VIEWS=24 SIZE=1024 CELLS=1024"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_np as gnp  # noqa: E402
from sfgs import geometry as geo  # noqa: E402

ROUNDS, VIEWS = int(os.environ.get("ROUNDS", 3)), int(os.environ.get("VIEWS", 24))
SIZE, CELLS = int(os.environ.get("SIZE", 1024)), int(os.environ.get("CELLS", 1024))
RES = 0.5
ORIGIN = np.array([4.0e5, 3.3e6, 20.0])
TRUE_SHIFT = (6, -9, 1.75)


def render_depth_device(terrain, cam, H, W, steps=256, reach=(0.6, 1.5)):
    """gnp.render_depth on the device (set-up, not timed): march every pixel's ray through the height field"""
    rows, cols = terrain.shape
    dev = terrain.device
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev),
                          indexing="ij")
    axes = torch.from_numpy(cam.axes).to(dev)
    centre = torch.from_numpy(cam.centre).to(dev)
    dirs = torch.stack([(u - gnp.pixel_centre(cam.cx, W)) / cam.focal_x, (v - gnp.pixel_centre(cam.cy, H)) / cam.focal_y,
                        torch.ones_like(u)], dim=-1) @ axes.T
    dist = float(np.linalg.norm(cam.centre - np.array([cols * RES / 2, rows * RES / 2, 0.0])))
    depth = torch.zeros((H, W), dtype=torch.float64, device=dev)
    for z in np.linspace(reach[0] * dist, reach[1] * dist, steps):
        p = centre + dirs * z
        gx, gy = torch.floor(p[..., 0] / RES).long(), torch.floor((rows * RES - p[..., 1]) / RES).long()
        inside = (gx >= 0) & (gx < cols) & (gy >= 0) & (gy < rows)
        ground = terrain[gy.clamp(0, rows - 1), gx.clamp(0, cols - 1)]
        hit = (depth == 0) & inside & (p[..., 2] <= ground)
        depth = torch.where(hit, torch.full_like(depth, z), depth)
    return depth.float()


def make_case():
    terrain = gnp.make_terrain(CELLS, CELLS, 2024, boxes=60)
    side = CELLS * RES
    target = np.array([side / 2, side / 2, 12.0])
    t_dev = torch.from_numpy(terrain).cuda()
    cams, depths = [], []
    for k in range(VIEWS):
        cam = gnp.look_down_camera(target, 62.0 + 3.0 * (k % 3), 360.0 * k / VIEWS + 11.0, 3.0 * side, focal=2.6 * SIZE,
                                   cx=0.02 * (k % 2), cy=-0.01 * (k % 3))
        cams.append(cam)
        depths.append(render_depth_device(t_dev, cam, SIZE, SIZE))
    rng = np.random.default_rng(7)
    dx, dy, dz = TRUE_SHIFT
    gt = np.roll(terrain, (-dy, -dx), axis=(0, 1)) + ORIGIN[2] + dz + rng.normal(0, 0.05, terrain.shape)
    gt[rng.random(gt.shape) < 0.05] = np.nan
    keep = rng.random(gt.shape) > 0.03                            # "not water"
    grid = geo.DsmGrid(ORIGIN[0], ORIGIN[1] + side, CELLS, CELLS, RES)
    return grid, cams, depths, gt, keep


def host_chain(grid, cams, depths, gt, keep, split):
    t0 = time.perf_counter()
    clouds = [gnp.unproject(d.cpu().numpy(), c.R, c.T, c.focal_x, c.focal_y, c.cx, c.cy, origin=ORIGIN) for d, c in zip(depths, cams)]
    cloud = np.vstack(clouds)
    t1 = time.perf_counter()
    pred, n = gnp.dsm_max(cloud, tuple(grid))
    pred = np.where(keep, pred, np.nan)
    t2 = time.perf_counter()
    dx, dy, a, b, _ = gnp.compute_shift(gt, pred, 5, False)
    t3 = time.perf_counter()
    m = gnp.dsm_metrics(pred, gt, keep, shift=(dx, dy, a, b))
    t4 = time.perf_counter()
    split.append({"download_unproject_stack": t1 - t0, "flatten_max": t2 - t1, "register": t3 - t2, "shift_compare": t4 - t3})
    return {"mae": float(m["mae"]), "rmse": float(m["rmse"]), "valid_pixels": int(m["valid_pixels"]),
            "completeness": float(m["completeness"]), "dx_offset": dx, "dy_offset": dy, "dz_offset": float(b), "total_points": n}


def device_stages(grid, cams, depths, gt_d, keep_d):
    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t

    def scatter():
        acc = geo.DsmAccumulator(grid, device=gt_d.device)
        for d, c in zip(depths, cams):
            acc.add_view(d, c, origin=ORIGIN)
        return torch.where(keep_d, acc.result(), torch.full_like(gt_d, float("nan")))
    pred, t_acc = timed(scatter)
    shift, t_reg = timed(lambda: geo.register(gt_d, pred))
    _, t_met = timed(lambda: geo.dsm_metrics(pred, gt_d, shift=shift, mask=keep_d))
    return {"scatter_24_views_finalize": t_acc, "register": t_reg, "shift_compare": t_met}


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    grid, cams, depths, gt, keep = make_case()
    gt_d, keep_d = torch.from_numpy(gt).cuda(), torch.from_numpy(keep).cuda()
    device = lambda: geo.evaluate_dsm(depths, cams, grid, gt_d, origin=ORIGIN, keep_mask=keep_d)
    for _ in range(2):
        got = device()
    rounds, host_split, dev_split = [], [], []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = device()                                            # ends with its host read
        t1 = time.perf_counter()
        want = host_chain(grid, cams, depths, gt, keep, host_split)
        t2 = time.perf_counter()
        rounds.append({"device_s": t1 - t0, "host_s": t2 - t1})
        dev_split.append(device_stages(grid, cams, depths, gt_d, keep_d))
    same = all(got[k] == want[k] for k in ("dx_offset", "dy_offset", "valid_pixels", "total_points", "completeness"))
    close = all(abs(got[k] - want[k]) <= 1e-9 * max(1.0, abs(want[k])) for k in ("mae", "rmse", "dz_offset"))
    faster = all(r["device_s"] < r["host_s"] for r in rounds)
    med = lambda xs: float(np.median(xs))
    result = {
        "tool": "bench_geometry", "views": VIEWS, "depth_size": [SIZE, SIZE], "grid_cells": [CELLS, CELLS], "resolution_m": RES,
        "gpu": torch.cuda.get_device_name(0), "rounds": rounds,
        "median_device_s": med([r["device_s"] for r in rounds]), "median_host_s": med([r["host_s"] for r in rounds]),
        "ratio_of_medians": med([r["host_s"] for r in rounds]) / med([r["device_s"] for r in rounds]),
        "device_faster_in_every_round": faster,
        "device_stage_median_s": {k: med([s[k] for s in dev_split]) for k in dev_split[0]},
        "host_stage_median_s": {k: med([s[k] for s in host_split]) for k in host_split[0]},
        "device_result": got, "host_result": want, "integers_equal": same, "floats_within_1e-9": close,
        "true_shift_dx_dy_dz": list(TRUE_SHIFT),
        "baseline": "vectorised numpy restatement (tests/geometry_np.py), float64, depth maps downloaded per view",
        "not_timed": "the reference's dsmr.py needs numba (not installed); its fallback flattening is a per-point Python loop: "
                     "neither is a fair baseline, the numpy spelling is faster than both",
    }
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    sys.exit(0 if faster and same and close else 1)


if __name__ == "__main__":
    main()
