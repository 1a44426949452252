#!/usr/bin/env python
"""Merged point cloud alone: sfgs.pointcloud (depth maps -> one float64 cloud on the device, its count and bounds) against the
host spelling of the same stage, at the evaluation's own size: 24 depth maps of 1024 x 1024 of tests/geometry_np.city_views'
seeded scene (its terrain, cameras and UTM origin; its ray march runs on the device here -- set-up, not timed).

The yardstick is the host spelling, not the code under test: per view `depth.cpu().numpy()` and the vectorised float64
restatement tests/geometry_np.unproject (a meshgrid-free spelling of the reference's depth_to_point_cloud), then np.vstack
over the views -- the stage that reads 0.349 s in profiles/r10_geometry_ab.txt. The device side is 24 add_view calls,
result() (its one host read: the count) and bounds(), ending in a synchronise. Both run in one process, alternating, ROUNDS
times after a warm-up, each under the host clock. The tool checks that the device rows and bounds equal the host's bit for
bit and exits with status 1 unless they do and the device side is faster in every round.

Also printed, from a pass of its own under torch.profiler: every kernel's launches and device time per launch, the bytes the
algorithm has to move per launch (depth and mask are read twice -- by the count and by the scatter kernel --, a stored row is
24 bytes, 27 with colours; the bounds read the rows once) and that many bytes over the kernel's time as a share of 8 TB/s.

usage: python tools/bench_pointcloud.py [--out FILE]      env: ROUNDS=3 VIEWS=24 SIZE=1024 CELLS=512"""
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_np as gnp  # noqa: E402
from sfgs import pointcloud  # noqa: E402

ROUNDS, VIEWS = int(os.environ.get("ROUNDS", 3)), int(os.environ.get("VIEWS", 24))
SIZE, CELLS = int(os.environ.get("SIZE", 1024)), int(os.environ.get("CELLS", 512))
SEED = 2024
ROOF_TBS = 8.0
PC_THREADS = 256      # csrc/pointcloud.hip: pixels per workgroup (one 8-byte count each)


def render_depth_device(terrain, res, cam, H, W, steps=192, reach=(0.5, 1.6)):
    """gnp.render_depth with the ray march on the device -> float32 [H,W] on the GPU (set-up, not timed)"""
    rows, cols = terrain.shape
    t = torch.from_numpy(np.nan_to_num(terrain, nan=0.0)).cuda()
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device="cuda"), torch.arange(W, dtype=torch.float64, device="cuda"),
                          indexing="ij")
    dirs = torch.stack([(u - gnp.pixel_centre(cam.cx, W)) / cam.focal_x, (v - gnp.pixel_centre(cam.cy, H)) / cam.focal_y,
                        torch.ones_like(u)], dim=-1) @ torch.from_numpy(cam.axes).cuda().T
    centre = torch.from_numpy(cam.centre).cuda()
    dist = float(np.linalg.norm(cam.centre - np.array([cols * res / 2, rows * res / 2, 0.0])))
    depth = torch.zeros((H, W), dtype=torch.float64, device="cuda")
    for z in np.linspace(reach[0] * dist, reach[1] * dist, steps):
        p = centre + dirs * z
        gx, gy = torch.floor(p[..., 0] / res).long(), torch.floor((rows * res - p[..., 1]) / res).long()
        inside = (gx >= 0) & (gx < cols) & (gy >= 0) & (gy < rows)
        hit = (depth == 0) & inside & (p[..., 2] <= t[gy.clamp(0, rows - 1), gx.clamp(0, cols - 1)])
        depth = torch.where(hit, torch.full_like(depth, z), depth)
    return depth.float()


def make_case():
    own = gnp.render_depth
    gnp.render_depth = render_depth_device                 # city_views' scene and cameras, its depth maps made on the device
    try:
        _, _, cams, depths, origin = gnp.city_views(VIEWS, SIZE, SIZE, SEED, cells=CELLS)
    finally:
        gnp.render_depth = own
    return cams, depths, origin


def host_spelling(cams, depths, origin):
    clouds = [gnp.unproject(d.cpu().numpy(), c.R, c.T, c.focal_x, c.focal_y, c.cx, c.cy, origin=origin) for d, c in zip(depths, cams)]
    return np.vstack(clouds)


def device_side(pc, cams, depths, origin):
    pc.reset()
    for d, c in zip(depths, cams):
        pc.add_view(d, c, origin=origin)
    points, _ = pc.result()                               # the one host read: the count
    bounds = pc.bounds()
    torch.cuda.synchronize()
    return points, bounds


def kernel_table(fn, per_launch_bytes):
    """Every device activity of one call of fn: launches, device us per launch (torch.profiler), algorithmic bytes per launch"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    table = {}
    for e in prof.key_averages():
        if e.device_time_total <= 0:
            continue
        us = e.device_time_total / e.count
        name = re.sub(r"\(.*", "", e.key).replace("void ", "").replace("sfgs::", "")[:60]
        nbytes = next((b for k, b in per_launch_bytes if k in e.key), None)
        while name in table:                               # never fold two profiler rows into one
            name += "'"
        row = {"launches": e.count, "us_per_launch": round(us, 2), "algorithmic_bytes_per_launch": nbytes}
        if nbytes:
            tbs = nbytes / (us * 1e-6) / 1e12
            row.update(TB_per_s=round(tbs, 3), share_of_8_TB_per_s=round(tbs / ROOF_TBS, 4))
        table[name] = row
    return table


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cams, depths, origin = make_case()
    P = SIZE * SIZE
    pc = pointcloud.PointCloud(VIEWS * P, device="cuda")
    for _ in range(2):
        points, bounds = device_side(pc, cams, depths, origin)
    rounds = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        points, bounds = device_side(pc, cams, depths, origin)
        t1 = time.perf_counter()
        want = host_spelling(cams, depths, origin)
        t2 = time.perf_counter()
        rounds.append({"device_s": t1 - t0, "host_s": t2 - t1})
    n = len(want)
    got = points.cpu().numpy()
    rows_equal = got.shape == want.shape and bool(np.array_equal(got.view(np.uint64), (want + 0.0).view(np.uint64)))
    bounds_equal = bool(np.array_equal(bounds.cpu().numpy(), np.stack([want.min(0), want.max(0)])))
    faster = all(r["device_s"] < r["host_s"] for r in rounds)
    nblk = -(-P // PC_THREADS)
    rows_per_view = n / VIEWS                              # mean over the views: a launch's share of the stored rows
    need = (("pc_count_kernel", 4 * P + 8 * nblk), ("scan_sums_kernel", None),
            ("pc_scatter_kernel", int(4 * P + 8 * nblk + 24 * rows_per_view)), ("pc_bounds_kernel", 24 * n),
            ("pc_bounds_final_kernel", None))
    kernels = kernel_table(lambda: device_side(pc, cams, depths, origin), need)
    med = lambda xs: float(np.median(xs))
    result = {
        "tool": "bench_pointcloud", "views": VIEWS, "depth_size": [SIZE, SIZE], "terrain_cells": [CELLS, CELLS], "seed": SEED,
        "gpu": torch.cuda.get_device_name(0), "points": n, "used_pixel_fraction": n / (VIEWS * P), "rounds": rounds,
        "median_device_s": med([r["device_s"] for r in rounds]), "median_host_s": med([r["host_s"] for r in rounds]),
        "ratio_of_medians": med([r["host_s"] for r in rounds]) / med([r["device_s"] for r in rounds]),
        "device_faster_in_every_round": faster, "rows_bit_equal": rows_equal, "bounds_equal": bounds_equal,
        "bounds": bounds.cpu().tolist(),
        "kernels": kernels,
        "algorithmic_bytes": "no mask, no colours: count = 4 P + 8 per workgroup; scatter = 4 P + 8 per workgroup + 24 per stored row "
                             "(mean over the views); bounds = 24 per stored row; share = bytes / time / 8 TB/s",
        "device_side": "reset, 24 add_view (3 launches each), result() (one host read: the count), bounds() (2 launches), synchronise",
        "baseline": "per view depth.cpu().numpy() + tests/geometry_np.unproject (vectorised float64), then np.vstack: the stage "
                    "download_unproject_stack of profiles/r10_geometry_ab.txt",
    }
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    sys.exit(0 if faster and rows_equal and bounds_equal else 1)


if __name__ == "__main__":
    main()
