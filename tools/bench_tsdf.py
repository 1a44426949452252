#!/usr/bin/env python
"""TSDF fusion and mesh extraction alone: sfgs.tsdf.TsdfVolume (csrc/tsdf.hip) on the scene of tools/bench_geometry.py: 24 depth
maps of 1024 x 1024 of a 512 m terrain, fused into 512 x 512 x 128 voxels of 1 m (truncation 3 voxels).

  (a) add_views against the numpy restatement (tests/tsdf_np.py) on the same box in the same run, on the first RESTATE_VIEWS views
      (the restatement holds some twenty float64 arrays of 33.5 M voxels per view: all 24 views would take minutes of host time
      that measure nothing new). Host: the host clock, the depth maps already downloaded. Device: events around the call. The
      two volumes must be the same bytes.
  (b) the batch: ONE launch for all 24 views against 24 launches of one view, alternating, ROUNDS times after a warm-up; events
      around the calls (the wrapper's table upload included: it is part of a call). The two volumes must be the same bytes.
  (c) --variant LIB: a second build of libsfgs.so whose integrate kernel has the other voxel-to-lane layout (tools/variants/
      tsdf_run_x.patch through tools/build_variant.sh: a workgroup is a run of 256 voxels along x instead of a brick of
      8 x 8 x 4). sfgs_tsdf_integrate of both libraries on the same table, alternating; the volumes must be the same bytes.
  (d) extract alone, on the fused volume: events around the three launches.
  (e) the integrate kernel's share of the 8 TB/s roofline in ALGORITHMIC bytes: the volume's tsdf and weight read once (8 bytes a
      voxel), the updated voxels written once (8 bytes each), every depth map read once (4 bytes a pixel). The gathers the kernel
      really makes (4 bytes for each (voxel, view) pair that reaches a depth map) are reported next to it.
Exits with status 1 unless every comparison of bytes holds and add_views is faster than the restatement.

usage: python tools/bench_tsdf.py [--variant LIB] [--out FILE]      env: ROUNDS=3 VIEWS=24 SIZE=1024 CELLS=1024 RESTATE_VIEWS=2 DIMS=512,512,128"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_geometry as bg  # noqa: E402
import consistency_np as cnp  # noqa: E402
import geometry_np as gnp  # noqa: E402
import tsdf_np as tnp  # noqa: E402
from sfgs import _lib as L  # noqa: E402
from sfgs.tsdf import TsdfVolume  # noqa: E402

ROUNDS = bg.ROUNDS
RESTATE_VIEWS = int(os.environ.get("RESTATE_VIEWS", 2))
DIMS = tuple(int(v) for v in os.environ.get("DIMS", "512,512,128").split(","))
HBM_BYTES_PER_S = 8.0e12


def device_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return out, start.elapsed_time(end)


def med(xs):
    return float(np.median(xs))


def equal_state(a, b):
    return bool(torch.equal(a.tsdf.view(torch.int32), b.tsdf.view(torch.int32)) and
                torch.equal(a.weight.view(torch.int32), b.weight.view(torch.int32)))


def raw_integrate(lib_path, vol, table, V):
    """-> run(): sfgs_tsdf_integrate of the library at lib_path on vol's buffers and the device table"""
    lib = L.C.CDLL(lib_path)
    fn = lib.sfgs_tsdf_integrate
    fn.restype, fn.argtypes = L.SYMBOLS["sfgs_tsdf_integrate"]
    block = vol._struct()
    stream = L.C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        rc = fn(L.C.byref(block), L.ptr(table), V, stream)
        assert rc == 0, rc
    return run


def device_table(vol, depths, cams):
    """The table add_views uploads, built here once so that (c) times the launch alone; it points into `depths`"""
    from sfgs.geometry import _check_view
    records = (L.SfgsTsdfView * len(depths))()
    for k, (d, cam) in enumerate(zip(depths, cams)):
        H, W, (M, c, _, cx_pix, cy_pix, fx, fy) = _check_view(vol.device, d, cam.R, cam.T, cam.focal_x, cam.focal_y, cam.cx, cam.cy,
                                                              None, None, centre_from_view=True)
        records[k] = L.SfgsTsdfView(d.data_ptr(), None, None, H, W, M, c, cx_pix, cy_pix, fx, fy)
    L.check(L.load().sfgs_tsdf_table_check(records, len(depths), 0))
    return torch.frombuffer(bytearray(bytes(records)), dtype=torch.uint8).cuda()


def main():
    variant = sys.argv[sys.argv.index("--variant") + 1] if "--variant" in sys.argv else None
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    _, cams, depths, _, _ = bg.make_case()
    V, (H, W) = len(depths), depths[0].shape
    terrain = gnp.make_terrain(bg.CELLS, bg.CELLS, 2024, boxes=60)
    side = bg.CELLS * bg.RES
    nx, ny, nz = DIMS
    voxel = side / nx
    spec = tnp.Volume(origin=(0.0, 0.0, float(np.floor(terrain.min())) - 8.0 * voxel), dims=DIMS, voxel_size=voxel, trunc=3.0 * voxel,
                      max_weight=64.0)
    nvox = nx * ny * nz

    def new_volume():
        return TsdfVolume(spec.origin, spec.dims, spec.voxel_size, spec.trunc, max_weight=spec.max_weight, device="cuda")

    # (a)
    n_a = max(1, min(RESTATE_VIEWS, V))
    host_views = [cnp.View(d.cpu().numpy(), c, None) for d, c in zip(depths[:n_a], cams[:n_a])]
    vol_a = new_volume()
    vol_a.add_views(depths[:n_a], cams[:n_a])                                  # warm-up
    vol_a.reset()
    torch.cuda.synchronize()
    _, dev_ms_a = device_ms(lambda: vol_a.add_views(depths[:n_a], cams[:n_a]))
    state, counters = tnp.empty_state(spec.dims), {}
    t0 = time.perf_counter()
    tnp.integrate(state, spec, host_views, None, counters)
    host_s = time.perf_counter() - t0
    equal_a = bool((vol_a.tsdf.cpu().numpy().view(np.uint32) == state.tsdf.view(np.uint32)).all() and
                   (vol_a.weight.cpu().numpy().view(np.uint32) == state.weight.view(np.uint32)).all())
    del state, host_views

    # (b)
    batched, single = new_volume(), new_volume()
    ms_batched, ms_single = [], []
    for r in range(ROUNDS + 1):                                               # the first round warms both up
        batched.reset()
        single.reset()
        torch.cuda.synchronize()
        _, a = device_ms(lambda: batched.add_views(depths, cams))
        _, b = device_ms(lambda: [single.add_view(d, c) for d, c in zip(depths, cams)])
        if r:
            ms_batched.append(a)
            ms_single.append(b)
    equal_b = equal_state(batched, single)
    updated = int((batched.weight > 0).sum().item())

    # (c)
    forms = None
    if variant:
        table = device_table(batched, depths, cams)
        vols = {"a": new_volume(), "b": new_volume()}
        runs = {"a": raw_integrate(L.LIB_PATH, vols["a"], table, V), "b": raw_integrate(variant, vols["b"], table, V)}
        times = {"a": [], "b": []}
        for r in range(max(ROUNDS, 5) + 1):
            for k in "ab":
                vols[k].reset()
                torch.cuda.synchronize()
                _, ms = device_ms(runs[k])
                if r:
                    times[k].append(ms)
        forms = {"committed_brick_8x8x4_ms": times["a"], "variant_run_x_ms": times["b"], "variant": os.path.basename(variant),
                 "committed_over_variant": med(times["a"]) / med(times["b"]),
                 "committed_faster_in_every_round": all(x < y for x, y in zip(times["a"], times["b"])),
                 "outputs_equal": equal_state(vols["a"], vols["b"]) and equal_state(vols["a"], batched)}
        kernel_ms = med(times["a"])
    else:
        kernel_ms = med(ms_batched)

    # (d)
    capacity = 16 * nx * ny
    batched.extract(capacity)
    torch.cuda.synchronize()
    ms_extract, found = [], 0
    for _ in range(ROUNDS):
        soup, ms = device_ms(lambda: batched.extract(capacity))
        ms_extract.append(ms)
        found = int(soup.num_triangles)

    # (e)
    algorithmic = 8 * nvox + 8 * updated + 4 * V * H * W
    pairs = V * nvox
    result = {
        "tool": "bench_tsdf", "views": V, "depth_size": [H, W], "dims": list(DIMS), "voxel_size": voxel, "trunc": spec.trunc,
        "gpu": torch.cuda.get_device_name(0),
        "a_add_views_against_restatement": {
            "views": n_a, "device_ms": dev_ms_a, "host_s": host_s, "host_over_device": host_s * 1e3 / dev_ms_a,
            "equal_bytes": equal_a, "outcomes": counters},
        "b_batch": {"one_launch_ms": ms_batched, "one_launch_per_view_ms": ms_single, "median_one_launch_ms": med(ms_batched),
                    "median_one_launch_per_view_ms": med(ms_single), "per_view_over_batched": med(ms_single) / med(ms_batched),
                    "equal_bytes": equal_b, "voxels_updated": updated, "voxels": nvox},
        "c_lane_layouts": forms,
        "d_extract": {"ms": ms_extract, "median_ms": med(ms_extract), "triangles": found, "capacity": capacity,
                      "cells": (nx - 1) * (ny - 1) * (nz - 1), "cells_per_second": (nx - 1) * (ny - 1) * (nz - 1) / (med(ms_extract) * 1e-3)},
        "e_roofline": {"integrate_ms": kernel_ms, "timed_as": "raw launch (c)" if variant else "add_views (b), wrapper included",
                       "algorithmic_bytes": algorithmic, "algorithmic_GB_per_s": algorithmic / (kernel_ms * 1e-3) / 1e9,
                       "share_of_8_TB_per_s": algorithmic / (kernel_ms * 1e-3) / HBM_BYTES_PER_S,
                       "pairs": pairs, "pairs_per_second": pairs / (kernel_ms * 1e-3), "gather_bytes_upper_bound": 4 * pairs},
        "baseline": "vectorised numpy restatement (tests/tsdf_np.py), float64, depth maps already on the host",
    }
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    ok = equal_a and equal_b and dev_ms_a < host_s * 1e3 and (forms is None or forms["outputs_equal"])
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
