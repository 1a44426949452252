#!/usr/bin/env python
"""True orthophoto alone: sfgs.ortho (rendered views -> colour, height, source per DSM cell on the device) at the evaluation's
own size: 24 views of 1024 x 1024 of tests/geometry_np.city_views' seeded scene into 1024 x 1024 cells (its terrain, cameras
and UTM origin; its ray march runs on the device here and the images are seeded noise -- set-up, not timed).

Four measurements, every pair in ONE process, alternating, ROUNDS times after a warm-up:
  1. the whole accumulation -- reset, 24 add_view, result(fill=0), synchronise -- against the numpy spelling of the same thing
     (per view depth.cpu(), image.cpu(), then tests/ortho_np.keys and resolve), both under the host clock. The tool checks that
     the five outputs equal the numpy spelling's bit for bit and exits with status 1 unless they do and the device side is
     faster in every round. The factor is reported, not promised.
  2. add_view per view against DsmAccumulator(mode="max").add_view on the same views (device events around the 24 calls, the
     accumulator emptied before each round). The DSM kernel is the yardstick: the same unprojection and cell rule, one 64-bit
     atomic max per landed point, 5 bytes read per pixel with a mask (4 without) where the orthophoto reads 12 more. The
     allowance is the yardstick's time + those 12 bytes per pixel at the rate sfgs.metrics' streaming kernel reaches at this
     size (STREAM_TBS, profiles/r12_metrics_ab.txt) + the yardstick's own round-to-round spread (max - min over the rounds).
  3. --variant LIB: a second build of libsfgs.so whose accumulate kernel has the other form (tools/variants/
     ortho_no_preread.patch through tools/build_variant.sh). sfgs_ortho_accumulate of both libraries on the same 24 prepared
     argument blocks, device events, alternating; the accumulators must end bit-identical.
  4. every kernel's device time per launch under torch.profiler, a pass of its own: the two accumulate kernels, and the resolve
     kernel at fill 0 and at fill 3.

usage: python tools/bench_ortho.py [--variant LIB] [--out FILE]      env: ROUNDS=5 VIEWS=24 SIZE=1024 CELLS=1024"""
import ctypes as C
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
import geometry_np as gnp  # noqa: E402
import ortho_np as onp  # noqa: E402
from bench_pointcloud import kernel_table, render_depth_device  # noqa: E402
from sfgs import _call, geometry, ortho  # noqa: E402
from sfgs import _lib as L  # noqa: E402

ROUNDS, VIEWS = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("VIEWS", 24))
SIZE, CELLS = int(os.environ.get("SIZE", 1024)), int(os.environ.get("CELLS", 1024))
SEED = 2024
STREAM_TBS = 4.2      # metrics_stream_kernel at 1024 x 1024: 4.2 - 4.3 TB/s of algorithmic bytes (profiles/r12_metrics_ab.txt)
FIELDS = ("rgb", "height", "source", "state", "coverage")


def make_case():
    own = gnp.render_depth
    gnp.render_depth = render_depth_device                 # city_views' scene and cameras, its depth maps made on the device
    try:
        grid, _, cams, depths, origin = gnp.city_views(VIEWS, SIZE, SIZE, SEED, cells=CELLS)
    finally:
        gnp.render_depth = own
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    images = [torch.rand((3, SIZE, SIZE), generator=gen, device="cuda") * 1.2 - 0.1 for _ in depths]
    return geometry.DsmGrid(*grid), cams, depths, images, origin


def numpy_spelling(grid, cams, depths, images, origin):
    views = [onp.View(d.cpu().numpy(), i.cpu().numpy(), c, None, k + 1) for k, (d, i, c) in enumerate(zip(depths, images, cams))]
    acc, n = onp.keys(views, tuple(grid), origin)
    return onp.resolve(acc, 0), n


def device_side(o, cams, depths, images, origin):
    o.reset()
    for d, i, c in zip(depths, images, cams):
        o.add_view(d, i, c, origin=origin)
    res = o.result(fill=0)
    torch.cuda.synchronize()
    return res


def timed_views(reset, add):
    """-> microseconds per view: device events around the VIEWS calls of add(k), the accumulator emptied first"""
    reset()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for k in range(VIEWS):
        add(k)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / VIEWS


def stats(xs):
    return {"median": round(float(np.median(xs)), 2), "min": round(min(xs), 2), "max": round(max(xs), 2),
            "rounds": [round(x, 2) for x in xs]}


def raw_accumulate(lib_path, grid, cams, depths, images, origin, acc, num):
    """-> add(k) calling sfgs_ortho_accumulate of the library at lib_path on prepared argument blocks"""
    lib = C.CDLL(lib_path)
    fn = lib.sfgs_ortho_accumulate
    fn.restype, fn.argtypes = L.SYMBOLS["sfgs_ortho_accumulate"]
    dev = depths[0].device
    blocks = []
    for k, (d, i, c) in enumerate(zip(depths, images, cams)):
        H, W, cam = geometry._check_view(dev, d, c.R, c.T, c.focal_x, c.focal_y, c.cx, c.cy, origin, None, image=i)
        blocks.append(L.SfgsOrthoViewArgs(C.sizeof(L.SfgsOrthoViewArgs), H, W, d.data_ptr(), None, *cam, grid.xoff, grid.yoff_top,
                                          grid.resolution, grid.xsize, grid.ysize, i.data_ptr(), k + 1))
    stream = _call.stream(dev)

    def add(k):
        rc = fn(C.byref(blocks[k]), L.ptr(acc), L.ptr(num), stream)
        if rc:
            raise RuntimeError(f"{lib_path}: sfgs_ortho_accumulate -> {rc}")
    return add


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    variant = sys.argv[sys.argv.index("--variant") + 1] if "--variant" in sys.argv else None
    grid, cams, depths, images, origin = make_case()
    P = SIZE * SIZE
    o = ortho.OrthoAccumulator(grid, device="cuda")
    dsm = geometry.DsmAccumulator(grid, mode="max", device="cuda")
    for _ in range(2):
        res = device_side(o, cams, depths, images, origin)

    # 1. the whole accumulation against the numpy spelling
    whole = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = device_side(o, cams, depths, images, origin)
        t1 = time.perf_counter()
        want, n = numpy_spelling(grid, cams, depths, images, origin)
        t2 = time.perf_counter()
        whole.append({"device_s": t1 - t0, "host_s": t2 - t1})
    got = {f: getattr(res, f).cpu().numpy() for f in FIELDS}
    equal = {f: bool(np.array_equal(got[f].view(np.uint32) if f == "height" else got[f],
                                    getattr(want, f).view(np.uint32) if f == "height" else getattr(want, f))) for f in FIELDS}
    equal["num_points"] = int(o.num_points) == n
    faster = all(r["device_s"] < r["host_s"] for r in whole)
    med = lambda xs: float(np.median(xs))

    # 2. per view against the DSM's accumulate kernel, the yardstick repeated for its own spread
    def dsm_reset():
        dsm._acc.zero_()
        dsm._num.zero_()
    add_ortho = lambda k: o.add_view(depths[k], images[k], cams[k], origin=origin, tag=k + 1)
    add_dsm = lambda k: dsm.add_view(depths[k], cams[k], origin=origin)
    for _ in range(2):
        timed_views(o.reset, add_ortho), timed_views(dsm_reset, add_dsm)
    t_ortho, t_dsm = [], []
    for r in range(ROUNDS):
        pair = [(t_ortho, o.reset, add_ortho), (t_dsm, dsm_reset, add_dsm)]
        for into, reset, add in (pair if r % 2 == 0 else pair[::-1]):
            into.append(timed_views(reset, add))
    dsm_heights_equal = bool(torch.equal(dsm.result().to(torch.float32).view(torch.int32), o.result().height.view(torch.int32)))
    extra_us = 12 * P / (STREAM_TBS * 1e12) * 1e6
    spread_us = max(t_dsm) - min(t_dsm)
    allowance_us = med(t_dsm) + extra_us + spread_us
    per_view = {"add_view_us": stats(t_ortho), "dsm_add_view_us": stats(t_dsm), "ratio_of_medians": round(med(t_ortho) / med(t_dsm), 3),
                "extra_bytes_per_pixel": 12, "stream_TB_per_s": STREAM_TBS, "extra_bytes_us": round(extra_us, 2),
                "yardstick_spread_us": round(spread_us, 2), "allowance_us": round(allowance_us, 2),
                "within_allowance": med(t_ortho) <= allowance_us, "float32_dsm_heights_equal": dsm_heights_equal}

    # 3. the two forms of the accumulate kernel
    forms = None
    if variant:
        acc_a, acc_b = torch.zeros_like(o._acc), torch.zeros_like(o._acc)
        num_a, num_b = torch.zeros_like(o._num), torch.zeros_like(o._num)
        add_a = raw_accumulate(L.LIB_PATH, grid, cams, depths, images, origin, acc_a, num_a)
        add_b = raw_accumulate(variant, grid, cams, depths, images, origin, acc_b, num_b)
        reset_a = lambda: (acc_a.zero_(), num_a.zero_())
        reset_b = lambda: (acc_b.zero_(), num_b.zero_())
        for _ in range(2):
            timed_views(reset_a, add_a), timed_views(reset_b, add_b)
        t_a, t_b = [], []
        for r in range(2 * ROUNDS):
            pair = [(t_a, reset_a, add_a), (t_b, reset_b, add_b)]
            for into, reset, add in (pair if r % 2 == 0 else pair[::-1]):
                into.append(timed_views(reset, add))
        forms = {"committed_library_us_per_view": stats(t_a), "variant_library_us_per_view": stats(t_b), "variant": os.path.basename(variant),
                 "committed_over_variant": round(med(t_a) / med(t_b), 3),
                 "committed_faster_in_every_round": all(a < b for a, b in zip(t_a, t_b)),
                 "accumulators_bit_identical": bool(torch.equal(acc_a, acc_b) and torch.equal(num_a, num_b) and torch.equal(acc_a, o._acc))}

    # 4. kernel times
    def one_pass():
        device_side(o, cams, depths, images, origin)
        dsm_reset()
        for k in range(VIEWS):
            add_dsm(k)
    need = (("ortho_accumulate_kernel", 16 * P), ("dsm_accumulate_kernel", 4 * P), ("ortho_resolve_kernel", 17 * grid.xsize * grid.ysize))
    kernels = {"accumulate_and_resolve_fill_0": kernel_table(one_pass, need),
               "resolve_fill_3": kernel_table(lambda: o.result(fill=3), need)}
    cover = got["coverage"]
    result = {
        "tool": "bench_ortho", "views": VIEWS, "view_size": [SIZE, SIZE], "cells": [grid.ysize, grid.xsize], "seed": SEED,
        "gpu": torch.cuda.get_device_name(0), "landed_points": n, "points_per_view": n / VIEWS,
        "cells_filled": int(cover[1:].sum()), "cells_empty": int(cover[0]),
        "whole_accumulation": {"rounds": whole, "median_device_s": med([r["device_s"] for r in whole]),
                               "median_host_s": med([r["host_s"] for r in whole]),
                               "ratio_of_medians": med([r["host_s"] for r in whole]) / med([r["device_s"] for r in whole]),
                               "device_faster_in_every_round": faster, "outputs_bit_equal": equal},
        "per_view": per_view, "accumulate_forms": forms, "kernels": kernels,
        "algorithmic_bytes": "no mask: ortho accumulate = 16 per pixel (depth + three image planes), dsm accumulate = 4 per pixel, the "
                             "accumulator's traffic not counted; resolve = 8 read + 9 written per cell; share = bytes / time / 8 TB/s",
        "device_side": "reset, 24 add_view (1 launch each), result(fill=0) (1 launch + the zeroing of coverage), synchronise",
        "baseline": "per view depth.cpu().numpy() and image.cpu().numpy(), tests/ortho_np.keys (vectorised float64 unprojection, "
                    "np.maximum.at on uint64 keys), then ortho_np.resolve",
    }
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    sys.exit(0 if faster and all(equal.values()) and dsm_heights_equal and (forms is None or forms["accumulators_bit_identical"]) else 1)


if __name__ == "__main__":
    main()
