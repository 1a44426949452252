#!/usr/bin/env python
"""Depth colorisation alone: the reference's spelling of colorize_depth_torch (render_video.py:129-170: download, numpy
where / reciprocal, two np.nanquantile over the frame, a 256-entry colormap lookup in float64, uint8, upload), restated here
with a device tensor in and a device tensor out, against sfgs.depthvis.colorize_depth in both output kinds, at 1080p and
1024^2. The colormap lookup is spelled in numpy on sfgs.depthvis.spectral_table() (the same array operations a matplotlib
colormap call performs on an H x W array), so the tool needs nothing the GPU tests do not need.

The variants run in ONE process, alternating (ROUNDS alternations; REF_ITERS calls of the reference spelling and ITERS calls
of each fused kind per round) after a warm-up; every round is timed on two clocks: device events around the round, and the
host clock around the round including a final synchronise. Also printed: launches per call (torch.profiler: kernels,
memsets and copies with device time), the fused result's equality with the reference spelling on the timed input, and every
kernel of the fused operator (torch.profiler's device time per launch, in a pass of its own) with the bytes the algorithm
needs, counted from shapes, over that time. The tool exits with status 1 unless both fused kinds are faster than the
reference spelling in every round on both clocks.

usage: python tools/bench_depthvis.py            env: ROUNDS=6 ITERS=200 REF_ITERS=3"""
import json
import os
import re
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
from sfgs import _lib as L  # noqa: E402
from sfgs import depthvis  # noqa: E402

ROUNDS, ITERS = int(os.environ.get("ROUNDS", 6)), int(os.environ.get("ITERS", 200))
REF_ITERS = int(os.environ.get("REF_ITERS", 3))
SIZES = ((1080, 1920), (1024, 1024))


_RGBA = np.concatenate([depthvis.spectral_table(), np.ones((256, 1))], axis=1)   # float64 [256,4], as a colormap holds it


def colormap_lookup(x):
    """A 256-entry colormap applied to a float array: float64 RGBA per element; below 0 -> entry 0, 1 and above -> entry
    255, NaN -> zeros."""
    xa = np.array(x, copy=True)
    bad = np.isnan(xa)
    with np.errstate(invalid="ignore"):
        xa *= 256
        xa[xa == 256] = 255
        under, over = xa < 0, xa >= 256
        xa = xa.astype(int)
    xa[under], xa[over], xa[bad] = 0, 255, 0
    rgba = _RGBA.take(xa, axis=0, mode="clip")
    rgba[bad] = 0.0
    return rgba


def reference_spelling(depth_tensor):
    """What the reference's function does per frame for mask=None, normalize=True, cmap='Spectral'."""
    depth = depth_tensor[0].detach().cpu().numpy()
    disp = 1. / np.where(depth > 0, depth, np.nan)
    lo, hi = np.nanquantile(disp, 0.01), np.nanquantile(disp, 0.99)
    colored = colormap_lookup(1.0 - (disp - lo) / (hi - lo))
    colored = (np.nan_to_num(colored, 0).clip(0, 1) * 255).astype(np.uint8)[:, :, :3]
    return (torch.from_numpy(colored).float() / 255.0).permute(2, 0, 1).to(depth_tensor.device)


def synthetic_depth(H, W, seed):
    """A rendered-like depth map: smooth structure, noise, 5 % holes (0 = nothing rendered)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = 60.0 + 25.0 * torch.sin(xx / W * 5.0) + 15.0 * torch.cos(yy / H * 3.0) + 0.5 * torch.randn(H, W, generator=g)
    d[torch.rand(H, W, generator=g) < 0.05] = 0.0
    return d[None].cuda()


def launches_per_call(fn, calls):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_time_total > 0) / calls


def kernel_table(fn, P, u8, calls):
    """Every device activity of `calls` calls of the fused operator: launches per call, device us per launch
    (torch.profiler), the bytes the algorithm needs and that many bytes over the kernel's time."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    need = (("depthvis_hist_kernel", 4 * P), ("depthvis_scan_kernel", None), ("depthvis_color_kernel", 4 * P + (3 * P if u8 else 12 * P)))
    table = {}
    for e in prof.key_averages():
        if e.device_time_total <= 0:
            continue
        us = e.device_time_total / e.count
        name = re.sub(r"\(.*", "", e.key).replace("void ", "").replace("sfgs::", "")[:60]   # keeps the template arguments: the three passes stay apart
        nbytes = next((b for k, b in need if k in e.key), None)
        while name in table:                               # never fold two profiler rows into one
            name += "'"
        table[name] = {"launches_per_call": e.count / calls, "us": round(us, 2), "bytes": nbytes}
    for row in table.values():
        row["TB_per_s"] = round(row["bytes"] / (row["us"] * 1e-6) / 1e12, 3) if row["bytes"] else None
    return table


def bench(H, W):
    depth = synthetic_depth(H, W, H + W)
    variants = {"reference": (lambda: reference_spelling(depth), REF_ITERS),
                "fused_float_chw": (lambda: depthvis.colorize_depth(depth), ITERS),
                "fused_uint8_hwc": (lambda: depthvis.colorize_depth(depth, out="uint8_hwc"), ITERS)}
    out = {"H": H, "W": W, "rounds": ROUNDS, "iters": {k: n for k, (_, n) in variants.items()}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = reference_spelling(depth)
        out["fused_equals_reference"] = bool(torch.equal(depthvis.colorize_depth(depth).view(torch.int32), want.view(torch.int32))
                                             and torch.equal(depthvis.colorize_depth(depth, out="uint8_hwc"),
                                                             (want * 255.0).round().to(torch.uint8).permute(1, 2, 0)))
        for name, (fn, n) in variants.items():             # warm-up + launches per call
            for _ in range(3 if name == "reference" else 30):
                fn()
            torch.cuda.synchronize()
            out[f"{name}_launches"] = launches_per_call(fn, 2 if name == "reference" else 5)
        dev = {k: [] for k in variants}
        wall = {k: [] for k in variants}
        for r in range(ROUNDS):
            order = list(variants.items())
            for name, (fn, n) in (order if r % 2 == 0 else order[::-1]):   # alternating, and alternating who goes first
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                for _ in range(n):
                    fn()
                b.record()
                torch.cuda.synchronize()
                wall[name].append((time.perf_counter() - t0) / n * 1e6)
                dev[name].append(a.elapsed_time(b) / n * 1e3)
    for name in variants:
        for clock, v in (("device_us", dev[name]), ("wall_us", wall[name])):
            out[f"{name}_{clock}"] = {"median": round(sorted(v)[len(v) // 2], 1), "min": round(min(v), 1), "max": round(max(v), 1),
                                      "rounds": [round(x, 1) for x in v]}
    for kind in ("fused_float_chw", "fused_uint8_hwc"):
        for clock in ("device_us", "wall_us"):
            out[f"{kind}_faster_every_round_{clock}"] = all(f < r for f, r in zip(
                out[f"{kind}_{clock}"]["rounds"], out[f"reference_{clock}"]["rounds"]))
            out[f"{kind}_speedup_{clock}"] = round(out[f"reference_{clock}"]["median"] / out[f"{kind}_{clock}"]["median"], 1)
        out[f"{kind}_kernels"] = kernel_table(variants[kind][0], H * W, kind.endswith("uint8_hwc"), 50)
    return out


if __name__ == "__main__":
    valu_tflops, sclk = L.box_probe()
    print(json.dumps({"box_probe": {"valu_tflops": round(valu_tflops, 2), "sclk_mhz_effective": round(sclk)}}))
    ok = True
    for H, W in SIZES:
        row = bench(H, W)
        print(json.dumps(row), flush=True)
        ok = ok and row["fused_equals_reference"] and all(v for k, v in row.items() if "_faster_every_round_" in k)
    sys.exit(0 if ok else 1)
