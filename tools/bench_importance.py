#!/usr/bin/env python
"""sfgs.importance.BlendStats.add per view -- split by device events into its forward (plan + inference render) and its
statistics kernels (blend_stats + views) -- next to the only other route to the per-Gaussian weight sum: a training forward plus
the backward of `color[0].sum()` (colors_precomp.grad[:, 0] = sum of w; it yields neither the maximum nor the hit count).

Scenes: the headline (sfgs.synth.cfg2: 2 M Gaussians, 1080p) and the opaque city seen from 25 degrees (city_scene, 2 M, 1080p).
Both routes run in ONE process, rounds interleaved (ROUNDS rounds of ITERS views each, alternating who goes first) after a
warm-up; every round is timed with device events around it. Printed, one JSON line per scene: per-view times of both routes
per round, the split of add, the statistics kernel's own time (torch.profiler), the view's list entries, blended pairs and
blended Gaussians, and the agreement of the two sums. There is no threshold: the tool reports what it finds.

usage: python tools/bench_importance.py            env: ROUNDS=5 ITERS=10 N=2000000 SCENES=headline,city_e25"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
from diff_gauss import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from sfgs import _lib as L  # noqa: E402
from sfgs.importance import BlendStats  # noqa: E402
from sfgs.synth import cfg2, city_scene  # noqa: E402

ROUNDS, ITERS = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("ITERS", 10))
N = int(os.environ.get("N", 2_000_000))
SCENES = os.environ.get("SCENES", "headline,city_e25").split(",")
W, H = 1920, 1080


def stats(v):
    return {"median": round(sorted(v)[len(v) // 2], 1), "min": round(min(v), 1), "max": round(max(v), 1),
            "rounds": [round(x, 1) for x in v]}


def bench(name):
    dev = torch.device("cuda:0")
    frame, g = cfg2(n=N) if name == "headline" else city_scene(N, W, H, 25.0, seed=0)
    settings = GaussianRasterizationSettings(
        H, W, frame["tanfovx"], frame["tanfovy"], frame["kernel_size"], None, frame["bg"].to(dev), frame["scale_modifier"],
        frame["view"].to(dev), frame["proj"].to(dev), 0, frame["campos"].to(dev), False, False)
    t = {k: v.to(dev) for k, v in g.items() if v is not None}
    table = BlendStats(N, dev)
    colors = t["colors_precomp"].clone().requires_grad_(True)
    raster = GaussianRasterizer(settings)

    def add():
        table.add(settings, **t)

    def backward():
        colors.grad = None
        color = raster(means3D=t["means3D"], means2D=None, colors_precomp=colors, opacities=t["opacities"],
                       scales=t["scales"], rotations=t["rotations"])[0]
        color[0].sum().backward()

    variants = {"add": add, "forward_backward": backward}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    # one view of each, compared
    table.reset()
    add()
    backward()
    torch.cuda.synchronize()
    ws, grad = table.weight_sum, colors.grad[:, 0].double()
    out = {"scene": name, "N": N, "size": [W, H], "rounds": ROUNDS, "iters": ITERS, "list_entries": int(table.last_duplicates),
           "blended_pairs": int(table.hits.sum()), "blended_gaussians": int((table.hits > 0).sum()),
           "rel_l2_sum_vs_grad": float((ws - grad).norm() / grad.norm()),
           "same_rows": bool(torch.equal(table.hits > 0, grad != 0))}
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(3):
            add()
        torch.cuda.synchronize()
    k = [e for e in prof.key_averages() if "blend_stats_kernel" in e.key]
    out["blend_stats_kernel_us"] = round(k[0].device_time_total / k[0].count, 1) if k else None
    k = [e for e in prof.key_averages() if "composite_fwd_kernel" in e.key]
    out["composite_fwd_kernel_us"] = round(k[0].device_time_total / k[0].count, 1) if k else None
    per_view = {v: [] for v in variants}
    split = {"forward": [], "statistics": []}
    for r in range(ROUNDS):
        order = list(variants.items())
        for vname, fn in (order if r % 2 == 0 else order[::-1]):
            table.timing = [] if vname == "add" else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(ITERS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per_view[vname].append(e0.elapsed_time(e1) / ITERS * 1e3)
            if vname == "add":
                split["forward"].append(float(np.mean([a.elapsed_time(b) for a, b, _ in table.timing])) * 1e3)
                split["statistics"].append(float(np.mean([b.elapsed_time(c) for _, b, c in table.timing])) * 1e3)
                table.timing = None
    out["add_us_per_view"] = stats(per_view["add"])
    out["add_forward_us"] = stats(split["forward"])
    out["add_statistics_us"] = stats(split["statistics"])
    out["forward_backward_us_per_view"] = stats(per_view["forward_backward"])
    out["add_over_forward_backward"] = round(out["add_us_per_view"]["median"] / out["forward_backward_us_per_view"]["median"], 3)
    return out


if __name__ == "__main__":
    valu_tflops, sclk = L.box_probe()
    print(json.dumps({"box_probe": {"valu_tflops": round(valu_tflops, 2), "sclk_mhz_effective": round(sclk)}}))
    for scene_name in SCENES:
        print(json.dumps(bench(scene_name)), flush=True)
        torch.cuda.empty_cache()
