#!/usr/bin/env python
"""The evaluation pass alone: the reference's spelling of training_report's per-view metrics (train.py:1064,1075,1090-1091:
two clamps, `l1_loss(image, gt_image).mean().double()`, `psnr(image, gt_image).mean().double()` with psnr of
utils/image_utils.py:17-19, and the two running `+=`), restated here, once as the reference has it and once with fused_ssim
added, against sfgs.metrics.Evaluator.add with and without SSIM, at 1920 x 1080 and 1024^2. sfgs.loss.photometric under
no_grad -- the existing kernel that moves the same bytes through the same tile -- runs in the same rounds as the yardstick of
the tile kernel.

The variants run in ONE process, alternating (ROUNDS alternations of ITERS calls each, and alternating who goes first) after
a warm-up; every round is timed on two clocks: device events around the round, and the host clock around the round including
a final synchronise. Also printed: launches per call (torch.profiler: kernels, memsets and copies with device time), every
kernel of the fused variants and of photometric (torch.profiler's device time per launch, in a pass of its own) with the
bytes the algorithm needs (2 * P * H * W * 4, counted from shapes) over that time and as a fraction of 8 TB/s, and the two
comparisons: Evaluator.add against the reference's spelling in every round, and the tile kernel plus finalisation against
photometric without gradients, with photometric's own round-to-round spread next to the difference. The tool exits with
status 1 unless Evaluator.add is faster than the reference's spelling in every round on both clocks.

usage: python tools/bench_metrics.py            env: ROUNDS=6 ITERS=200"""
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
from fused_ssim import fused_ssim  # noqa: E402
from sfgs import _lib as L  # noqa: E402
from sfgs import loss, metrics  # noqa: E402

ROUNDS, ITERS = int(os.environ.get("ROUNDS", 6)), int(os.environ.get("ITERS", 200))
SIZES = ((1080, 1920), (1024, 1024))
PEAK_TB_S = 8.0


def l1_loss(network_output, gt):                       # utils/loss_utils.py:17-18
    return torch.abs((network_output - gt)).mean()


def psnr(img1, img2):                                  # utils/image_utils.py:17-19
    mse = (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


class ReferenceLoop:
    """The metrics statements of training_report's loop body around two running sums (which start as Python floats)."""

    def __init__(self, with_ssim):
        self.with_ssim = with_ssim
        self.reset()

    def reset(self):
        self.l1_test, self.psnr_test, self.ssim_test = 0.0, 0.0, 0.0

    @torch.no_grad()
    def add(self, render, original_image):
        image = torch.clamp(render, 0.0, 1.0)
        gt_image = torch.clamp(original_image, 0.0, 1.0)
        self.l1_test += l1_loss(image, gt_image).mean().double()
        self.psnr_test += psnr(image, gt_image).mean().double()
        if self.with_ssim:
            self.ssim_test += fused_ssim(image[None], gt_image[None], train=False).double()


def synthetic_pair(H, W, seed):
    """A render-like pair: a target in [0, 1] and a noisy estimate of it that leaves [0, 1] here and there."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g)
    return (gt + 0.1 * torch.randn(3, H, W, generator=g)).cuda(), gt.cuda()


def profiled(fn, calls):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return [e for e in prof.key_averages() if e.device_time_total > 0]


def launches_per_call(fn, calls):
    return sum(e.count for e in profiled(fn, calls)) / calls


def kernel_table(fn, nbytes, calls):
    """Every device activity of `calls` calls: launches per call, device us per launch (torch.profiler), and for the kernels
    that pass over the pair the bytes the algorithm needs over the kernel's time."""
    table = {}
    for e in profiled(fn, calls):
        us = e.device_time_total / e.count
        name = re.sub(r"\(.*", "", e.key).replace("void ", "").replace("sfgs::", "")[:60]
        streams = any(k in e.key for k in ("metrics_tile_kernel", "metrics_stream_kernel", "loss_photo_fwd_kernel"))
        while name in table:                               # never fold two profiler rows into one
            name += "'"
        table[name] = {"launches_per_call": e.count / calls, "us": round(us, 2), "bytes": nbytes if streams else None}
    for row in table.values():
        row["TB_per_s"] = round(row["bytes"] / (row["us"] * 1e-6) / 1e12, 3) if row["bytes"] else None
        row["fraction_of_8_TB_per_s"] = round(row["TB_per_s"] / PEAK_TB_S, 3) if row["bytes"] else None
    return table


def stats(v):
    return {"median": round(sorted(v)[len(v) // 2], 1), "min": round(min(v), 1), "max": round(max(v), 1),
            "rounds": [round(x, 1) for x in v]}


def bench(H, W):
    image, gt = synthetic_pair(H, W, H + W)
    ref, ref_ssim = ReferenceLoop(False), ReferenceLoop(True)
    ev = metrics.Evaluator(max(ITERS, 64))

    def photometric():
        with torch.no_grad():
            return loss.photometric(image, gt)
    variants = {"reference": (lambda: ref.add(image, gt), ref.reset),
                "reference_with_fused_ssim": (lambda: ref_ssim.add(image, gt), ref_ssim.reset),
                "evaluator_add": (lambda: ev.add(image, gt), ev.reset),
                "evaluator_add_no_ssim": (lambda: ev.add(image, gt, ssim=False), ev.reset),
                "photometric_no_grad": (photometric, lambda: None)}
    out = {"H": H, "W": W, "rounds": ROUNDS, "iters": ITERS, "algorithmic_bytes": 2 * 3 * H * W * 4}
    for name, (fn, reset) in variants.items():             # warm-up + launches per call
        reset()
        for _ in range(30):
            fn()
        torch.cuda.synchronize()
        out[f"{name}_launches"] = launches_per_call(fn, 5)
    # the figures agree: the fused row against the reference's spelling on the timed input
    ev.reset()
    ref_ssim.reset()
    ev.add(image, gt)
    ref_ssim.add(image, gt)
    row = ev.result()["per_view"][0]
    out["evaluator_row"] = {k: float(v) for k, v in zip(metrics.ROW, row)}
    out["reference_values"] = {"l1": ref_ssim.l1_test.item(), "psnr": ref_ssim.psnr_test.item(), "ssim": ref_ssim.ssim_test.item()}
    dev = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    for r in range(ROUNDS):
        order = list(variants.items())
        for name, (fn, reset) in (order if r % 2 == 0 else order[::-1]):   # alternating, and alternating who goes first
            reset()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(ITERS):
                fn()
            b.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / ITERS * 1e6)
            dev[name].append(a.elapsed_time(b) / ITERS * 1e3)
    for name in variants:
        out[f"{name}_device_us"] = stats(dev[name])
        out[f"{name}_wall_us"] = stats(wall[name])
    for kind in ("evaluator_add", "evaluator_add_no_ssim"):
        for clock in ("device_us", "wall_us"):
            out[f"{kind}_faster_than_reference_every_round_{clock}"] = all(f < r for f, r in zip(
                out[f"{kind}_{clock}"]["rounds"], out[f"reference_{clock}"]["rounds"]))
            out[f"{kind}_speedup_{clock}"] = round(out[f"reference_{clock}"]["median"] / out[f"{kind}_{clock}"]["median"], 2)
    out["evaluator_add_speedup_over_reference_with_fused_ssim_device_us"] = round(
        out["reference_with_fused_ssim_device_us"]["median"] / out["evaluator_add_device_us"]["median"], 2)
    for name in ("evaluator_add", "evaluator_add_no_ssim", "photometric_no_grad"):
        variants[name][1]()
        out[f"{name}_kernels"] = kernel_table(variants[name][0], out["algorithmic_bytes"], 50)
    # the tile kernel plus finalisation against photometric without gradients: kernel time (profiler) and round time (events)
    ksum = lambda t: round(sum(r["us"] * r["launches_per_call"] for r in t.values()), 2)
    photo = out["photometric_no_grad_device_us"]
    out["tile_vs_photometric"] = {
        "metrics_kernels_us": ksum(out["evaluator_add_kernels"]), "photometric_kernels_us": ksum(out["photometric_no_grad_kernels"]),
        "add_minus_photometric_device_us_per_round": [round(a - p, 1) for a, p in zip(out["evaluator_add_device_us"]["rounds"],
                                                                                       photo["rounds"])],
        "photometric_round_to_round_spread_us": round(photo["max"] - photo["min"], 1)}
    t = out["tile_vs_photometric"]
    t["no_slower_beyond_spread"] = bool(out["evaluator_add_device_us"]["median"] <= photo["median"] + t["photometric_round_to_round_spread_us"]
                                        and t["metrics_kernels_us"] <= t["photometric_kernels_us"] + t["photometric_round_to_round_spread_us"])
    return out


if __name__ == "__main__":
    valu_tflops, sclk = L.box_probe()
    print(json.dumps({"box_probe": {"valu_tflops": round(valu_tflops, 2), "sclk_mhz_effective": round(sclk)}}))
    ok = True
    for H, W in SIZES:
        row = bench(H, W)
        print(json.dumps(row), flush=True)
        ok = ok and all(v for k, v in row.items() if k.startswith("evaluator_add_faster_than_reference_every_round_"))
    sys.exit(0 if ok else 1)
