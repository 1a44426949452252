#!/usr/bin/env python
"""The loss block between render() and loss.backward() alone (train.py:205-234): the reference's torch spelling (with
fused_ssim, as the training loop runs it today) against sfgs.loss.training_loss, forward + backward, at 1080p and 1024^2.

Both variants run in ONE process, alternating (ROUNDS alternations of ITERS iterations each); every round is timed on two
clocks: device events around the round, and the host clock around the round including a final synchronise. Also printed:
launches per iteration of each variant (torch profiler) and, for the fused variant, every kernel's time (the library's
event profiler, in a pass of its own) with the bytes the algorithm needs, counted from shapes, over that time.

usage: python tools/bench_loss.py            env: ROUNDS=8 ITERS=50 INVALID=zero|drop"""
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
from fused_ssim import fused_ssim  # noqa: E402
from sfgs import _lib as L  # noqa: E402
from sfgs.loss import training_loss  # noqa: E402

ROUNDS, ITERS = int(os.environ.get("ROUNDS", 8)), int(os.environ.get("ITERS", 50))
INVALID = os.environ.get("INVALID", "zero")
LAM, LAMD = 0.2, 0.5


def pearson_corrcoef(preds, target):   # torchmetrics' formula for one update
    preds, target = preds.squeeze(), target.squeeze()
    n = preds.shape[0]
    mx, my = preds.mean(), target.mean()
    var_x = ((preds - mx) * (preds - mx)).sum() / (n - 1)
    var_y = ((target - my) * (target - my)).sum() / (n - 1)
    corr_xy = ((preds - mx) * (target - my)).sum() / (n - 1)
    return torch.clamp(corr_xy / (var_x * var_y).sqrt(), -1.0, 1.0)


def torch_loss(image, depth, original_image, original_depth, mask):
    """train.py:205-234 as written."""
    gt_image = mask * original_image
    gt_depth = mask * original_depth
    image = mask * image
    depth = mask * depth
    Ll1 = torch.abs(image - gt_image).mean()
    ssim_value = fused_ssim(image.unsqueeze(0), gt_image.unsqueeze(0))
    loss = (1.0 - LAM) * Ll1 + LAM * (1.0 - ssim_value)
    gt_depth = gt_depth.reshape(-1, 1)
    depth = depth.reshape(-1, 1)
    nan_inf_mask = torch.isnan(depth) | torch.isinf(depth) | torch.isnan(gt_depth) | torch.isinf(gt_depth)
    depth[nan_inf_mask] = 0.0
    gt_depth[nan_inf_mask] = 0.0
    depth_loss = (1 - pearson_corrcoef(gt_depth, depth)).mean()
    loss += LAMD * depth_loss
    return loss


def fused_loss(image, depth, original_image, original_depth, mask):
    return training_loss(image, depth, original_image, original_depth, mask, LAM, LAMD, invalid=INVALID)[0]


def algorithmic_bytes(C, H, W):
    """bytes each fused kernel has to move, from shapes (f32; P pixels; one mask plane)"""
    P = H * W
    return {"loss_photo_fwd": (2 * C + 1 + 3 * C) * 4 * P, "loss_depth_fwd": 12 * P, "loss_final": 0,
            "loss_photo_bwd": (3 * C + 2 * C + 1 + C) * 4 * P, "loss_depth_bwd": 16 * P}


def bench(H, W):
    g = torch.Generator().manual_seed(H)
    C = 3
    gt_image = torch.rand(C, H, W, generator=g).cuda()
    gt_depth = (400.0 + 20.0 * torch.randn(1, H, W, generator=g)).cuda()
    mask = (torch.rand(1, H, W, generator=g) < 0.8).float().cuda()
    image = (gt_image + 0.05 * torch.randn(C, H, W, device="cuda")).clamp(0, 1).requires_grad_(True)
    depth = 0.9 * gt_depth + 6.0 * torch.randn(1, H, W, device="cuda") + 7.0
    depth.view(-1)[torch.rand(H * W, device="cuda") < 0.01] = float("nan")
    depth.requires_grad_(True)
    variants = {"torch": torch_loss, "fused": fused_loss}

    def iteration(fn):
        fn(image, depth, gt_image, gt_depth, mask).backward()
        image.grad = depth.grad = None

    out = {"H": H, "W": W, "rounds": ROUNDS, "iters": ITERS, "invalid": INVALID}
    for name, fn in variants.items():       # warm-up + launches per iteration
        for _ in range(20):
            iteration(fn)
        torch.cuda.synchronize()
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                iteration(fn)
            torch.cuda.synchronize()
        out[f"{name}_launches"] = sum(e.count for e in prof.key_averages() if e.device_time_total > 0) / 5
    dev = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():   # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(ITERS):
                iteration(fn)
            b.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / ITERS * 1e3)
            dev[name].append(a.elapsed_time(b) / ITERS)
    for name in variants:
        for clock, v in (("device_ms", dev[name]), ("wall_ms", wall[name])):
            out[f"{name}_{clock}"] = {"median": round(sorted(v)[len(v) // 2], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    for clock in ("device_ms", "wall_ms"):
        out[f"speedup_{clock}"] = round(out[f"torch_{clock}"]["median"] / out[f"fused_{clock}"]["median"], 2)
        out[f"faster_beyond_spread_{clock}"] = out[f"fused_{clock}"]["max"] < out[f"torch_{clock}"]["min"]
    # per-kernel time of the fused variant (events around every launch: a pass of its own), bytes from shapes over it
    L.profile_enable(True)
    L.profile_collect()
    for _ in range(ITERS):
        iteration(fused_loss)
    prof = L.profile_collect()
    L.profile_enable(False)
    nbytes = algorithmic_bytes(C, H, W)
    out["fused_kernels"] = {k: {"us": round(ms / n * 1e3, 2), "bytes": nbytes.get(k),
                                "TB_per_s": round(nbytes[k] / (ms / n * 1e-3) / 1e12, 3) if nbytes.get(k) else None}
                            for k, (ms, n) in prof.items()}
    return out


if __name__ == "__main__":
    valu_tflops, sclk = L.box_probe()
    print(json.dumps({"box_probe": {"valu_tflops": round(valu_tflops, 2), "sclk_mhz_effective": round(sclk)}}))
    for H, W in ((1080, 1920), (1024, 1024)):
        print(json.dumps(bench(H, W)))
