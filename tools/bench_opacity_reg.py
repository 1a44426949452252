#!/usr/bin/env python
"""The opacity regulariser alone (train.py:236-242): the reference's torch spelling -- sigmoid, clamp,
binary_cross_entropy(opacity, opacity), times lambda_opacity, and their autograd mirror -- against
sfgs.loss.opacity_entropy, forward + backward, at N = 100 k, 500 k, 2 M and 8 M raw opacities in float32 and in float64
(what `_opacity` is from the first reset_opacity on).

Both variants run in ONE process, alternating (ROUNDS alternations of ITERS iterations each) after a warm-up; every round is
timed on two clocks: device events around the round, and the host clock around the round including a final synchronise.
Also printed: launches per iteration of each variant (torch's via torch.profiler, ours via the library's event profiler) and,
for the fused variant, every kernel's time (the event profiler, in a pass of its own) with the bytes the algorithm has to
move -- N * s read forward, N * s read + N * s written backward, s the element size -- over that time.

usage: python tools/bench_opacity_reg.py            env: ROUNDS=8 ITERS=50 SIZES=100000,500000,2000000,8000000"""
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
from sfgs import _lib as L  # noqa: E402
from sfgs.loss import opacity_entropy  # noqa: E402

ROUNDS, ITERS = int(os.environ.get("ROUNDS", 8)), int(os.environ.get("ITERS", 50))
SIZES = [int(v) for v in os.environ.get("SIZES", "100000,500000,2000000,8000000").split(",")]
LAMBDA_OPACITY = 10.0   # the reference README's main command


def torch_term(opacity_raw):
    """train.py:239-242 as written, on get_opacity = sigmoid(_opacity) (scene/gaussian_model.py:234)."""
    opacity = torch.sigmoid(opacity_raw).clamp(1.0e-3, 1.0 - 1.0e-3)
    opacity_loss = torch.nn.functional.binary_cross_entropy(opacity, opacity)
    return LAMBDA_OPACITY * opacity_loss


def fused_term(opacity_raw):
    return LAMBDA_OPACITY * opacity_entropy(opacity_raw)


def bench(n, dtype):
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, 1, generator=g, dtype=dtype) * 3.0).cuda().requires_grad_(True)
    variants = {"torch": torch_term, "fused": fused_term}
    size = x.element_size()

    def iteration(fn):
        fn(x).backward()
        x.grad = None

    out = {"N": n, "dtype": str(dtype).replace("torch.", ""), "rounds": ROUNDS, "iters": ITERS}
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
    for r in range(ROUNDS):
        order = list(variants.items())
        for name, fn in (order if r % 2 == 0 else order[::-1]):   # alternating, and alternating who goes first
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(ITERS):
                iteration(fn)
            b.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / ITERS * 1e6)
            dev[name].append(a.elapsed_time(b) / ITERS * 1e3)
    for name in variants:
        for clock, v in (("device_us", dev[name]), ("wall_us", wall[name])):
            out[f"{name}_{clock}"] = {"median": round(sorted(v)[len(v) // 2], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    for clock in ("device_us", "wall_us"):
        out[f"speedup_{clock}"] = round(out[f"torch_{clock}"]["median"] / out[f"fused_{clock}"]["median"], 2)
        out[f"fused_not_slower_{clock}"] = out[f"fused_{clock}"]["median"] <= out[f"torch_{clock}"]["median"]
    # the fused variant's own kernels (events around every launch: a pass of its own), bytes from shapes over their time
    L.profile_enable(True)
    L.profile_collect()
    for _ in range(ITERS):
        iteration(fused_term)
    prof = L.profile_collect()
    L.profile_enable(False)
    nbytes = {"opacity_entropy_fwd": n * size, "opacity_entropy_final": 0, "opacity_entropy_bwd": 2 * n * size}
    out["fused_library_launches"] = {k: cnt / ITERS for k, (_, cnt) in prof.items()}
    out["fused_kernels"] = {k: {"us": round(ms / cnt * 1e3, 2), "bytes": nbytes.get(k),
                                "TB_per_s": round(nbytes[k] / (ms / cnt * 1e-3) / 1e12, 3) if nbytes.get(k) else None}
                            for k, (ms, cnt) in prof.items()}
    return out


if __name__ == "__main__":
    valu_tflops, sclk = L.box_probe()
    print(json.dumps({"box_probe": {"valu_tflops": round(valu_tflops, 2), "sclk_mhz_effective": round(sclk)}}))
    for n in SIZES:
        for dtype in (torch.float32, torch.float64):
            print(json.dumps(bench(n, dtype)), flush=True)
