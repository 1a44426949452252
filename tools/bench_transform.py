#!/usr/bin/env python
"""sfgs.transform.transform_gaussians against the torch spelling of the same similarity transform, written here: positions
(`s * (xyz @ R.T) + t`), log-scales (`+ log s`), quaternions (the Hamilton product, column by column), the SH coefficients
beyond DC (one matmul per band on a strided slice of [N,15,3]) and filter_3D, at N = 2 M and 16 M Gaussians, SH degree 3, in
the model's layout ([N,15,3]), both out of place.

The two run in ONE process, alternating (ROUNDS rounds of ITERS calls each, alternating who goes first) after a warm-up; every
round is timed with device events around it and with the host clock around it including a final synchronise. Printed, one
JSON line per size: both variants' times per round, launches per call (torch.profiler), the kernel's own time per launch
(torch.profiler) with the bytes the algorithm needs, 2 * 4 * N * (3 + 3 + 4 + 45 + 1) -- every float read once and written
once -- over that time and as a fraction of 8 TB/s, and whether the kernel beat the torch spelling in every round. The tool
exits with status 1 unless it did, on both clocks, at both sizes.

usage: python tools/bench_transform.py            env: ROUNDS=5 ITERS=20 SIZES=2000000,16000000"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
from sfgs import _lib as L  # noqa: E402
from sfgs import transform as T  # noqa: E402

ROUNDS, ITERS = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("ITERS", 20))
SIZES = tuple(int(v) for v in os.environ.get("SIZES", "2000000,16000000").split(","))
PEAK_TB_S = 8.0


class TorchSpelling:
    """The transform as one writes it in torch: constants on the device once, then a dozen launches per call."""

    def __init__(self, sim, dev):
        c = T.kernel_constants(sim)
        f = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
        self.R, self.t, self.q = f(c["R"]), f(c["t"]), f(c["q"])
        self.D = [f(c["D1"]), f(c["D2"]), f(c["D3"])]
        self.s, self.log_s = float(c["s"]), float(c["log_s"])

    @torch.no_grad()
    def __call__(self, xyz, scaling, rotation, features_rest, filter_3D):
        xyz2 = self.s * (xyz @ self.R.T) + self.t
        scaling2 = scaling + self.log_s
        aw, ax, ay, az = self.q
        bw, bx, by, bz = rotation.unbind(1)
        rotation2 = torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                                 aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], 1)
        rest2 = torch.empty_like(features_rest)
        for (a, b), D in zip(((0, 3), (3, 8), (8, 15)), self.D):
            rest2[:, a:b] = torch.einsum("ij,njc->nic", D, features_rest[:, a:b])
        return xyz2, scaling2, rotation2, rest2, filter_3D * self.s


def profiled(fn, calls):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return [e for e in prof.key_averages() if e.device_time_total > 0]


def stats(v):
    return {"median": round(sorted(v)[len(v) // 2], 1), "min": round(min(v), 1), "max": round(max(v), 1),
            "rounds": [round(x, 1) for x in v]}


def bench(N, sim):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N)
    rnd = lambda *shape: torch.randn(*shape, generator=g, device=dev)
    tensors = (rnd(N, 3) * 100, rnd(N, 3), rnd(N, 4), rnd(N, 15, 3) * 0.3, torch.rand(N, 1, generator=g, device=dev))
    spelled = TorchSpelling(sim, dev)
    variants = {"torch": lambda: spelled(*tensors), "kernel": lambda: T.transform_gaussians(sim, *tensors)}
    out = {"N": N, "rounds": ROUNDS, "iters": ITERS, "algorithmic_bytes": 2 * 4 * N * (3 + 3 + 4 + 45 + 1)}
    # the two agree on the timed input (float32 against float32: a loose check that both compute the same transform)
    a, b = variants["torch"](), variants["kernel"]()
    out["max_abs_difference"] = [float((x - y).abs().max()) for x, y in zip(a, b)]
    del a, b
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        rows = profiled(fn, 3)
        out[f"{name}_launches_per_call"] = sum(e.count for e in rows) / 3
        if name == "kernel":
            k = [e for e in rows if "similarity_kernel" in e.key]
            assert len(k) == 1, [e.key for e in rows]
            us = k[0].device_time_total / k[0].count
            tb_s = out["algorithmic_bytes"] / (us * 1e-6) / 1e12
            out["similarity_kernel"] = {"us": round(us, 1), "TB_per_s": round(tb_s, 3),
                                        "fraction_of_8_TB_per_s": round(tb_s / PEAK_TB_S, 3)}
    dev_us, wall_us = {k: [] for k in variants}, {k: [] for k in variants}
    for r in range(ROUNDS):
        order = list(variants.items())
        for name, fn in (order if r % 2 == 0 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(ITERS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            wall_us[name].append((time.perf_counter() - t0) / ITERS * 1e6)
            dev_us[name].append(e0.elapsed_time(e1) / ITERS * 1e3)
    for name in variants:
        out[f"{name}_device_us"], out[f"{name}_wall_us"] = stats(dev_us[name]), stats(wall_us[name])
    for clock in ("device_us", "wall_us"):
        out[f"kernel_faster_every_round_{clock}"] = all(k < t for k, t in zip(out[f"kernel_{clock}"]["rounds"],
                                                                             out[f"torch_{clock}"]["rounds"]))
        out[f"speedup_{clock}"] = round(out[f"torch_{clock}"]["median"] / out[f"kernel_{clock}"]["median"], 2)
    return out


if __name__ == "__main__":
    valu_tflops, sclk = L.box_probe()
    print(json.dumps({"box_probe": {"valu_tflops": round(valu_tflops, 2), "sclk_mhz_effective": round(sclk)}}))
    q = np.random.default_rng(1).normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    sim = T.Similarity(R, 0.37, (100.0, -50.0, 20.0))
    ok = True
    for N in SIZES:
        row = bench(N, sim)
        print(json.dumps(row), flush=True)
        ok = ok and row["kernel_faster_every_round_device_us"] and row["kernel_faster_every_round_wall_us"]
        torch.cuda.empty_cache()
    sys.exit(0 if ok else 1)
