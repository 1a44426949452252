#!/usr/bin/env python
"""The jittered ground truth alone: the reference's spelling of `gt_image = mask * original_image` and create_offset_gt
(train.py:207, 64-77: np.meshgrid of Python ranges, stack, cast, a pageable upload, six elementwise launches, grid_sample),
restated here with device tensors in and a device tensor out, against sfgs.resample.resample_gt, at 1920 x 1080 and 1024^2,
C = 3, with a [1,H,W] mask and without one.

Both variants run in ONE process, alternating and alternating who goes first (ROUNDS rounds; REF_ITERS calls of the reference
spelling and ITERS calls of the kernel path per round) after a warm-up; every round is timed on two clocks: device events
around the round, and the host clock around the round including a final synchronise. Also measured: launches per call
(torch.profiler: kernels, memsets and copies with device time); the host part of the reference spelling alone (meshgrid,
stack, cast: host clock, no device involved); the kernel's own time -- an event pair around KERNEL_ITERS back-to-back calls
of the library entry into one preallocated output (no allocation, no Python between the launches but the ctypes call), and
torch.profiler's device time per launch as a second opinion -- with the bytes the algorithm needs, (2 + C + C + [1]) * 4 * H * W,
over that time and that as a share of ROOF_TBS (8 TB/s); and the kernel path's error next to the reference spelling's, both
against the float64 oracle (tests/resample_np.py), on the timed input.

The output is a report in text, then one JSON line per case. The tool exits with status 1 unless the kernel path is faster
than the reference spelling in every round on both clocks, in every case.

usage: python tools/bench_resample.py            env: ROUNDS=6 ITERS=200 REF_ITERS=5 KERNEL_ITERS=500"""
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
from resample_np import resample64  # noqa: E402
from sfgs import _lib as L  # noqa: E402
from sfgs.resample import resample_gt  # noqa: E402

ROUNDS, ITERS = int(os.environ.get("ROUNDS", 6)), int(os.environ.get("ITERS", 200))
REF_ITERS, KERNEL_ITERS = int(os.environ.get("REF_ITERS", 5)), int(os.environ.get("KERNEL_ITERS", 500))
ROOF_TBS = 8.0
SIZES = ((1080, 1920), (1024, 1024))
CH = 3


def host_grid(height, width):
    """train.py:67-68: the part of create_offset_gt that never leaves the host."""
    meshgrid = np.meshgrid(range(width), range(height), indexing='xy')
    return np.stack(meshgrid, axis=0).astype(np.float32)


@torch.no_grad()
def create_offset_gt(image, offset):   # train.py:64-77
    height, width = image.shape[1:]
    id_coords = torch.from_numpy(host_grid(height, width)).cuda()
    id_coords = id_coords.permute(1, 2, 0) + offset
    id_coords[..., 0] /= (width - 1)
    id_coords[..., 1] /= (height - 1)
    id_coords = id_coords * 2 - 1
    return torch.nn.functional.grid_sample(image[None], id_coords[None], align_corners=True, padding_mode="border")[0]


def reference_spelling(image, offset, mask):
    """train.py:207 and :215. Without a mask the product is left out (in train.py it is always there: ones (1,1,1))."""
    return create_offset_gt(image if mask is None else mask * image, offset)


def launches_per_call(fn, calls):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    rows = {e.key: (e.count / calls, e.device_time_total / e.count) for e in prof.key_averages() if e.device_time_total > 0}
    return sum(n for n, _ in rows.values()), rows


def kernel_event_pair(image, offset, mask):
    """us per launch: events around KERNEL_ITERS calls of sfgs_resample_gt into one output."""
    lib = L.load()
    Cc, H, W = image.shape
    out = torch.empty_like(image)
    args = L.SfgsResampleArgs(C.sizeof(L.SfgsResampleArgs), Cc, H, W, image.data_ptr(), None if mask is None else mask.data_ptr(),
                              0 if mask is None else mask.numel(), offset.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref_args, out_ptr = C.byref(args), L.ptr(out)
    for _ in range(50):
        L.check(lib.sfgs_resample_gt(ref_args, out_ptr, stream))
    samples = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(KERNEL_ITERS):
            lib.sfgs_resample_gt(ref_args, out_ptr, stream)
        b.record()
        torch.cuda.synchronize()
        samples.append(a.elapsed_time(b) / KERNEL_ITERS * 1e3)
    return sorted(samples)


def bench(H, W, with_mask):
    g = torch.Generator().manual_seed(H + W + int(with_mask))
    image = torch.rand(CH, H, W, generator=g).cuda()
    offset = (torch.rand(H, W, 2, generator=g) - 0.5).cuda()                        # train.py:190
    mask = (torch.rand(1, H, W, generator=g) < 0.8).float().cuda() if with_mask else None
    variants = {"reference": (lambda: reference_spelling(image, offset, mask), REF_ITERS),
                "kernel": (lambda: resample_gt(image, offset, mask), ITERS)}
    out = {"H": H, "W": W, "C": CH, "mask": with_mask, "rounds": ROUNDS, "iters": {k: n for k, (_, n) in variants.items()}}
    want = resample64(image.cpu().numpy(), offset.cpu().numpy(), None if mask is None else mask.cpu().numpy())
    out["e_kernel"] = float(np.abs(resample_gt(image, offset, mask).cpu().numpy() - want).max())
    out["e_reference"] = float(np.abs(reference_spelling(image, offset, mask).cpu().numpy() - want).max())
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        host_grid(H, W)
        t.append((time.perf_counter() - t0) * 1e3)
    out["reference_host_grid_ms"] = {"median": round(sorted(t)[2], 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    for name, (fn, n) in variants.items():             # warm-up + launches per call
        for _ in range(3 if name == "reference" else 30):
            fn()
        torch.cuda.synchronize()
        out[f"{name}_launches"], rows = launches_per_call(fn, 2 if name == "reference" else 20)
        if name == "kernel":
            out["kernel_profiler_us"] = round(next(us for k, (_, us) in rows.items() if "resample_gt_kernel" in k), 2)
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
    for clock in ("device_us", "wall_us"):
        out[f"kernel_faster_every_round_{clock}"] = all(f < r for f, r in zip(out[f"kernel_{clock}"]["rounds"],
                                                                              out[f"reference_{clock}"]["rounds"]))
        out[f"speedup_{clock}"] = round(out[f"reference_{clock}"]["median"] / out[f"kernel_{clock}"]["median"], 1)
    pair = kernel_event_pair(image, offset, mask)
    nbytes = (2 + CH + CH + int(with_mask)) * 4 * H * W
    out["kernel_event_pair_us"] = {"median": round(pair[len(pair) // 2], 2), "min": round(pair[0], 2), "max": round(pair[-1], 2)}
    out["algorithmic_bytes"] = nbytes
    for key, us in (("event_pair", pair[len(pair) // 2]), ("profiler", out["kernel_profiler_us"])):
        out[f"TB_per_s_{key}"] = round(nbytes / (us * 1e-6) / 1e12, 3)
        out[f"roofline_share_{key}"] = round(nbytes / (us * 1e-6) / 1e12 / ROOF_TBS, 3)
    return out


def report(row):
    name = f"{row['H']} x {row['W']}, C = {row['C']}, " + ("[1,H,W] mask" if row["mask"] else "no mask")
    print(f"   {name}   (max |. - oracle64|: kernel {row['e_kernel']:.3e}, reference spelling {row['e_reference']:.3e})")
    print("   variant        device us [min .. max]               host us [min .. max]                 launches")
    for v in ("reference", "kernel"):
        d, w = row[f"{v}_device_us"], row[f"{v}_wall_us"]
        print(f"   {v:<12} {d['median']:>10.1f} [{d['min']:>10.1f} .. {d['max']:>10.1f}]   {w['median']:>10.1f} "
              f"[{w['min']:>10.1f} .. {w['max']:>10.1f}]   {row[f'{v}_launches']:>6.1f}")
    print(f"   per round, device us:  reference: {row['reference_device_us']['rounds']}  kernel: {row['kernel_device_us']['rounds']}")
    print(f"   per round, host us:    reference: {row['reference_wall_us']['rounds']}  kernel: {row['kernel_wall_us']['rounds']}")
    print(f"   kernel path faster than the reference spelling in EVERY round: device {row['kernel_faster_every_round_device_us']}, "
          f"host {row['kernel_faster_every_round_wall_us']};  reference / kernel (medians): {row['speedup_device_us']} x, "
          f"{row['speedup_wall_us']} x")
    h = row["reference_host_grid_ms"]
    print(f"   the reference's host part alone (meshgrid, stack, cast): {h['median']} ms [{h['min']} .. {h['max']}]")
    p = row["kernel_event_pair_us"]
    print(f"   the kernel: {p['median']} us [{p['min']} .. {p['max']}] by event pair over {KERNEL_ITERS} back-to-back launches, "
          f"{row['kernel_profiler_us']} us per launch by torch.profiler; {row['algorithmic_bytes']} algorithmic bytes -> "
          f"{row['TB_per_s_event_pair']} / {row['TB_per_s_profiler']} TB/s = {100 * row['roofline_share_event_pair']:.1f} % / "
          f"{100 * row['roofline_share_profiler']:.1f} % of {ROOF_TBS:g} TB/s")
    print()


if __name__ == "__main__":
    valu_tflops, sclk = L.box_probe()
    print("resample_gt (create_offset_gt of train.py:64-77 on mask * original_image) -- sfgs.resample / csrc/resample.hip")
    print(f"One MI355X (box probe: valu_tflops {valu_tflops:.2f}, sclk_mhz_effective {sclk:.0f}). Measured by tools/bench_resample.py "
          f"in ONE process: {ROUNDS} rounds of {REF_ITERS} reference calls and {ITERS} kernel-path calls, alternating.")
    print("us per call = median of the rounds [min .. max]; device clock = events around a round, host clock = around a round "
          "including the final synchronise.\n")
    ok, rows = True, []
    for H, W in SIZES:
        for with_mask in (True, False):
            row = bench(H, W, with_mask)
            rows.append(row)
            report(row)
            sys.stdout.flush()
            ok = ok and row["kernel_faster_every_round_device_us"] and row["kernel_faster_every_round_wall_us"]
    for row in rows:
        print(json.dumps(row))
    sys.exit(0 if ok else 1)
