#!/usr/bin/env python
"""Multi-view depth consistency alone: sfgs.consistency.ViewSet (csrc/consistency.hip) against its numpy restatement
(tests/consistency_np.py) on the scene of tools/bench_geometry.py: 24 depth maps of 1024 x 1024 of a 1024 x 1024-cell terrain.

  (a) one reference view against its 23 sources: ViewSet.check and consistency_np.check in one process, alternating, ROUNDS
      times after a warm-up. Device: events around the launch. Host: the host clock, started after a device synchronise; the
      depth maps are downloaded beforehand and that is not timed. The two results must be the same bytes.
  (b) all reference views on the device: events per view -> time per view, pixel pairs per second (V (V - 1) H W pairs; a pair
      that leaves at its first test counts like one that runs to the end) and the bytes gathered: 4 per pair that reaches the
      source's depth map. That number depends on the data; it is exact for view 0 (the restatement counts its branches) and an
      upper bound, 4 bytes for every pair, for the set.
  (c) informational, no bar: evaluate_dsm on the same scene with 3 x 3-blurred depth maps (consistency_np.blur3, the stand-in
      for a splatting depth map's blend at an edge) against the terrain itself, with and without consistency=.
  (d) --variant LIB: a second build of libsfgs.so whose kernel has the other pixel-to-lane layout (tools/variants/
      consistency_row_major.patch through tools/build_variant.sh: a workgroup is a row-major run of 256 pixels instead of a
      16 x 16 tile). sfgs_consistency_check of both libraries on the same table and the same prepared argument blocks, all
      reference views, alternating sets; the outputs must be the same bytes.
Rates only: the guides give no FP64 vector peak for this chip, so no share of peak is claimed.
Exits with status 1 unless check() is faster than the restatement in every round of (a) and equal to it.

usage: python tools/bench_consistency.py [--variant LIB] [--out FILE]      env: ROUNDS=3 VIEWS=24 SIZE=1024 CELLS=1024"""
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
from sfgs import geometry as geo  # noqa: E402
from sfgs.consistency import ViewSet  # noqa: E402

ROUNDS = bg.ROUNDS
PARAMS = {"rel_tol": 0.01, "px_tol": 1.0, "min_views": 2}


def device_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return out, start.elapsed_time(end)


def raw_check(lib_path, vs):
    """-> run(i, count, keep): sfgs_consistency_check of the library at lib_path on vs's table, reference view i"""
    from sfgs import _lib as L
    lib = L.C.CDLL(lib_path)
    fn = lib.sfgs_consistency_check
    fn.restype, fn.argtypes = L.SYMBOLS["sfgs_consistency_check"]
    blocks = [L.SfgsConsistencyArgs(L.C.sizeof(L.SfgsConsistencyArgs), len(vs), i, H, W, PARAMS["min_views"], vs._table.data_ptr(),
                                    PARAMS["rel_tol"], PARAMS["px_tol"] * PARAMS["px_tol"]) for i, (H, W) in enumerate(vs.sizes)]
    stream = L.C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(i, count, keep):
        rc = fn(L.C.byref(blocks[i]), L.ptr(count), L.ptr(keep), stream)
        assert rc == 0, rc
    return run


def layouts(variant, vs, rounds):
    from sfgs import _lib as L
    V = len(vs)
    outs = {k: [(torch.zeros(s, dtype=torch.uint8, device="cuda"), torch.zeros(s, dtype=torch.uint8, device="cuda")) for s in vs.sizes]
            for k in "ab"}
    runs = {"a": raw_check(L.LIB_PATH, vs), "b": raw_check(variant, vs)}
    times = {"a": [], "b": []}
    for r in range(rounds + 1):                                               # the first round warms both up
        for k in "ab":
            _, ms = device_ms(lambda: [runs[k](i, *outs[k][i]) for i in range(V)])
            if r:
                times[k].append(ms / V)
    same = all(bool((x == y).all()) for a, b in zip(outs["a"], outs["b"]) for x, y in zip(a, b))
    med = lambda xs: float(np.median(xs))
    return {"committed_tile_16x16_ms_per_view": times["a"], "variant_row_major_ms_per_view": times["b"],
            "variant": os.path.basename(variant), "committed_over_variant": med(times["a"]) / med(times["b"]),
            "committed_faster_in_every_round": all(x < y for x, y in zip(times["a"], times["b"])), "outputs_equal": same}


def main():
    variant = sys.argv[sys.argv.index("--variant") + 1] if "--variant" in sys.argv else None
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    grid, cams, depths, _, _ = bg.make_case()
    V, (H, W) = len(depths), depths[0].shape
    host_views = [cnp.View(d.cpu().numpy(), c, None) for d, c in zip(depths, cams)]
    vs = ViewSet(depths, cams)

    # (a)
    for _ in range(2):
        vs.check(0, **PARAMS)
    torch.cuda.synchronize()
    rounds, branches = [], {}
    for _ in range(ROUNDS):
        (count, keep), ms = device_ms(lambda: vs.check(0, **PARAMS))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want_count, want_keep = cnp.check(host_views, 0, branches=branches, **PARAMS)
        host_s = time.perf_counter() - t0
        equal = bool((count.cpu().numpy() == want_count).all() and (keep.cpu().numpy() == want_keep).all())
        rounds.append({"device_ms": ms, "host_s": host_s, "host_over_device": host_s * 1e3 / ms, "equal_bytes": equal})
    pairs_view = (V - 1) * H * W
    reached = sum(branches[k] for k in cnp.BRANCHES[1:])                      # pairs that load the source's depth

    # (b)
    for i in range(V):
        vs.check(i, **PARAMS)
    torch.cuda.synchronize()
    per_view = [[device_ms(lambda i=i: vs.check(i, **PARAMS))[1] for i in range(V)] for _ in range(ROUNDS)]
    set_ms = [sum(r) for r in per_view]
    med_set = float(np.median(set_ms))

    # (d)
    forms = layouts(variant, vs, max(ROUNDS, 5)) if variant else None

    # (c)
    terrain = gnp.make_terrain(bg.CELLS, bg.CELLS, 2024, boxes=60)
    truth = torch.from_numpy(terrain + bg.ORIGIN[2]).cuda()
    blurred = [torch.from_numpy(cnp.blur3(v.depth)).cuda() for v in host_views]
    plain = geo.evaluate_dsm(blurred, cams, grid, truth, origin=bg.ORIGIN)
    filtered = geo.evaluate_dsm(blurred, cams, grid, truth, origin=bg.ORIGIN, consistency=PARAMS)
    sharp_plain = geo.evaluate_dsm(depths, cams, grid, truth, origin=bg.ORIGIN)
    sharp_filtered = geo.evaluate_dsm(depths, cams, grid, truth, origin=bg.ORIGIN, consistency=PARAMS)

    faster = all(r["device_ms"] < r["host_s"] * 1e3 for r in rounds)
    equal = all(r["equal_bytes"] for r in rounds)
    med = lambda xs: float(np.median(xs))
    result = {
        "tool": "bench_consistency", "views": V, "depth_size": [H, W], "params": PARAMS, "gpu": torch.cuda.get_device_name(0),
        "a_one_reference_view": {
            "pairs": pairs_view, "rounds": rounds, "median_device_ms": med([r["device_ms"] for r in rounds]),
            "median_host_s": med([r["host_s"] for r in rounds]),
            "host_ns_per_pair": med([r["host_s"] for r in rounds]) * 1e9 / pairs_view,
            "device_ns_per_pair": med([r["device_ms"] for r in rounds]) * 1e6 / pairs_view,
            "ratio_of_medians": med([r["host_s"] for r in rounds]) * 1e3 / med([r["device_ms"] for r in rounds]),
            "branches_view0": branches, "kept_fraction_view0": float(want_keep.mean()),
            "bytes_gathered_view0": 4 * reached, "gathered_fraction_of_pairs_view0": reached / pairs_view},
        "b_all_reference_views": {
            "set_ms_per_round": set_ms, "median_set_ms": med_set, "median_ms_per_view": med_set / V,
            "min_max_ms_per_view": [float(np.min(per_view)), float(np.max(per_view))],
            "pairs": V * pairs_view, "pairs_per_second": V * pairs_view / (med_set * 1e-3),
            "bytes_gathered_upper_bound": 4 * V * pairs_view,
            "gather_GB_per_s_upper_bound": 4 * V * pairs_view / (med_set * 1e-3) / 1e9},
        "c_evaluate_dsm_blurred_depths": {"unfiltered": plain, "filtered": filtered, "mae_unfiltered_m": plain["mae"],
                                          "mae_filtered_m": filtered["mae"]},
        "c_evaluate_dsm_unblurred_depths": {"unfiltered": sharp_plain, "filtered": sharp_filtered},
        "d_lane_layouts": forms,
        "device_faster_in_every_round": faster, "equal_bytes_in_every_round": equal,
        "baseline": "vectorised numpy restatement (tests/consistency_np.py), float64, depth maps already on the host",
    }
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    sys.exit(0 if faster and equal else 1)


if __name__ == "__main__":
    main()
