#!/usr/bin/env python
"""Measuring a mesh: Mesh.face_grid, Mesh.sample and Mesh.closest (csrc/mesh_query.hip) on the cleaned mesh of the city volume of
tools/bench_tsdf.py (24 depth maps of 1024 x 1024 fused into 512 x 512 x 128 voxels of 1 m, extracted, welded, cleaned: about 4 M
faces) and on its decimations at 2 and 4 voxels.

  grid        face_grid of the cleaned mesh in the volume's own frame at cell = 1, 2 and 4 voxels: time (with the one host read of
              the pair total), pairs per face, share of empty cells, longest cell list, length of the large list.
  sample      Mesh.sample of the cleaned mesh at one sample per voxel^2.
  decimation  the samples of the mesh decimated at 2 and at 4 voxels against the cleaned mesh, and the cleaned mesh's samples
              against the decimated one: mean, 99th percentile and maximum of the distance, in voxels -- the geometric error of
              Mesh.decimate. The grid of the mesh searched has cell = 2 voxels.
  cloud       the 24-view merged cloud of tools/bench_pointcloud.py (sfgs.pointcloud, float64 rows, world frame) against the
              cleaned mesh with max_distance = 4 voxels, and its summary (MeshDistance.summary).
  compare     sfgs.mesh.compare of the mesh decimated at 4 voxels and the cleaned mesh: Chamfer distance, precision, recall, F-score.
  --variant LIB  a second build of libsfgs.so (tools/build_variant.sh with tools/variants/mesh_query_wave.patch: a wave per
              query), sfgs_mesh_closest of both libraries alternating on every distance workload; the answers must be the same bytes.
  scale       the device's own brute force (_max_cells = 0) and the numpy restatement (tests/mesh_query_np.py) on the mesh
              decimated at 4 voxels with few queries; the three routes and the restatement must give the same bytes.
ROUNDS times each after a warm-up, events around the calls; the kernels' own times from torch.profiler in a run of their own.
Exits with status 1 unless every comparison of bytes holds.

usage: python tools/bench_mesh_distance.py [--variant LIB] [--out FILE]      env: ROUNDS=3 VIEWS=24 SIZE=1024 CELLS=1024 DIMS=512,512,128"""
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
import geometry_np as gnp  # noqa: E402
import mesh_query_np as mq  # noqa: E402
from sfgs import _lib as L  # noqa: E402
from sfgs import pointcloud  # noqa: E402
from sfgs.mesh import compare  # noqa: E402
from sfgs.tsdf import TsdfVolume  # noqa: E402

ROUNDS = bg.ROUNDS
DIMS = tuple(int(v) for v in os.environ.get("DIMS", "512,512,128").split(","))
BRUTE_QUERIES, NUMPY_QUERIES = 4096, 128


def device_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return out, start.elapsed_time(end)


def timed(fn):
    """-> (the last result, [ms] of ROUNDS calls after one warm-up)"""
    out, ts = fn(), []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        out, ms = device_ms(fn)
        ts.append(ms)
    return out, ts


def med(xs):
    return float(np.median(xs))


def kernel_times(fn):
    """-> {kernel name: microseconds} of the query kernels' launches inside fn(), or a note when the profiler cannot see them"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            if "mq_" in e.key or "vf_sort" in e.key:
                us = getattr(e, "device_time_total", None)
                us = getattr(e, "cuda_time_total", 0.0) if us is None else us
                name = e.key.split("(")[0].split("<")[0].replace("void ", "").replace("sfgs::", "")
                out[name] = out.get(name, 0.0) + float(us)
        return out or "torch.profiler saw none of the query kernels"
    except Exception as e:  # noqa: BLE001 -- a diagnostic; the timings above do not depend on it
        return f"torch.profiler unavailable: {type(e).__name__}: {e}"


VARIANT, EQUAL = None, [True]


def raw_closest(lib_path, grid, points, max_distance):
    """-> (run(), sqdist, face): sfgs_mesh_closest of the library at lib_path on a filled grid"""
    lib = L.C.CDLL(lib_path)
    fn = lib.sfgs_mesh_closest
    fn.restype, fn.argtypes = L.SYMBOLS["sfgs_mesh_closest"]
    k = int(points.shape[0])
    sq, face = torch.empty(k, dtype=torch.float64, device="cuda"), torch.empty(k, dtype=torch.int32, device="cuda")
    state = torch.empty(4, dtype=torch.int64, device="cuda")
    stream = L.C.c_void_p(torch.cuda.current_stream().cuda_stream)
    md = float("inf") if max_distance is None else float(max_distance)

    def run():
        rc = fn(L.C.byref(grid._args), L.ptr(points), int(points.dtype == torch.float64), k, md, L.ptr(sq), L.ptr(face), None, L.ptr(state), stream)
        assert rc == 0, rc
    return run, sq, face


def variant_row(points, grid, max_distance, committed):
    runs = {"a": raw_closest(L.LIB_PATH, grid, points, max_distance), "b": raw_closest(VARIANT, grid, points, max_distance)}
    times = {"a": [], "b": []}
    for r in range(ROUNDS + 1):
        for key in "ab":
            torch.cuda.synchronize()
            _, ms = device_ms(runs[key][0])
            if r:
                times[key].append(ms)
    same = all(torch.equal(runs[key][1], committed.sqdist) and torch.equal(runs[key][2], committed.face) for key in "ab")
    EQUAL[0] = EQUAL[0] and same
    return {"thread_per_query_ms": times["a"], "wave_per_query_ms": times["b"], "wave_over_thread": med(times["b"]) / med(times["a"]),
            "thread_faster_in_every_round": all(x < y for x, y in zip(times["a"], times["b"])), "outputs_equal": same}


def distance_row(points, mesh, grid, voxel, max_distance=None, thresholds=()):
    d, ts = timed(lambda: mesh.closest(points, grid, max_distance=max_distance))
    answered, without, skipped = d.check()
    dist = d.distance[d.face >= 0] / voxel
    extra = {}
    if thresholds:
        s, st = timed(lambda: d.summary([t * voxel for t in thresholds]))
        extra["summary"] = {"summary_ms": st, "median_summary_ms": med(st), "mean_voxels": s.mean / voxel, "rms_voxels": s.rms / voxel,
                            "max_voxels": s.max / voxel, "thresholds_voxels": list(thresholds), "fraction_of_queries_within": list(s.fractions)}
    if VARIANT:
        extra["variant"] = variant_row(points, grid, max_distance, d)
    return {**extra, "point_dtype": str(points.dtype), "max_distance_voxels": None if max_distance is None else max_distance / voxel, "queries": int(points.shape[0]), "answered": answered, "without_a_face": without, "closest_ms": ts, "median_closest_ms": med(ts),
            "queries_per_second": points.shape[0] / (med(ts) * 1e-3), "mean_voxels": float(dist.mean()),
            "p99_voxels": float(torch.quantile(dist[:: max(1, dist.numel() // 4_000_000)], 0.99)), "max_voxels": float(dist.max()),
            "kernels_us": kernel_times(lambda: mesh.closest(points, grid, max_distance=max_distance))}


def main():
    global VARIANT
    VARIANT = sys.argv[sys.argv.index("--variant") + 1] if "--variant" in sys.argv else None
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    _, cams, depths, _, _ = bg.make_case()
    V, (H, W) = len(depths), depths[0].shape
    terrain = gnp.make_terrain(bg.CELLS, bg.CELLS, 2024, boxes=60)
    side = bg.CELLS * bg.RES
    nx, ny, nz = DIMS
    voxel = side / nx
    origin = (0.0, 0.0, float(np.floor(terrain.min())) - 8.0 * voxel)
    vol = TsdfVolume(origin, DIMS, voxel, 3.0 * voxel, max_weight=64.0, colors=False, device="cuda")
    vol.add_views(depths, cams)
    cloud = pointcloud.PointCloud(V * H * W, device="cuda")
    for d, c in zip(depths, cams):
        cloud.add_view(d, c)
    cloud_points = cloud.result()[0]                                                # float64 [k,3], the world frame
    del depths
    cleaned = vol.extract(16 * nx * ny).mesh().clean(min_triangles=64, largest=1)
    meshes = {"cleaned": cleaned, "decimated_2_voxels": cleaned.decimate(2 * voxel, origin),
              "decimated_4_voxels": cleaned.decimate(4 * voxel, origin)}
    sizes = {k: [int(x) for x in m._sizes()] for k, m in meshes.items()}
    torch.cuda.synchronize()

    grids = {}
    for k in (1, 2, 4):
        dims = tuple(-(-d // k) for d in DIMS)
        grid, ts = timed(lambda: cleaned.face_grid(k * voxel, origin, dims))
        pairs, large, skipped = grid.check()
        lengths = grid.cell_start[1:] - grid.cell_start[:-1]
        grids[f"cell_{k}_voxels"] = {"dims": list(dims), "build_ms": ts, "median_build_ms": med(ts), "pairs": pairs,
                                     "pairs_per_face": pairs / max(sizes["cleaned"][1], 1), "empty_cell_share": float((lengths == 0).float().mean()),
                                     "longest_cell_list": int(lengths.max()), "large_list": large, "faces_left_out": skipped,
                                     "kernels_us": kernel_times(lambda: cleaned.face_grid(k * voxel, origin, dims))}
        del grid, lengths

    density = 1.0 / (voxel * voxel)
    samples, ts = timed(lambda: cleaned.sample(density, seed=1))
    sample_row = {"density_per_voxel2": 1.0, "samples": int(samples.points.shape[0]), "sample_ms": ts, "median_sample_ms": med(ts),
                  "kernels_us": kernel_times(lambda: cleaned.sample(density, seed=1))}

    dims2 = tuple(-(-d // 2) for d in DIMS)
    full_grid = cleaned.face_grid(2 * voxel, origin, dims2)
    decimation = {}
    for which in ("decimated_2_voxels", "decimated_4_voxels"):
        small = meshes[which]
        pts = small.sample(density, seed=2).points
        decimation[which] = {"vertices_faces": sizes[which],
                             "its_samples_to_the_cleaned_mesh": distance_row(pts, cleaned, full_grid, voxel),
                             "the_cleaned_meshs_samples_to_it": distance_row(samples.points, small, small.face_grid(2 * voxel, origin, dims2), voxel)}

    cloud_row = distance_row(cloud_points, cleaned, full_grid, voxel, max_distance=4 * voxel, thresholds=(0.25, 0.5, 1.0, 2.0, 4.0))
    taus = (0.25, 0.5, 1.0, 2.0)
    t0 = time.perf_counter()
    cmp = compare(meshes["decimated_4_voxels"], cleaned, density, max_distance=4 * voxel, thresholds=[t * voxel for t in taus], seed=3)
    torch.cuda.synchronize()
    compare_row = {"a": "decimated_4_voxels", "b": "cleaned", "wall_s_first_call": time.perf_counter() - t0, "chamfer_voxels": cmp.chamfer / voxel,
                   "thresholds_voxels": list(taus), "precision": list(cmp.precision), "recall": list(cmp.recall), "fscore": list(cmp.fscore),
                   "a_to_b_mean_max_voxels": [cmp.a_to_b.mean / voxel, cmp.a_to_b.max / voxel],
                   "b_to_a_mean_max_voxels": [cmp.b_to_a.mean / voxel, cmp.b_to_a.max / voxel]}

    # scale: the device's brute force and the restatement, and the byte comparisons
    small = meshes["decimated_4_voxels"]
    pts = samples.points[:: max(1, samples.points.shape[0] // BRUTE_QUERIES)][:BRUTE_QUERIES].contiguous()
    answers, rows = {}, {}
    for route in (0, None, 1 << 30):
        grid = small.face_grid(4 * voxel, _max_cells=route)
        d, ts = timed(lambda: small.closest(pts, grid, closest_points=True))
        answers[route] = d
        rows[str(route)] = {"closest_ms": ts, "median_closest_ms": med(ts)}
    equal = all(torch.equal(answers[r].sqdist, answers[None].sqdist) and torch.equal(answers[r].face, answers[None].face) and
                torch.equal(answers[r].point, answers[None].point) for r in (0, 1 << 30))
    Vh, Fh = small.vertices.cpu().numpy(), small.faces.cpu().numpy()
    Ph = pts[:NUMPY_QUERIES].cpu().numpy()
    t0 = time.perf_counter()
    sq, face, point, _ = mq.closest(Vh, Fh, Ph)
    host_s = time.perf_counter() - t0
    got = answers[None]
    equal_r = got.sqdist[:NUMPY_QUERIES].cpu().numpy().tobytes() == sq.tobytes() and \
        got.face[:NUMPY_QUERIES].cpu().numpy().tobytes() == face.tobytes() and got.point[:NUMPY_QUERIES].cpu().numpy().tobytes() == point.tobytes()
    result = {"tool": "bench_mesh_distance", "views_fused": V, "view_size": [H, W], "dims": list(DIMS), "voxel_size": voxel,
              "gpu": torch.cuda.get_device_name(0), "rounds": ROUNDS, "max_cells_default": mq.MAX_CELLS_DEFAULT, "meshes": sizes,
              "kernel_form": "a thread per query", "variant": None if VARIANT is None else os.path.basename(VARIANT),
              "merged_cloud_to_the_cleaned_mesh": cloud_row, "compare_decimated_4_voxels_with_cleaned": compare_row, "grid_of_the_cleaned_mesh": grids, "sample_of_the_cleaned_mesh": sample_row,
              "decimation_error": decimation,
              "scale_decimated_4_voxels": {"queries": int(pts.shape[0]), "device_by_max_cells": rows, "routes_equal_bytes": bool(equal),
                                           "numpy_queries": NUMPY_QUERIES, "numpy_s": host_s,
                                           "numpy_us_per_query": host_s * 1e6 / NUMPY_QUERIES, "numpy_equal_bytes": bool(equal_r)},
              "not_measured": ["queries bucketed by their starting cell (not built)", "a trained scene"],
              "every_comparison_of_bytes_holds": bool(equal and equal_r and EQUAL[0])}
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    sys.exit(0 if equal and equal_r and EQUAL[0] else 1)


if __name__ == "__main__":
    main()
