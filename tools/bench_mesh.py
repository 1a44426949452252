#!/usr/bin/env python
"""Mesh finishing alone: sfgs.mesh (csrc/mesh.hip) on the soups of two volumes -- the city of tools/bench_tsdf.py (24 depth maps
of 1024 x 1024 fused into 512 x 512 x 128 voxels) and tests/tsdf_np.wavy_volume -- each stage next to its host spelling, measured
in the same run on the same box, ROUNDS times after a warm-up:

  weld         TriangleSoup.mesh() (events around the call)   against  TriangleSoup.weld(), its device-to-host copy included
  components   Mesh.components()                              against  the numpy pass tests/mesh_np.components on the host's F
  clean        Mesh.clean(min_triangles=64, largest=1), the components handed in      (no host spelling exists; for scale only)
  save_ply     Mesh.save_ply (host clock, the copy included)  against  TriangleSoup.save_ply(weld=True)
  decimate     Mesh.decimate at cell = 2 x and 4 x the voxel  against  the numpy restatement tests/mesh_simplify_np.decimate
  vertex_faces Mesh.vertex_faces()                            against  mesh_simplify_np.vertex_faces (a stable argsort)
  normals      Mesh.vertex_normals(), with and without a prebuilt adjacency      against  mesh_simplify_np.vertex_normals

and checks that both sides describe the same mesh: byte-sorted device V equals the host weld's V, the numpy labels equal the
device's, and the restatement's bytes equal the device's for the three new stages. Per entry point it reports the time, the ALGORITHMIC bytes (every input read once, every output written once) over
8 TB/s, and for the weld the table's load factor (unique vertices / slots) and the mean probe length (a second, untimed weld with
probe_stats=True); for the decimation the same of its cluster table, and per kernel the algorithmic bytes over the
kernel's own time. Per kernel times come from torch.profiler when it can see the library's launches.
Exits with status 1 unless every comparison holds.

usage: python tools/bench_mesh.py [--out FILE] [--only city|wavy]      env: ROUNDS=3 VIEWS=24 SIZE=1024 CELLS=1024 DIMS=512,512,128"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_geometry as bg  # noqa: E402
import geometry_np as gnp  # noqa: E402
import mesh_np as mnp  # noqa: E402
import mesh_simplify_np as snp  # noqa: E402
import tsdf_np as tnp  # noqa: E402
from sfgs.tsdf import TsdfVolume  # noqa: E402

ROUNDS = bg.ROUNDS
DIMS = tuple(int(v) for v in os.environ.get("DIMS", "512,512,128").split(","))
HBM_BYTES_PER_S = 8.0e12
KERNELS = ("weld_", "cc_", "clean_", "compact_", "scan_sums_", "mesh_", "dec_", "vf_", "vn_")


def device_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return out, start.elapsed_time(end)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def med(xs):
    return float(np.median(xs))


def city_soup():
    _, cams, depths, _, _ = bg.make_case()
    terrain = gnp.make_terrain(bg.CELLS, bg.CELLS, 2024, boxes=60)
    nx, ny, nz = DIMS
    voxel = bg.CELLS * bg.RES / nx
    vol = TsdfVolume((0.0, 0.0, float(np.floor(terrain.min())) - 8.0 * voxel), DIMS, voxel, 3.0 * voxel, max_weight=64.0, device="cuda")
    vol.add_views(depths, cams)
    return vol.extract(16 * nx * ny), voxel, tuple(float(v) for v in vol.origin)


def wavy_soup():
    tsdf, weight, rgb, origin, voxel = tnp.wavy_volume((72, 64, 64), colors=True)
    nz, ny, nx = tsdf.shape
    vol = TsdfVolume(origin, (nx, ny, nz), voxel, trunc=1.0, colors=True, device="cuda")
    vol.load(torch.from_numpy(tsdf).cuda(), torch.from_numpy(weight).cuda(), torch.from_numpy(rgb).cuda())
    return vol.extract(200_000), float(voxel), tuple(float(v) for v in origin)


def kernel_times(fn):
    """-> {kernel name: microseconds} of the library's launches inside fn(), or a note when the profiler cannot see them"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            if any(k in e.key for k in KERNELS):
                us = getattr(e, "device_time_total", None)
                us = getattr(e, "cuda_time_total", 0.0) if us is None else us
                out[e.key.split("(")[0]] = out.get(e.key.split("(")[0], 0.0) + float(us)
        return out or "torch.profiler saw none of the library's kernels"
    except Exception as e:  # noqa: BLE001 -- a diagnostic; the timings above do not depend on it
        return f"torch.profiler unavailable: {type(e).__name__}: {e}"


def stage(name, algorithmic_bytes, device_times, host_times, timed_as):
    r = {"device_ms": device_times, "median_device_ms": med(device_times), "timed_as": timed_as, "algorithmic_bytes": algorithmic_bytes,
         "algorithmic_GB_per_s": algorithmic_bytes / (med(device_times) * 1e-3) / 1e9,
         "share_of_8_TB_per_s": algorithmic_bytes / (med(device_times) * 1e-3) / HBM_BYTES_PER_S}
    if host_times is not None:
        r.update({"host_ms": host_times, "median_host_ms": med(host_times), "host_over_device": med(host_times) / med(device_times),
                  "device_faster_in_every_round": all(d < h for d, h in zip(device_times, host_times))})
    return name, r


def per_kernel(times, bytes_of):
    """kernel name -> {us, algorithmic_bytes, share_of_8_TB_per_s} for the kernels whose bytes are stated"""
    if not isinstance(times, dict):
        return times
    out = {}
    for name, us in times.items():
        key = next((k for k in bytes_of if name.endswith(k) or k in name), None)
        out[name] = {"us": us}
        if key is not None and us > 0:
            out[name].update({"algorithmic_bytes": bytes_of[key], "share_of_8_TB_per_s": bytes_of[key] / (us * 1e-6) / HBM_BYTES_PER_S})
    return out


def same_bytes(t, a):
    return bool(t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes())


def run_simplify(mesh, voxel, origin):
    """The decimation, adjacency and normal stages on a welded mesh -> (stages, details, every comparison held)"""
    m, n = int(mesh.num_vertices), int(mesh.num_faces)
    k = 2 if mesh.color_buffer is not None else 1
    V, F = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    C = None if mesh.color_buffer is None else mesh.colors.cpu().numpy()
    stages, details, equal = {}, {}, True
    for factor in (2, 4):
        cell = factor * voxel
        mesh.decimate(cell, origin)                                                    # warm-up
        t_dev, t_host = [], []
        for r in range(ROUNDS):
            print(f"bench_mesh: decimate at {factor} voxels, round {r + 1} of {ROUNDS}", file=sys.stderr, flush=True)
            (out, vmap), ms = device_ms(lambda: mesh.decimate(cell, origin, return_map=True))
            t_dev.append(ms)
            want, ms = host_ms(lambda: snp.decimate(V, F, C, cell, origin))
            t_host.append(ms)
            equal &= same_bytes(out.vertices, want[0]) and same_bytes(out.faces, want[1]) and same_bytes(vmap, want[3])
            equal &= C is None or same_bytes(out.colors, want[2])
        info = want[4]
        kv, kf, K = len(want[0]), len(want[1]), info["clusters"]
        probed = mesh.decimate(cell, origin, probe_stats=True)
        slots = 64
        while slots < 6 * ((m + 2) // 3):
            slots *= 2
        name = f"decimate_{factor}_voxels"
        stages.update([stage(name, 12 * m * k + 12 * n + 12 * kv * k + 12 * kf, t_dev, t_host,
                             f"device: events around Mesh.decimate(cell={factor} voxels, return_map=True); host: mesh_simplify_np.decimate")])
        kernel_bytes = {"dec_cell_kernel": 12 * m + 13 * m, "weld_insert_kernel": 13 * m + 8 * m, "weld_rep_kernel": 10 * m,
                        "dec_sum_kernel": 12 * m * k + 8 * m + 4 * m + 28 * m + 24 * m * (k - 1), "dec_face_kernel": 24 * n + 26 * n,
                        "dec_mark_kernel": 13 * n, "dec_resolve_kernel": m + K * (12 + 24 * k + 12 * k), "clean_faces_kernel": n + 40 * kf,
                        "dec_map_kernel": 13 * m}
        details[name] = {"cell": cell, "clusters": K, "single_member_clusters": info["single"], "collapsed_faces": info["collapsed"],
                         "duplicate_faces": info["duplicates"], "unreferenced_clusters": info["unreferenced"],
                         "output": {"vertices": kv, "faces": kf, "faces_kept_share": kf / max(n, 1)},
                         "cluster_table": {"slots": slots, "load_factor": K / slots, "mean_probe_length": probed.weld_probes / max(m, 1)},
                         "kernels": per_kernel(kernel_times(lambda: mesh.decimate(cell, origin)), kernel_bytes),
                         "note": "weld_insert_kernel / weld_rep_kernel run twice (cells, then sorted triples): their times are the "
                                 "sums, their bytes those of the vertex pass"}
    adj = mesh.vertex_faces()
    mesh.vertex_normals(adj)
    mesh.vertex_normals()
    t_vf, t_vf_host, t_vn, t_vn_adj, t_vn_host = [], [], [], [], []
    for r in range(ROUNDS):
        print(f"bench_mesh: adjacency and normals, round {r + 1} of {ROUNDS}", file=sys.stderr, flush=True)
        got, ms = device_ms(lambda: mesh.vertex_faces())
        t_vf.append(ms)
        want, ms = host_ms(lambda: snp.vertex_faces(F, m))
        t_vf_host.append(ms)
        equal &= same_bytes(got.offsets, want[0]) and same_bytes(got.records, want[1]) and got.check() == 0
        normals, ms = device_ms(lambda: mesh.vertex_normals())
        t_vn.append(ms)
        with_adj, ms = device_ms(lambda: mesh.vertex_normals(adj))
        t_vn_adj.append(ms)
        want_n, ms = host_ms(lambda: snp.vertex_normals(V, F, want))
        t_vn_host.append(ms)
        equal &= same_bytes(normals, want_n) and same_bytes(with_adj, want_n)
    stages.update([
        stage("vertex_faces", 12 * n + 4 * m + 12 * n, t_vf, t_vf_host, "device: events around Mesh.vertex_faces(); host: stable argsort + bincount"),
        stage("vertex_normals", 12 * n + 12 * m + 12 * m, t_vn, t_vn_host,
              "device: events around Mesh.vertex_normals(), the adjacency built in the call; host: mesh_simplify_np.vertex_normals, adjacency given"),
        stage("vertex_normals_prebuilt_adjacency", 4 * m + 12 * n + 12 * n + 12 * m + 12 * m, t_vn_adj, t_vn_host,
              "device: events around Mesh.vertex_normals(adjacency); host: as above"),
    ])
    valence = np.diff(want[0])
    details["adjacency"] = {"max_valence": int(valence.max()), "mean_valence": float(valence.mean()),
                            "kernels": per_kernel(kernel_times(lambda: mesh.vertex_faces()),
                                                  {"vf_count_kernel": 12 * n + 4 * m, "vf_fill_kernel": 12 * n + 4 * m + 12 * n,
                                                   "vf_sort_kernel": 4 * m + 24 * n, "vf_offsets_kernel": 12 * m})}
    # the normal kernel reads per record a face (12 bytes) and three positions (36 bytes): gathers; algorithmic = each once
    details["normals"] = {"kernels": per_kernel(kernel_times(lambda: mesh.vertex_normals(adj)), {"vn_kernel": 4 * m + 24 * n + 24 * m}),
                          "gathered_bytes": 4 * m + 3 * n * (4 + 12 + 36) + 12 * m}
    return stages, details, equal


def run(soup, tmp, voxel=None, origin=None):
    from sfgs.mesh import weld
    n = int(soup.num_triangles)
    assert n <= soup.capacity, (n, soup.capacity)
    colours = soup.color_buffer is not None
    k = 2 if colours else 1
    # warm-up of every path (allocator, code objects), and the objects the later stages use
    mesh = soup.mesh()
    cc = mesh.components()
    cleaned = mesh.clean(min_triangles=64, largest=1, components=cc)
    m, count = int(mesh.num_vertices), cc.check()
    torch.cuda.synchronize()

    t_weld, t_weld_host, t_cc, t_cc_host, t_clean, t_ply, t_ply_host = [], [], [], [], [], [], []
    equal_weld = equal_labels = True
    for r in range(ROUNDS):
        print(f"bench_mesh: {n} triangles, round {r + 1} of {ROUNDS}", file=sys.stderr, flush=True)
        got, ms = device_ms(lambda: soup.mesh())
        t_weld.append(ms)
        (hostV, hostF), ms = host_ms(lambda: soup.weld())
        t_weld_host.append(ms)
        keys = got.vertices.cpu().numpy().view(np.dtype((np.void, 12))).reshape(-1)
        equal_weld &= bool(np.sort(keys).tobytes() == np.ascontiguousarray(hostV).tobytes()) and len(hostF) == n
        gcc, ms = device_ms(lambda: mesh.components())
        t_cc.append(ms)
        F_host = mesh.faces.cpu().numpy()
        want, ms = host_ms(lambda: mnp.components(F_host, m))
        t_cc_host.append(ms)
        equal_labels &= bool(gcc.labels.cpu().numpy().tobytes() == want[0].tobytes() and
                             gcc.triangles.cpu().numpy().tobytes() == want[1].tobytes() and gcc.check() == want[3])
        _, ms = device_ms(lambda: mesh.clean(min_triangles=64, largest=1, components=cc))
        t_clean.append(ms)
        _, ms = host_ms(lambda: mesh.save_ply(os.path.join(tmp, "device.ply")))
        t_ply.append(ms)
        _, ms = host_ms(lambda: soup.save_ply(os.path.join(tmp, "host.ply"), weld=True))
        t_ply_host.append(ms)
    probed = weld(soup.buffer, soup.color_buffer, n, probe_stats=True)
    slots = 64
    while slots < 6 * n:
        slots *= 2
    kept_v, kept_f = int(cleaned.num_vertices), int(cleaned.num_faces)
    stages = dict([
        stage("weld", 36 * n * k + 12 * m * k + 12 * n, t_weld, t_weld_host,
              "device: events around TriangleSoup.mesh(); host: TriangleSoup.weld(), the copy of the soup included"),
        stage("components", 12 * n + 12 * m, t_cc, t_cc_host, "device: events around Mesh.components(); host: numpy min-label pass on F"),
        stage("clean", 12 * n + 12 * m * k + 4 * m + 12 * kept_f + 12 * kept_v * k, t_clean, None,
              "events around Mesh.clean(min_triangles=64, largest=1, components=...)"),
        stage("save_ply", 12 * m * k + 12 * n, t_ply, t_ply_host,
              "host clock; device: Mesh.save_ply, the copy of V, F and colours included; host: TriangleSoup.save_ply(weld=True)"),
    ])
    simplify_stages, simplify, equal_simplify = run_simplify(mesh, voxel, origin)
    stages.update(simplify_stages)
    return {"triangles": n, "soup_records": 3 * n, "welded_vertices": m, "components": count, "colours": colours,
            "simplify": simplify, "equal_simplify": equal_simplify,
            "cleaned": {"vertices": kept_v, "faces": kept_f},
            "weld_table": {"slots": slots, "load_factor": m / slots, "mean_probe_length": probed.weld_probes / (3 * n)},
            "stages": stages, "equal_weld": equal_weld, "equal_labels": equal_labels,
            "kernels_us": {"weld": kernel_times(lambda: soup.mesh()), "components": kernel_times(lambda: mesh.components()),
                           "clean": kernel_times(lambda: mesh.clean(min_triangles=64, largest=1, components=cc))}}


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    result = {"tool": "bench_mesh", "gpu": torch.cuda.get_device_name(0), "rounds": ROUNDS, "dims": list(DIMS)}
    with tempfile.TemporaryDirectory() as tmp:
        for name, make in (("wavy", wavy_soup), ("city", city_soup)):
            if only in (None, name):
                soup, voxel, origin = make()
                result[name] = run(soup, tmp, voxel, origin)
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    ok = all(result[k]["equal_weld"] and result[k]["equal_labels"] and result[k]["equal_simplify"] for k in ("wavy", "city") if k in result)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
