#!/usr/bin/env python
"""Rendering a mesh alone: Mesh.render (csrc/mesh_raster.hip) at 1024 x 1024 on the mesh of the city volume of tools/bench_tsdf.py
(24 depth maps of 1024 x 1024 fused into 512 x 512 x 128 voxels of 1 m, extracted, welded, cleaned: about 4 M faces).

  workloads   the cleaned mesh from a fused, an oblique and an inside camera (faces below a pixel); the mesh decimated at 2 and at 4
              voxels from the fused camera (faces of several pixels); a close-up of the cleaned mesh (faces of hundreds of pixels);
              two faces that fill the frame. ROUNDS times each after a warm-up, events around the call, out= reused, with colours
              and flat normals; the kernels' own times from torch.profiler.
  yardsticks  TsdfVolume.raycast of the same camera with a prebuilt ray_skip() table, in the same run; the numpy restatement
              (tests/mesh_render_np.py) on a 64 x 64 view of the mesh decimated at 4 voxels, for scale, against the kernels on the
              same view: the two must be the same bytes.
  sweep       _small_max over SWEEP on every workload: which faces their own thread rasterises. Every value must give the same bytes.
  --variant LIB  a second build of libsfgs.so (tools/build_variant.sh with a patch of tools/variants/), sfgs_mesh_render of both
              libraries alternating on every workload; the views must be the same bytes.
  difference  |rendered depth of the cleaned mesh - ray-cast depth of the volume| from the fused camera where both hit, in voxels.
Exits with status 1 unless every comparison of bytes holds.

usage: python tools/bench_mesh_render.py [--variant LIB] [--out FILE]      env: ROUNDS=3 VIEWS=24 SIZE=1024 CELLS=1024 DIMS=512,512,128"""
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_geometry as bg  # noqa: E402
import consistency_np as cnp  # noqa: E402
import geometry_np as gnp  # noqa: E402
import mesh_render_np as mr  # noqa: E402
from sfgs import _lib as L  # noqa: E402
from sfgs.geometry import _check_view  # noqa: E402
from sfgs.mesh import Mesh, MeshView  # noqa: E402
from sfgs.tsdf import TsdfVolume  # noqa: E402

ROUNDS = bg.ROUNDS
DIMS = tuple(int(v) for v in os.environ.get("DIMS", "512,512,128").split(","))
SWEEP = (0, 4, 16, 64, 256, 1024, 4096)


def device_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return out, start.elapsed_time(end)


def med(xs):
    return float(np.median(xs))


def same_bytes(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32))
               for x, y in ((a.depth, b.depth), (a.face, b.face), (a.normal, b.normal), (a.rgb, b.rgb))) and \
        torch.equal(a.counts, b.counts)


def kernel_times(fn):
    """-> {kernel name: microseconds} of the rasteriser's launches inside fn(), or a note when the profiler cannot see them"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            if "mr_" in e.key:
                us = getattr(e, "device_time_total", None)
                us = getattr(e, "cuda_time_total", 0.0) if us is None else us
                name = e.key.split("(")[0].split("<")[0].replace("void ", "").replace("sfgs::", "")
                out[name] = out.get(name, 0.0) + float(us)
        return out or "torch.profiler saw none of the rasteriser's kernels"
    except Exception as e:  # noqa: BLE001 -- a diagnostic; the timings above do not depend on it
        return f"torch.profiler unavailable: {type(e).__name__}: {e}"


def new_view(H, W, colours=True):
    return MeshView(torch.zeros((1, H, W), device="cuda"), torch.zeros((H, W), dtype=torch.int32, device="cuda"),
                    torch.zeros((3, H, W), device="cuda"), torch.zeros((3, H, W), device="cuda") if colours else None,
                    torch.zeros(8, dtype=torch.int64, device="cuda"))


def raw_render(lib_path, mesh, cam, H, W, out):
    """-> run(): sfgs_mesh_render of the library at lib_path on the mesh's buffers, into `out` (flat normals, the default route)"""
    lib = L.C.CDLL(lib_path)
    fn, sb = lib.sfgs_mesh_render, lib.sfgs_mesh_render_scratch_bytes
    fn.restype, fn.argtypes = L.SYMBOLS["sfgs_mesh_render"]
    sb.restype, sb.argtypes = L.SYMBOLS["sfgs_mesh_render_scratch_bytes"]
    _, _, (M, c, _, cx_pix, cy_pix, fx, fy) = _check_view(mesh.device, out.depth, cam.R, cam.T, cam.focal_x, cam.focal_y,
                                                          getattr(cam, "cx", 0.0), getattr(cam, "cy", 0.0), None, None, centre_from_view=True)
    m, n = mesh._sizes()
    args = L.SfgsMeshRender(L.C.sizeof(L.SfgsMeshRender), H, W, 0, M, c, cx_pix, cy_pix, fx, fy, 0.0, float("inf"), m, n, -1,
                            mesh.vertex_buffer.data_ptr(), None if mesh.color_buffer is None else mesh.color_buffer.data_ptr(),
                            mesh.face_buffer.data_ptr(), None, out.depth.data_ptr(), out.face.data_ptr(), out.normal.data_ptr(),
                            None if out.rgb is None else out.rgb.data_ptr(), out._state.data_ptr())
    scratch = torch.empty(sb(m, n, H, W), dtype=torch.uint8, device="cuda")
    stream = L.C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        rc = fn(L.C.byref(args), L.ptr(scratch), scratch.numel(), stream)
        assert rc == 0, rc
    return run


def box_pixels(mesh, cam, H, W):
    """median, 99th percentile and maximum of the clipped boxes of the faces all of whose vertices lie in front of the camera, in
    pixels: a diagnostic formed on the device in float64 (floor / ceil of the projected corners, not the rasteriser's snap)"""
    k = cnp.constants(cam, H, W)
    M, c = torch.from_numpy(k.M).cuda(), torch.from_numpy(k.c).cuda()
    p = (mesh.vertices.double() - c) @ M.T
    z = p[:, 2]
    u, v = p[:, 0] * k.focal_x / z + k.cx_pix, p[:, 1] * k.focal_y / z + k.cy_pix
    F = mesh.faces.long()
    ok = (z[F] > 0).all(dim=1)
    fu, fv = u[F][ok], v[F][ok]
    c0, c1 = fu.min(dim=1).values.ceil().clamp(min=0), fu.max(dim=1).values.floor().clamp(max=W - 1)
    r0, r1 = fv.min(dim=1).values.ceil().clamp(min=0), fv.max(dim=1).values.floor().clamp(max=H - 1)
    px = ((c1 - c0 + 1) * (r1 - r0 + 1))[(c0 <= c1) & (r0 <= r1)].cpu().numpy()
    return {"faces_with_a_box": int(len(px)), "median": float(np.median(px)) if len(px) else 0.0,
            "p99": float(np.percentile(px, 99)) if len(px) else 0.0, "max": int(px.max()) if len(px) else 0}


def main():
    variant = sys.argv[sys.argv.index("--variant") + 1] if "--variant" in sys.argv else None
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    _, cams, depths, _, _ = bg.make_case()
    V, (H, W) = len(depths), depths[0].shape
    terrain = gnp.make_terrain(bg.CELLS, bg.CELLS, 2024, boxes=60)
    side = bg.CELLS * bg.RES
    nx, ny, nz = DIMS
    voxel = side / nx
    origin = (0.0, 0.0, float(np.floor(terrain.min())) - 8.0 * voxel)
    target = np.array([side / 2, side / 2, 12.0])
    vol = TsdfVolume(origin, DIMS, voxel, 3.0 * voxel, max_weight=64.0, colors=True, device="cuda")
    v, u = torch.meshgrid(torch.arange(H, device="cuda") / H, torch.arange(W, device="cuda") / W, indexing="ij")
    image = torch.stack([u, v, 0.5 * (u + v)]).float().contiguous()
    vol.add_views(depths, cams, images=[image] * V)
    del depths
    table = vol.ray_skip()
    full = vol.extract(16 * nx * ny).mesh()
    cleaned = full.clean(min_triangles=64, largest=1)
    meshes = {"cleaned": cleaned, "decimated_2_voxels": cleaned.decimate(2 * voxel, origin),
              "decimated_4_voxels": cleaned.decimate(4 * voxel, origin)}
    quad = Mesh(torch.tensor([[-20.0, -30.0, 0.5], [W + 80.0, -25.0, 0.0], [W + 90.0, H + 70.0, 1.0], [-15.0, H + 60.0, 0.25]], device="cuda"),
                torch.tensor([[0, 3, 1], [1, 3, 2]], dtype=torch.int32, device="cuda"),
                torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.5, 0.5, 0.5]], device="cuda"))
    meshes["quad"] = quad
    fused, oblique = cams[0], gnp.look_down_camera(target, 45.0, 77.0, 3.0 * side, focal=2.6 * bg.SIZE)
    inside = gnp.look_down_camera(target, 35.0, 200.0, 0.3 * side, focal=0.8 * bg.SIZE)
    close = gnp.look_down_camera(target, 60.0, 30.0, 40.0, focal=1.0 * bg.SIZE)
    workloads = {"cleaned_fused_camera": ("cleaned", fused), "cleaned_oblique_45_degrees": ("cleaned", oblique),
                 "cleaned_inside_the_volume": ("cleaned", inside), "decimated_2_voxels_fused_camera": ("decimated_2_voxels", fused),
                 "decimated_4_voxels_fused_camera": ("decimated_4_voxels", fused), "cleaned_close_up": ("cleaned", close),
                 "quad_two_faces": ("quad", mr.pixel_camera(W, H))}
    sizes = {k: [int(x) for x in m._sizes()] for k, m in meshes.items()}
    torch.cuda.synchronize()

    equal, rows = True, {}
    for name, (which, cam) in workloads.items():
        mesh = meshes[which]
        out = mesh.render(cam, H, W)                                                    # the warm-up, and the out= tensors
        ray = None if which == "quad" else vol.raycast(cam, H, W, skip=table)
        t_render, t_ray = [], []
        for _ in range(ROUNDS):
            torch.cuda.synchronize()
            t_render.append(device_ms(lambda: mesh.render(cam, H, W, out=out))[1])
            if ray is not None:
                torch.cuda.synchronize()
                t_ray.append(device_ms(lambda: vol.raycast(cam, H, W, skip=table, out=ray))[1])
        sweep = {}
        for sm in SWEEP:
            o = mesh.render(cam, H, W, _small_max=sm)
            ts = []
            for _ in range(ROUNDS):
                torch.cuda.synchronize()
                ts.append(device_ms(lambda: mesh.render(cam, H, W, _small_max=sm, out=o))[1])
            sweep[str(sm)] = med(ts)
            equal = equal and same_bytes(o, out)
        rows[name] = {"mesh": which, "vertices_faces": sizes[which], "render_ms": t_render, "median_render_ms": med(t_render),
                      "raycast_prebuilt_table_ms": t_ray or None, "median_raycast_ms": med(t_ray) if t_ray else None,
                      "render_over_raycast": med(t_render) / med(t_ray) if t_ray else None,
                      "counts_drawn_culled_clipped_degenerate": list(out.check()), "hit_pixels": int((out.depth > 0).sum().item()),
                      "box_pixels": box_pixels(mesh, cam, H, W),
                      "kernels_us": kernel_times(lambda: mesh.render(cam, H, W, out=out)), "small_max_sweep_median_ms": sweep}
        if variant:
            outs = {"a": new_view(H, W), "b": new_view(H, W)}
            runs = {"a": raw_render(L.LIB_PATH, mesh, cam, H, W, outs["a"]), "b": raw_render(variant, mesh, cam, H, W, outs["b"])}
            times = {"a": [], "b": []}
            for r in range(ROUNDS + 1):
                for k in "ab":
                    torch.cuda.synchronize()
                    _, ms = device_ms(runs[k])
                    if r:
                        times[k].append(ms)
            same = same_bytes(outs["a"], outs["b"]) and same_bytes(outs["a"], out)
            equal = equal and same
            rows[name]["variant"] = {"committed_ms": times["a"], "variant_ms": times["b"], "committed_over_variant": med(times["a"]) / med(times["b"]),
                                     "committed_faster_in_every_round": all(x < y for x, y in zip(times["a"], times["b"])),
                                     "outputs_equal": same}

    # the difference to the ray-cast volume, fused camera
    a, b = cleaned.render(fused, H, W).depth, vol.raycast(fused, H, W, skip=table).depth
    both = (a > 0) & (b > 0)
    diff = ((a - b).abs()[both] / voxel).double().cpu().numpy()
    difference = {"pixels_both_hit": int(both.sum().item()), "mesh_only": int(((a > 0) & ~(b > 0)).sum().item()),
                  "raycast_only": int((~(a > 0) & (b > 0)).sum().item()), "median_voxels": float(np.median(diff)),
                  "p99_voxels": float(np.percentile(diff, 99))}

    # the restatement, for scale
    small_mesh = meshes["decimated_4_voxels"]
    f = 64 / bg.SIZE
    small = types.SimpleNamespace(R=fused.R, T=fused.T, focal_x=fused.focal_x * f, focal_y=fused.focal_y * f, cx=fused.cx, cy=fused.cy)
    Vh, Fh, Ch = small_mesh.vertices.cpu().numpy(), small_mesh.faces.cpu().numpy(), small_mesh.colors.cpu().numpy()
    t0 = time.perf_counter()
    ref = mr.render(Vh, Fh, Ch, small, 64, 64)
    host_s = time.perf_counter() - t0
    small_mesh.render(small, 64, 64)
    torch.cuda.synchronize()
    host_rounds, dev_rounds = [host_s], []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        view, ms = device_ms(lambda: small_mesh.render(small, 64, 64))
        dev_rounds.append(ms)
    equal_r = all(getattr(view, k).cpu().numpy().tobytes() == getattr(ref, k).tobytes() for k in ("depth", "face", "normal", "rgb")) and \
        view.counts.tolist() == ref.counts.tolist()
    result = {"tool": "bench_mesh_render", "views_fused": V, "view_size": [H, W], "dims": list(DIMS), "voxel_size": voxel,
              "gpu": torch.cuda.get_device_name(0), "rounds": ROUNDS, "small_max_default": mr.SMALL_MAX_DEFAULT,
              "workloads": rows, "variant": None if variant is None else os.path.basename(variant),
              "depth_difference_to_raycast_fused_camera": difference,
              "restatement_64x64_decimated_4_voxels": {"host_s": host_rounds, "device_ms": dev_rounds,
                                                       "host_over_device": host_s * 1e3 / med(dev_rounds),
                                                       "device_faster_in_every_round": all(d < host_s * 1e3 for d in dev_rounds),
                                                       "hit_pixels": int((ref.depth > 0).sum()), "equal_bytes": bool(equal_r)},
              "every_comparison_of_bytes_holds": bool(equal and equal_r)}
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    sys.exit(0 if equal and equal_r else 1)


if __name__ == "__main__":
    main()
