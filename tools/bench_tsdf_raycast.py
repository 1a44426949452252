#!/usr/bin/env python
"""Ray-casting a TSDF volume alone: TsdfVolume.raycast / ray_skip (csrc/tsdf.hip) on the city volume of tools/bench_tsdf.py: 24
depth maps of 1024 x 1024 fused into 512 x 512 x 128 voxels of 1 m, then seen at 1024 x 1024 from three places: one of the fused
cameras, an oblique camera 45 degrees above the horizon, and a camera inside the volume.

  (a) per camera, three ways -- skip=False (every sample), a prebuilt ray_skip() table, skip=None (the table built in the call) --
      each with normals and colours (a coloured volume) and with neither (normals=False on a volume without colours);
      alternating, ROUNDS times after a warm-up, events around the call, out= reused. The three ways must give the same bytes.
  (b) ray_skip() alone: the table's build time.
  (c) samples per ray, from the host build of the product's header (tests/host_check/tsdf_raycast_check.cpp) on a 64 x 64 view
      from the same three places (the focal length scaled with the size): uniform against skipping, jumps, the longest jump.
  (d) the numpy restatement (tests/tsdf_raycast_np.py) on a 64 x 48 view from the fused camera, for scale, against the kernel on
      the same view; the two must be the same bytes.
  (e) --variant LIB: a second build of libsfgs.so whose kernel gives a wave a run of 64 pixels of one row instead of an 8 x 8
      tile (tools/variants/tsdf_raycast_row.patch through tools/build_variant.sh). sfgs_tsdf_raycast of both libraries on the
      coloured volume with normals, with the prebuilt table and without one, alternating; the views must be the same bytes.
Exits with status 1 unless every comparison of bytes holds.

usage: python tools/bench_tsdf_raycast.py [--variant LIB] [--out FILE]      env: ROUNDS=5 VIEWS=24 SIZE=1024 CELLS=1024 DIMS=512,512,128"""
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
import geometry_np as gnp  # noqa: E402
import tsdf_raycast_hostcheck as rhc  # noqa: E402
import tsdf_raycast_np as rnp  # noqa: E402
from sfgs import _lib as L  # noqa: E402
from sfgs.geometry import _check_view  # noqa: E402
from sfgs.tsdf import RayView, TsdfVolume  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", 5))
DIMS = tuple(int(v) for v in os.environ.get("DIMS", "512,512,128").split(","))
WAYS = ("skip_false", "prebuilt_table", "skip_none")


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
               for x, y in ((a.depth, b.depth), (a.normal, b.normal), (a.rgb, b.rgb)))


def scaled(cam, size):
    """The camera at size x size pixels with the field of view it has at SIZE"""
    f = size / bg.SIZE
    return types.SimpleNamespace(R=cam.R, T=cam.T, focal_x=cam.focal_x * f, focal_y=cam.focal_y * f, cx=cam.cx, cy=cam.cy)


def raw_raycast(lib_path, vol, cam, H, W, table, out):
    """-> run(): sfgs_tsdf_raycast of the library at lib_path on vol's buffers, into `out`"""
    lib = L.C.CDLL(lib_path)
    fn = lib.sfgs_tsdf_raycast
    fn.restype, fn.argtypes = L.SYMBOLS["sfgs_tsdf_raycast"]
    _, _, (M, c, _, cx_pix, cy_pix, fx, fy) = _check_view(vol.device, out.depth, cam.R, cam.T, cam.focal_x, cam.focal_y, cam.cx, cam.cy,
                                                          None, None, centre_from_view=True)
    ray = L.SfgsTsdfRay(L.C.sizeof(L.SfgsTsdfRay), H, W, M, c, cx_pix, cy_pix, fx, fy, 0.0, float("inf"), vol.voxel_size,
                        out.depth.data_ptr(), out.normal.data_ptr(), out.rgb.data_ptr())
    block = vol._struct()
    stream = L.C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        rc = fn(L.C.byref(block), L.C.byref(ray), L.ptr(table), 0 if table is None else table.numel(), stream)
        assert rc == 0, rc
    return run


def new_view(H, W):
    return RayView(*(torch.zeros((n, H, W), dtype=torch.float32, device="cuda") for n in (1, 3, 3)))


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
    places = {"fused_camera": cams[0],
              "oblique_45_degrees": gnp.look_down_camera(target, 45.0, 77.0, 3.0 * side, focal=2.6 * bg.SIZE),
              "inside_the_volume": gnp.look_down_camera(target, 35.0, 200.0, 0.3 * side, focal=0.8 * bg.SIZE)}
    c = places["inside_the_volume"].centre
    assert all(origin[a] + 0.5 * voxel <= c[a] <= origin[a] + (DIMS[a] - 0.5) * voxel for a in range(3)), c

    coloured = TsdfVolume(origin, DIMS, voxel, 3.0 * voxel, colors=True, device="cuda")
    v, u = torch.meshgrid(torch.arange(H, device="cuda") / H, torch.arange(W, device="cuda") / W, indexing="ij")
    image = torch.stack([u, v, 0.5 * (u + v)]).float().contiguous()
    coloured.add_views(depths, cams, images=[image] * V)
    plain = TsdfVolume(origin, DIMS, voxel, 3.0 * voxel, device="cuda").load(coloured.tsdf, coloured.weight)
    del depths
    torch.cuda.synchronize()

    # (b)
    coloured.ray_skip()
    torch.cuda.synchronize()
    ms_table = [device_ms(coloured.ray_skip)[1] for _ in range(ROUNDS)]
    tables = {"full": coloured.ray_skip(), "bare": plain.ray_skip()}
    flagged = int(tables["full"].table.sum().item())

    # (a)
    volumes = {"full": (coloured, True), "bare": (plain, False)}
    a, equal = {}, True
    for place, cam in places.items():
        a[place] = {}
        for kind, (vol, normals) in volumes.items():
            skips = {"skip_false": False, "prebuilt_table": tables[kind], "skip_none": None}
            outs = {w: vol.raycast(cam, H, W, normals=normals, skip=skips[w]) for w in WAYS}     # the warm-up, and the out= tensors
            times = {w: [] for w in WAYS}
            for _ in range(ROUNDS):
                for w in WAYS:
                    torch.cuda.synchronize()
                    times[w].append(device_ms(lambda: vol.raycast(cam, H, W, normals=normals, skip=skips[w], out=outs[w]))[1])
            same = same_bytes(outs["skip_false"], outs["prebuilt_table"]) and same_bytes(outs["skip_false"], outs["skip_none"])
            equal = equal and same
            a[place][kind] = {"ms": times, "median_ms": {w: med(times[w]) for w in WAYS}, "equal_bytes": same,
                              "hit_pixels": int((outs["skip_false"].depth > 0).sum().item()),
                              "skip_none_over_skip_false": med(times["skip_none"]) / med(times["skip_false"]),
                              "skip_none_faster_in_every_round": all(x < y for x, y in zip(times["skip_none"], times["skip_false"]))}

    # (e)
    shapes = None
    if variant:
        shapes = {}
        for place, cam in places.items():
            shapes[place] = {}
            for way, table in (("prebuilt_table", tables["full"].table), ("skip_false", None)):
                outs = {"a": new_view(H, W), "b": new_view(H, W)}
                runs = {"a": raw_raycast(L.LIB_PATH, coloured, cam, H, W, table, outs["a"]),
                        "b": raw_raycast(variant, coloured, cam, H, W, table, outs["b"])}
                times = {"a": [], "b": []}
                for r in range(ROUNDS + 1):
                    for k in "ab":
                        torch.cuda.synchronize()
                        _, ms = device_ms(runs[k])
                        if r:
                            times[k].append(ms)
                same = same_bytes(outs["a"], outs["b"])
                equal = equal and same
                shapes[place][way] = {"committed_tile_8x8_ms": times["a"], "variant_row_64x1_ms": times["b"],
                                      "committed_over_variant": med(times["a"]) / med(times["b"]),
                                      "committed_faster_in_every_round": all(x < y for x, y in zip(times["a"], times["b"])),
                                      "outputs_equal": same}

    # (c), (d): on the host
    tsdf, weight = coloured.tsdf.cpu().numpy(), coloured.weight.cpu().numpy()
    samples = {}
    for place, cam in places.items():
        small = scaled(cam, 64)
        uniform = rhc.raycast(tsdf, weight, None, origin, voxel, small, 64, 64, normals=False, skip=False)
        skipping = rhc.raycast(tsdf, weight, None, origin, voxel, small, 64, 64, normals=False, skip=True)
        equal = equal and uniform.depth.tobytes() == skipping.depth.tobytes()
        samples[place] = {"uniform_per_ray": uniform.samples / 4096, "skipping_per_ray": skipping.samples / 4096,
                          "jumps_per_ray": skipping.jumps / 4096, "longest_jump": skipping.longest, "longest_run": skipping.longest_run,
                          "hit_pixels": int((uniform.depth > 0).sum())}
    small = types.SimpleNamespace(**{**vars(scaled(cams[0], 64)), "cy": 0.0})
    t0 = time.perf_counter()
    ref = rnp.raycast(tsdf, weight, None, origin, voxel, small, 48, 64)
    host_s = time.perf_counter() - t0
    plain.raycast(small, 48, 64)
    torch.cuda.synchronize()
    view, dev_ms = device_ms(lambda: plain.raycast(small, 48, 64))
    equal_d = view.depth.cpu().numpy().tobytes() == ref.depth.tobytes() and view.normal.cpu().numpy().tobytes() == ref.normal.tobytes()

    result = {"tool": "bench_tsdf_raycast", "views_fused": V, "view_size": [H, W], "dims": list(DIMS), "voxel_size": voxel,
              "step": voxel, "gpu": torch.cuda.get_device_name(0), "rounds": ROUNDS,
              "a_ms_per_view": a,
              "b_table": {"ms": ms_table, "median_ms": med(ms_table), "bricks": int(tables["full"].table.numel()), "flagged": flagged},
              "c_samples_per_ray_64x64": samples,
              "e_wave_shapes": shapes, "variant": None if variant is None else os.path.basename(variant),
              "d_restatement_64x48": {"host_s": host_s, "device_ms": dev_ms, "host_over_device": host_s * 1e3 / dev_ms,
                                      "hits": ref.hits, "equal_bytes": equal_d},
              "every_comparison_of_bytes_holds": bool(equal and equal_d)}
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    sys.exit(0 if equal and equal_d else 1)


if __name__ == "__main__":
    main()
