#!/usr/bin/env python
"""Golden vectors of sfgs.transform, from the reference's OWN code:

(a) utils.sh_utils.eval_sh on fixed random coefficients [P,3,16] and 64 fixed unit directions, at degrees 0 ... 3 (float32, as
    the renderer calls it): what pins the basis order and signs that sh_rotation's matrices are defined in.
(b) scene.dataset_readers.readSatelliteInfo on a tiny synthetic satellite dataset built in a temporary directory
    (points3D.txt, transforms_train.json / transforms_test.json with R, T and transform_matrix_rotated, 4 x 4 PNGs). Kept:
    the input points, R_fix, T_fix, every camera's (R, T) as readSatelliteCamerasFromTransforms returns it and as
    readSatelliteInfo leaves it, and the normalised points read back from the points3D.ply the reader wrote (float32).
    The reference only PRINTS scale and z_min; the fixture holds them as restated from lines 381-390 on the same points, and
    the test checks that they reproduce the PLY.

Runs only in the authoring container (it imports /root/reference read-only and stubs the third-party modules this image
lacks, as the other generators do; plyfile is sfgs.ply's stand-in). Everything runs on the CPU. Only data goes into the npz.

usage: python tests/golden/make_golden_transform.py [--check]     (--check: regenerate and compare with the committed file)
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "reference_transform.npz")
N_DIRS, N_SH, N_POINTS = 64, 6, 200


def import_reference():
    sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
    from sfgs import ply as sply
    sply.install_as_plyfile()
    for name in ("OpenEXR", "Imath", "mediapy"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    from scene import dataset_readers
    from utils import sh_utils
    return dataset_readers, sh_utils


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def sh_part(sh_utils):
    rng = np.random.default_rng(20240)
    dirs = rng.normal(size=(N_DIRS, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    sh = rng.normal(size=(N_SH, 3, 16)) * 0.15
    sh[:, :, 0] = rng.uniform(0.5, 1.5, size=(N_SH, 3))        # colours + 0.5 stay positive: the renderer's clamp at 0 hides nothing
    out = {"sh_dirs": dirs, "sh_coeffs": sh.astype(np.float32)}
    d32, s32 = torch.tensor(dirs, dtype=torch.float32), torch.tensor(sh, dtype=torch.float32)
    for deg in range(4):
        # every coefficient set at every direction: [N_SH, N_DIRS, 3]
        out[f"sh_colour_deg{deg}"] = sh_utils.eval_sh(deg, s32[:, None], d32[None]).numpy().astype(np.float32)
    return out


def write_dataset(path, rng):
    from PIL import Image
    R_fix, T_fix = rotation(rng), rng.normal(size=3) * 30.0
    pts = rng.normal(size=(N_POINTS, 3)) * np.array([400.0, 300.0, 40.0]) + np.array([1000.0, -2000.0, 150.0])
    with open(os.path.join(path, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n")
        for i, p in enumerate(pts):
            r, g, b = (int(v) for v in rng.integers(0, 256, size=3))
            f.write(f"{i + 1} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {r} {g} {b} 0.5 1 0\n")
    os.makedirs(os.path.join(path, "images"))
    R4 = np.eye(4)
    R4[:3, :3] = R_fix
    for split, count in (("train", 3), ("test", 2)):
        frames = []
        for i in range(count):
            name = f"images/{split}_{i}.png"
            Image.fromarray(rng.integers(1, 256, size=(4, 4, 3), dtype=np.uint8)).save(os.path.join(path, name))
            c2w = np.eye(4)
            c2w[:3, :3] = rotation(rng)
            c2w[:3, 3] = rng.normal(size=3) * 500.0 + np.array([0.0, 0.0, 3000.0])
            frames.append({"file_path": name, "transform_matrix_rotated": c2w.tolist(), "fl_x": 900.0 + i, "fl_y": 910.0 + i,
                           "cx": 2.0, "cy": 2.0})
        with open(os.path.join(path, f"transforms_{split}.json"), "w") as f:
            json.dump({"R": R4.tolist(), "T": T_fix.tolist(), "frames": frames}, f)
    return pts, R_fix, T_fix


def satellite_part(dataset_readers):
    rng = np.random.default_rng(20241)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        pts, R_fix, T_fix = write_dataset(tmp, rng)
        before = []
        for split in ("train", "test"):
            with contextlib.redirect_stdout(io.StringIO()):
                cams, R, T = dataset_readers.readSatelliteCamerasFromTransforms(tmp, f"transforms_{split}.json", False)
            np.testing.assert_array_equal(R, R_fix)
            np.testing.assert_array_equal(T, T_fix)
            before += cams
        with contextlib.redirect_stdout(io.StringIO()) as log:
            info = dataset_readers.readSatelliteInfo(tmp, False, True)
        assert "Error converting" not in log.getvalue(), log.getvalue()
        after = list(info.train_cameras) + list(info.test_cameras)
        assert len(after) == len(before) == 5
        read_back, _, _ = dataset_readers.read_points3D_text(os.path.join(tmp, "points3D.txt"))
        np.testing.assert_array_equal(read_back, pts)             # repr() round-trips float64
        pcd = dataset_readers.fetchPly(os.path.join(tmp, "points3D.ply"))
        out["sat_points_normalised"] = np.asarray(pcd.points, dtype=np.float32)
    out.update(sat_points=pts, sat_R_fix=R_fix, sat_T_fix=T_fix,
               sat_cam_R_in=np.stack([c.R for c in before]), sat_cam_T_in=np.stack([c.T for c in before]),
               sat_cam_R_out=np.stack([c.R for c in after]), sat_cam_T_out=np.stack([c.T for c in after]))
    # lines 381-390 on the same points: the two numbers the reference prints
    xyz = np.matmul(pts, R_fix.T) - T_fix
    scale = 256 / np.percentile(np.linalg.norm(xyz, axis=1), 99)
    z_min = np.percentile((xyz * scale)[:, 2], 1)
    for line in log.getvalue().splitlines():                      # ... and what it printed agrees
        if line.startswith("Point cloud radius:"):
            assert abs(float(line.split("scale:")[1]) - scale) <= 1e-12 * scale, line
        if line.startswith("Point cloud z_min:"):
            assert abs(float(line.split(":")[1]) - z_min) <= 1e-12 * abs(z_min), line
    out.update(sat_scale=np.float64(scale), sat_z_min=np.float64(z_min))
    return out


def generate():
    dataset_readers, sh_utils = import_reference()
    out = sh_part(sh_utils)
    out.update(satellite_part(dataset_readers))
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert set(old.files) == set(out), set(old.files) ^ set(out)
        for k in out:
            np.testing.assert_array_equal(old[k], out[k], err_msg=k)
        print("reference_transform.npz reproduced exactly")
        return
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
