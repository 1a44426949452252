"""sfgs.pointcloud without a GPU: the C header, the library and the ctypes binding agree on ABI 27 and on the layout of
SfgsPointCloudViewArgs; the three entry points refuse every bad argument with -1 and a message before any GPU work; the
wrapper's argument checks run before the library is loaded; the PLY table builder on numpy arrays, through sfgs.ply and back.
The kernels: tests/test_gpu_pointcloud.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from sfgs import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sfgs_pointcloud_scratch_bytes", "sfgs_pointcloud_append", "sfgs_pointcloud_bounds")


def test_header_library_and_binding_agree(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfgs.h"
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    declared_version = int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1))
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() and L.ABI_VERSION >= 27
    struct, name = L.SfgsPointCloudViewArgs, "SfgsPointCloudViewArgs"
    fields = [f for f, _ in struct._fields_]
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    declared = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields
    # the camera and origin fields of SfgsDsmViewArgs, in its order, and `image`
    dsm = [f for f, _ in L.SfgsDsmViewArgs._fields_]
    assert [f for f in fields if f != "image"] == dsm[:dsm.index("focal_y") + 1]
    src = tmp_path / f"{name}.c"
    prints = "\n".join(f'  printf("{f} %zu\\n", offsetof({name}, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                   f'  printf("sizeof %zu\\n", sizeof({name}));\n{prints}\n  return 0;\n}}\n')
    exe = tmp_path / name
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == C.sizeof(struct)
    for f in fields:
        assert int(out[f]) == getattr(struct, f).offset, f


def test_every_bad_argument_is_refused_with_minus_one_and_a_message():
    lib = L.load()
    dummy = C.c_double(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value        # never dereferenced: every call below is refused first

    def view(**kw):
        a = L.SfgsPointCloudViewArgs(C.sizeof(L.SfgsPointCloudViewArgs), 1024, 1024, fp, None, None,
                                     (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_double * 3)(), (C.c_double * 3)(), 512.0, 512.0,
                                     2000.0, 2000.0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(rc, what):
        assert rc == -1, what
        assert lib.sfgs_last_error(), what

    need = lib.sfgs_pointcloud_scratch_bytes(1024, 1024)
    assert 1024 * 1024 // 256 * 8 <= need <= 1 << 20       # one word per 256-pixel workgroup, and the bounds' partials
    assert lib.sfgs_pointcloud_scratch_bytes(1, 1) >= 6 * 8  # any valid size covers sfgs_pointcloud_bounds
    for H, W in ((0, 4), (4, 0), (-1, 4), (32768, 32769), (1 << 30, 2)):
        assert lib.sfgs_pointcloud_scratch_bytes(H, W) == 0 and lib.sfgs_last_error(), (H, W)
        refused(lib.sfgs_pointcloud_append(C.byref(view(H=H, W=W)), fp, None, 10, fp, fp, 1 << 40, None), (H, W))
    assert lib.sfgs_pointcloud_scratch_bytes(32768, 32768) > 0
    cap = 1024 * 1024
    for bad in ({"struct_size": 8}, {"struct_size": C.sizeof(L.SfgsPointCloudViewArgs) + 8}, {"depth": None}, {"focal_x": 0.0},
                {"focal_y": 0.0}, {"image": fp}):           # an image without a colour buffer
        refused(lib.sfgs_pointcloud_append(C.byref(view(**bad)), fp, None, cap, fp, fp, need, None), bad)
    refused(lib.sfgs_pointcloud_append(None, fp, None, cap, fp, fp, need, None), "args")
    refused(lib.sfgs_pointcloud_append(C.byref(view()), None, None, cap, fp, fp, need, None), "points")
    refused(lib.sfgs_pointcloud_append(C.byref(view()), fp, fp, cap, fp, fp, need, None), "colors without an image")
    refused(lib.sfgs_pointcloud_append(C.byref(view()), fp, None, cap, None, fp, need, None), "state")
    refused(lib.sfgs_pointcloud_append(C.byref(view()), fp, None, cap, fp, None, need, None), "scratch")
    refused(lib.sfgs_pointcloud_append(C.byref(view()), fp, None, -1, fp, fp, need, None), "capacity")
    refused(lib.sfgs_pointcloud_append(C.byref(view()), fp, None, cap, fp, fp, need - 1, None), "scratch_bytes")
    assert b"scratch" in lib.sfgs_last_error()
    small = lib.sfgs_pointcloud_scratch_bytes(1, 1)
    out6 = (C.c_double * 6)()
    refused(lib.sfgs_pointcloud_bounds(None, fp, cap, out6, fp, small, None), "points")
    refused(lib.sfgs_pointcloud_bounds(fp, None, cap, out6, fp, small, None), "state")
    refused(lib.sfgs_pointcloud_bounds(fp, fp, cap, None, fp, small, None), "out6")
    refused(lib.sfgs_pointcloud_bounds(fp, fp, cap, out6, None, small, None), "scratch")
    refused(lib.sfgs_pointcloud_bounds(fp, fp, -1, out6, fp, small, None), "capacity")
    refused(lib.sfgs_pointcloud_bounds(fp, fp, cap, out6, fp, small - 1, None), "scratch_bytes")
    with pytest.raises(RuntimeError, match="libsfgs error -1"):
        L.check(lib.sfgs_pointcloud_bounds(fp, fp, -1, out6, fp, small, None))


def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    from sfgs import pointcloud as pcm
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    assert set(pcm.__all__) >= {"PointCloud", "depth_to_points"}
    for kw in ({"capacity": 0}, {"capacity": -4}, {"capacity": 2.5}, {"capacity": True}, {"capacity": 8, "device": "cpu"}):
        with pytest.raises(ValueError):
            pcm.PointCloud(**kw)
    cam = dict(R=np.eye(3), T=np.zeros(3), focal_x=100.0, focal_y=100.0)
    d = torch.ones(6, 8)
    for colors in (False, True):
        pc = object.__new__(pcm.PointCloud)               # the checks of add_depth need no device
        pc.capacity, pc.device, pc._colors = 48, torch.device("cuda:0"), (torch.empty(48, 3, dtype=torch.uint8) if colors else None)
        img = {"image": torch.ones(3, 6, 8)} if colors else {}
        for bad in (np.ones((6, 8), np.float32), d.double(), torch.ones(2, 6, 8), torch.ones(0, 8)):
            with pytest.raises(ValueError):
                pc.add_depth(bad, **cam, **img)
        for kw in ({"mask": torch.ones(6, 8)}, {"mask": torch.ones(6, 7, dtype=torch.bool)}, {"origin": [1.0, 2.0]},
                   {"origin": [1.0, 2.0, np.nan]}, {"focal_x": 0.0}, {"R": np.eye(2)}, {"T": [0.0, 1.0]},
                   {"image": None if colors else torch.ones(3, 6, 8)}, {"image": torch.ones(3, 6, 7)} if colors else {"mask": 3},
                   {"image": torch.ones(3, 6, 8).double()} if colors else {"mask": 3}):
            with pytest.raises(ValueError):
                pc.add_depth(d, **{**cam, **img, **kw})
        with pytest.raises(ValueError, match="GPU"):
            pc.add_depth(d, **cam, **img)
    with pytest.raises(ValueError, match="GPU"):
        pcm.depth_to_points(d, type("Cam", (), cam))
    from sfgs import geometry as geo
    with pytest.raises(ValueError, match="PointCloud"):
        geo.evaluate_dsm([d], [cam], geo.DsmGrid(0.0, 8.0, 8, 8, 1.0), torch.ones(8, 8), cloud=object())


def test_ply_table_on_numpy_arrays_and_through_the_file(tmp_path):
    from sfgs.ply import read_ply, write_ply
    from sfgs.pointcloud import ply_table
    rng = np.random.default_rng(3)
    pts = rng.normal(0, 1, (11, 3)) * 1e3 + np.array([4.0e5, 3.3e6, 20.0])
    pts[4, 2] = np.pi * 1e-300                             # a value float32 cannot hold: the columns must be double
    col = rng.integers(0, 256, (11, 3), dtype=np.uint8)
    plain, coloured = ply_table(pts), ply_table(pts, col)
    assert plain.dtype.names == ("x", "y", "z") and coloured.dtype.names == ("x", "y", "z", "red", "green", "blue")
    assert all(plain.dtype[n] == np.float64 for n in "xyz") and all(coloured.dtype[n] == np.uint8 for n in ("red", "green", "blue"))
    assert plain.itemsize == 24 and coloured.itemsize == 27
    for table, want_col in ((plain, None), (coloured, col)):
        path = tmp_path / "cloud.ply"
        write_ply(str(path), table)
        head = path.read_bytes().split(b"end_header\n")[0].decode().splitlines()
        assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 11"]
        assert head[3:6] == ["property double x", "property double y", "property double z"]
        assert head[6:] == ([] if want_col is None else ["property uchar red", "property uchar green", "property uchar blue"])
        (name, back), = read_ply(str(path))
        assert name == "vertex" and len(back) == 11
        np.testing.assert_array_equal(np.stack([back[n] for n in "xyz"], axis=1).view(np.uint64), pts.view(np.uint64))
        if want_col is not None:
            np.testing.assert_array_equal(np.stack([back[n] for n in ("red", "green", "blue")], axis=1), want_col)
    assert len(ply_table(np.zeros((0, 3)))) == 0
    for bad in (pts.astype(np.float32), pts[:, :2], pts.reshape(-1)):
        with pytest.raises(ValueError):
            ply_table(bad)
    for bad in (col[:5], col.astype(np.int32), col[:, :2]):
        with pytest.raises(ValueError):
            ply_table(pts, bad)
