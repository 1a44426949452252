"""sfgs.consistency without a GPU: the restatement tests/consistency_np.py (what tests/test_gpu_consistency.py holds the kernel
to) reaches every branch of the pair test on the shared scene and does what it is for -- on blurred depth maps the filtered DSM
is ten times closer to the terrain --, the header, the library and the binding agree on the two new symbols and the two new
structs with the ABI version unchanged, the library refuses every bad argument before any GPU work, and the wrapper's argument
checks run before the library is loaded."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import consistency_np as cnp
import geometry_np as gnp
from sfgs import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sfgs_consistency_table_check", "sfgs_consistency_check")
E_ARG = -1


def header():
    return open(os.path.join(ROOT, "include", "sfgs.h")).read()


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_the_shared_scene_reaches_every_branch():
    _, _, views, _ = cnp.city(5, 48, 64)
    total, hist = dict.fromkeys(cnp.BRANCHES, 0), np.zeros(5, dtype=np.int64)
    for i in range(5):
        left = {}
        count, keep = cnp.check(views, i, 0.01, 1.0, 2, branches=left)
        assert count.dtype == keep.dtype == np.uint8 and count.shape == keep.shape == (48, 64)
        np.testing.assert_array_equal(keep, count >= 2)
        used = cnp.used_pixels(views[i].depth, None)
        assert not count[~used].any()
        hist += np.bincount(count[used], minlength=5)
        for name in cnp.BRANCHES:
            total[name] += left[name]
    assert all(total[name] >= 50 for name in cnp.BRANCHES), total
    assert sum(total.values()) == 4 * hist.sum()                              # every used pixel meets its four sources
    # the figures the scene was chosen with (a float64 prototype written apart from this restatement gave the same)
    assert total == {"behind_or_outside": 11353, "source_unused": 122, "depth_failed": 20583, "round_trip_failed": 1608,
                     "accepted": 21242}
    assert hist.tolist() == [2988, 4284, 3178, 2506, 771]


def test_project_inverts_unproject_and_check_agrees_with_a_per_pixel_loop():
    _, _, views, _ = cnp.city(3, 24, 32)
    k = cnp.constants(views[1].camera, 24, 32)
    row, col = np.mgrid[0:24, 0:32].reshape(2, -1)
    d = np.random.default_rng(1).uniform(80.0, 120.0, row.size).astype(np.float32)
    u, v, z = cnp.project(k, cnp.unproject_pixels(k, row, col, d))
    assert np.abs(u - col).max() < 1e-9 and np.abs(v - row).max() < 1e-9 and np.abs(z - d).max() < 1e-9
    # the pair test as scalar Python, pixel by pixel and source by source, in the order include/sfgs.h gives
    K = [cnp.constants(w.camera, 24, 32) for w in views]
    for i in range(3):
        want = np.zeros((24, 32), dtype=np.uint8)
        for r in range(24):
            for c in range(32):
                d = views[i].depth[r, c]
                if not (d > 0 and np.isfinite(d)):
                    continue
                w = cnp.unproject_pixels(K[i], np.array([r]), np.array([c]), np.array([d]))
                for j in range(3):
                    if j == i:
                        continue
                    u, v, z = (float(t[0]) for t in cnp.project(K[j], w))
                    if not z > 0:
                        continue
                    fu, fv = np.floor(u + 0.5), np.floor(v + 0.5)
                    if not (0 <= fu < 32 and 0 <= fv < 24):
                        continue
                    dj = views[j].depth[int(fv), int(fu)]
                    if not (dj > 0 and np.isfinite(dj)) or not abs(float(dj) - z) <= 0.01 * z:
                        continue
                    w2 = cnp.unproject_pixels(K[j], np.array([int(fv)]), np.array([int(fu)]), np.array([dj]))
                    u2, v2, z2 = (float(t[0]) for t in cnp.project(K[i], w2))
                    if z2 > 0 and (u2 - c) * (u2 - c) + (v2 - r) * (v2 - r) <= 1.0:
                        want[r, c] += 1
        count, keep = cnp.check(views, i, 0.01, 1.0, 1)
        np.testing.assert_array_equal(count, want)
        np.testing.assert_array_equal(keep, want >= 1)
        assert 0 < (want > 0).sum() < want.size


def test_blur3_is_the_edge_padded_box_mean_and_keeps_zeros():
    d = np.random.default_rng(2).uniform(1.0, 9.0, (5, 6)).astype(np.float32)
    d[2, 3] = 0.0
    b = cnp.blur3(d)
    assert b.dtype == np.float32 and b[2, 3] == 0.0
    for r, c in ((0, 0), (4, 5), (1, 2), (0, 3)):
        rows, cols = np.clip([r - 1, r, r + 1], 0, 4), np.clip([c - 1, c, c + 1], 0, 5)
        assert abs(float(b[r, c]) - d.astype(np.float64)[np.ix_(rows, cols)].mean()) < 1e-6
    np.testing.assert_array_equal(cnp.blur3(np.full((4, 4), 7.0, dtype=np.float32)), np.float32(7.0))


def test_filtered_dsm_of_blurred_depths_is_ten_times_closer_to_the_terrain():
    grid, terrain, views, origin = cnp.city(8, 96, 128, blurred=True)
    truth = terrain + origin[2]
    plain = cnp.dsm_of(views, grid, origin)
    filtered = cnp.dsm_of(views, grid, origin, cnp.masks(views, 0.01, 1.0, 2))
    mae_plain, mae_filtered = np.nanmean(np.abs(plain - truth)), np.nanmean(np.abs(filtered - truth))
    n_plain, n_filtered = int(np.isfinite(plain).sum()), int(np.isfinite(filtered).sum())
    print(f"MAE {mae_plain:.3f} m unfiltered, {mae_filtered:.3f} m filtered; cells {n_plain} -> {n_filtered} of {truth.size}")
    assert mae_filtered <= 0.1 * mae_plain                 # measured: 0.288 m against 8.06 m
    assert n_filtered >= 0.8 * n_plain and n_filtered >= 0.8 * truth.size      # measured: 3560 of 4087 filled, of 4096 cells


# ---- header, library, binding ---------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(tmp_path):
    hdr = header()
    lib = L.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfgs.h"
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    declared_version = int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1))
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() == 28         # symbols were added, nothing else moved
    for struct, name in ((L.SfgsConsistencyView, "SfgsConsistencyView"), (L.SfgsConsistencyArgs, "SfgsConsistencyArgs")):
        fields = [f for f, _ in struct._fields_]
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        declared = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                    for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
        assert declared == fields
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
    # the camera constants of a record are GeoCamera's without the origin, in the order the point cloud's view carries them
    pc = [f for f, _ in L.SfgsPointCloudViewArgs._fields_]
    assert [f for f, _ in L.SfgsConsistencyView._fields_][4:] == [f for f in pc[pc.index("M"):] if f != "origin"]


def test_every_bad_argument_is_refused_before_any_gpu_work():
    lib = L.load()
    dummy = C.c_double(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value        # never dereferenced: every call below is refused first

    def table(n=3, **kw):
        t = (L.SfgsConsistencyView * n)()
        for k in range(n):
            t[k] = L.SfgsConsistencyView(fp, None, 8, 8, (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_double * 3)(), 4.0, 4.0,
                                         10.0, 10.0)
        for name, v in kw.items():
            setattr(t[n - 1], name, v)
        return t

    def refused(rc, what):
        assert rc == E_ARG, what
        assert lib.sfgs_last_error(), what

    assert lib.sfgs_consistency_table_check(table(), 3) == 0
    assert lib.sfgs_consistency_table_check(table(256), 256) == 0
    assert lib.sfgs_consistency_table_check(table(2), 2) == 0
    for v in (1, 0, -1, 257):
        refused(lib.sfgs_consistency_table_check(table(), v), v)
    refused(lib.sfgs_consistency_table_check(None, 3), "NULL table")
    for bad in ({"H": 0}, {"W": -1}, {"H": 1 << 16, "W": 1 << 15}, {"depth": None}, {"focal_x": 0.0}, {"focal_y": 0.0}):
        refused(lib.sfgs_consistency_table_check(table(**bad), 3), bad)
    assert b"SfgsConsistencyView 2" in lib.sfgs_last_error()

    def args(**kw):
        a = L.SfgsConsistencyArgs(C.sizeof(L.SfgsConsistencyArgs), 3, 0, 8, 8, 2, fp, 0.01, 1.0)
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    for bad in ({"struct_size": 8}, {"struct_size": C.sizeof(L.SfgsConsistencyArgs) + 8}, {"V": 1}, {"V": 257}, {"ref": -1}, {"ref": 3},
                {"H": 0}, {"W": -2}, {"H": 1 << 16, "W": 1 << 15}, {"min_views": 0}, {"min_views": -1}, {"table": None},
                {"rel_tol": 0.0}, {"rel_tol": -0.01}, {"rel_tol": float("inf")}, {"rel_tol": float("nan")}, {"px_tol2": 0.0},
                {"px_tol2": -1.0}, {"px_tol2": float("nan")}):
        refused(lib.sfgs_consistency_check(C.byref(args(**bad)), fp, fp, None), bad)
    refused(lib.sfgs_consistency_check(None, fp, fp, None), "args")
    refused(lib.sfgs_consistency_check(C.byref(args()), None, fp, None), "count")
    refused(lib.sfgs_consistency_check(C.byref(args()), fp, None, None), "keep")
    with pytest.raises(RuntimeError, match="libsfgs error -1"):
        L.check(lib.sfgs_consistency_check(C.byref(args(ref=7)), fp, fp, None))


def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    from sfgs import consistency as cm
    from sfgs import geometry as geo
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    assert set(cm.__all__) >= {"ViewSet"} and not hasattr(cm, "install")
    cam = types.SimpleNamespace(R=np.eye(3), T=np.zeros(3), focal_x=100.0, focal_y=100.0)
    d = torch.ones(6, 8)
    # the set: V, lengths, dtype, shape, masks, cameras
    for depths, cams, masks in (([d], [cam], None), ([], [], None), ([d] * 257, [cam] * 257, None), ([d, d], [cam], None),
                                ([d, d], [cam, cam], [None]), ([d, d.double()], [cam, cam], None), ([d, torch.ones(2, 6, 8)], [cam, cam], None),
                                ([d, torch.ones(0, 8)], [cam, cam], None), ([d, np.ones((6, 8), np.float32)], [cam, cam], None),
                                ([np.ones((6, 8), np.float32), d], [cam, cam], None), (d, [cam, cam], 5),
                                ([d, d], [cam, cam], [None, torch.ones(6, 8)]), ([d, d], [cam, cam], [torch.ones(6, 7, dtype=torch.bool), None]),
                                ([d, d], [cam, types.SimpleNamespace(R=np.eye(3))], None),
                                ([d, d], [cam, types.SimpleNamespace(**{**vars(cam), "focal_x": 0.0})], None),
                                ([d, d], [cam, types.SimpleNamespace(**{**vars(cam), "R": np.eye(2)})], None),
                                ([d, d], [cam, types.SimpleNamespace(**{**vars(cam), "T": [0.0, np.nan, 0.0]})], None)):
        with pytest.raises(ValueError):
            cm.ViewSet(depths, cams, masks)
    with pytest.raises(ValueError, match="GPU"):           # everything else is right: the device check is the last one
        cm.ViewSet([d, torch.ones(3, 4)], [cam, cam], [None, torch.ones(3, 4, dtype=torch.uint8)])
    # check() and masks(): the checks need no device
    vs = object.__new__(cm.ViewSet)
    vs.sizes, vs.device = [(6, 8), (3, 4)], torch.device("cuda:0")
    assert len(vs) == 2
    for i in (-1, 2, 1.0, True, None, "0"):
        with pytest.raises(ValueError, match="i must"):
            vs.check(i)
    bad = ({"rel_tol": 0.0}, {"rel_tol": -0.01}, {"rel_tol": np.inf}, {"rel_tol": np.nan}, {"rel_tol": None}, {"px_tol": 0.0},
           {"px_tol": -1.0}, {"px_tol": np.nan}, {"px_tol": "wide"}, {"min_views": 0}, {"min_views": -3}, {"min_views": 1.0},
           {"min_views": True}, {"min_views": None})
    for kw in bad:
        with pytest.raises(ValueError, match=next(iter(kw))):
            vs.check(0, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            vs.masks(**kw)
    with pytest.raises(AssertionError, match="the library was loaded"):       # px_tol = inf is allowed: the checks pass
        vs.check(1, rel_tol=0.005, px_tol=np.inf, min_views=1)
    # evaluate_dsm(consistency=)
    grid = geo.DsmGrid(0.0, 8.0, 8, 8, 1.0)
    ok = {"rel_tol": 0.01, "px_tol": 1.0, "min_views": 2}
    for c in ((0.01, 1.0, 2), {"rel_tol": 0.01, "px_tol": 1.0}, {**ok, "radius": 1}, {**ok, "rel_tol": 0.0}, {**ok, "px_tol": np.nan},
              {**ok, "min_views": 0}):
        with pytest.raises(ValueError, match="consistency|rel_tol|px_tol|min_views"):
            geo.evaluate_dsm([d, d], [cam, cam], grid, torch.ones(8, 8), consistency=c)
    with pytest.raises(ValueError, match="GPU"):           # a good dict goes on to the checks evaluate_dsm always made
        geo.evaluate_dsm([d, d], [cam, cam], grid, torch.ones(8, 8), consistency=ok)
