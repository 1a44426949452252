"""TsdfVolume.raycast without a GPU: the host build of the product's csrc/tsdf_math.h (tests/host_check/tsdf_raycast_check.cpp),
with the uniform and with the skipping march, equals the numpy restatement tests/tsdf_raycast_np.py -- which has the uniform
march only -- byte for byte on the shared scenes and on a scene per branch; the restatement finds the analytic sphere and gives
the fused depth maps back; the empty-space table equals the numpy table; header, library and binding agree on the new symbols
with the ABI version unchanged; library and wrapper refuse bad arguments before any GPU work.

Every count below was taken from the restatement (hits, samples, branch codes) or from the host build (jumps) and is asserted
exactly: the scenes are seeded, the arithmetic is IEEE float64."""
import ctypes as C
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import consistency_np as cnp
import tsdf_np as tnp
import tsdf_raycast_hostcheck as rhc
import tsdf_raycast_np as rnp
from sfgs import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sfgs_tsdf_skip_bytes", "sfgs_tsdf_skip_build", "sfgs_tsdf_raycast")
E_ARG = -1
WAVY, wavy, volume_of, branch_scenes, BRANCH_SCENES = rnp.WAVY, rnp.wavy, rnp.volume_of, rnp.branch_scenes, rnp.BRANCH_SCENES


def same_bytes(got, ref, what):
    for name in ("depth", "normal", "rgb"):
        g, r = getattr(got, name), getattr(ref, name)
        assert (g is None) == (r is None), f"{name}, {what}"
        if r is not None:
            assert g.shape == r.shape and g.dtype == r.dtype == np.float32, f"{name}, {what}"
            np.testing.assert_array_equal(g.view(np.uint32), r.view(np.uint32), err_msg=f"{name}, {what}")


def both_marches(case, cam, H, W, what, **kw):
    """The restatement, and the host build with either march held to it -> (restatement, uniform, skipping)"""
    ref = rnp.raycast(*case, cam, H, W, **kw)
    uniform = rhc.raycast(*case, cam, H, W, skip=False, **kw)
    skipping = rhc.raycast(*case, cam, H, W, skip=True, **kw)
    same_bytes(uniform, ref, f"{what}, uniform march")
    same_bytes(skipping, ref, f"{what}, skipping march")
    assert uniform.samples == ref.samples and uniform.jumps == 0, what   # the two uniform marches evaluate the same samples
    assert skipping.samples <= uniform.samples, what
    miss = ref.depth[0] == 0
    assert int((~miss).sum()) == ref.hits == rnp.count(ref.code, "hit"), what
    for a in (ref.normal, ref.rgb):
        if a is not None:
            assert not a[:, miss].any(), what                             # zeros where depth is 0
    print(what, "hits", ref.hits, "of", H * W, "samples", ref.samples, "skipping", skipping.samples, skipping.jumps, skipping.longest,
          skipping.longest_run, {n: rnp.count(ref.code, n) for n in rnp.BRANCHES})
    return ref, uniform, skipping


# ---- host build == restatement ---------------------------------------------------------------------------------------------------
def test_sphere_with_colours_equals_the_restatement():
    ref, _, _ = both_marches(tnp.sphere_volume(colors=True), rnp.sphere_camera(), 20, 24, "sphere")
    assert ref.hits == 74 and rnp.count(ref.code, "missed_box") == 135 and rnp.count(ref.code, "ran_out") == 271    # 15 % hit
    assert np.ptp(ref.rgb[:, ref.depth[0] > 0]) > 0.5
    norm = np.linalg.norm(ref.normal[:, ref.depth[0] > 0].astype(np.float64), axis=0)
    assert np.abs(norm - 1).max() < 1e-6                                    # float32 of a unit vector


@pytest.mark.parametrize("view, hits, samples, skipped_to", ((0, 840, 25452, 10399), (2, 617, 14404, 8040), (3, 1920, 3840, 3840)))
def test_fused_volume_equals_the_restatement(view, hits, samples, skipped_to):
    vol, views, _, state = rnp.fused_volume()
    H, W = views[view].depth.shape
    ref, _, skipping = both_marches(volume_of(state, vol), views[view].camera, H, W, f"fusion scene from camera {view}")
    assert (ref.hits, ref.samples, skipping.samples) == (hits, samples, skipped_to)
    if view == 3:                                                             # inside the box, everything within two samples
        assert rnp.count(ref.code, "starts_at_near") == H * W == ref.hits
    else:                                                                     # 44 % and 58 % hit
        assert 0.1 * H * W < ref.hits < 0.9 * H * W and skipping.jumps > 1000


def test_wavy_volume_from_above_takes_runs_over_several_bricks():
    ref, uniform, skipping = both_marches(wavy(), rnp.wavy_top_camera(WAVY), 40, 48, "wavy from above")
    assert (ref.hits, uniform.samples) == (896, 38828)                        # 47 % hit
    assert (skipping.samples, skipping.jumps, skipping.longest, skipping.longest_run) == (22205, 2391, 7, 40)
    assert skipping.samples < uniform.samples
    # A jump stays in one brick of 8 cells, and from above a lattice step of one voxel crosses about a cell: 7 is as long as a
    # jump gets here. The run of samples not evaluated goes on through brick after brick: 40 lattice steps, five bricks.
    assert skipping.longest_run >= 9
    # with 0.37 voxels per step a single jump inside one brick is that long too
    fine = rhc.raycast(*wavy(), rnp.wavy_top_camera(WAVY), 40, 48, step=0.37 * 0.25, skip=True)
    assert (fine.longest, fine.longest_run) == (21, 106) and fine.longest >= 9


@pytest.mark.parametrize("dims", ((2, 9, 10), (10, 2, 17), (18, 11, 2), (24, 20, 16), (9, 9, 9), (26, 17, 10)))
def test_skip_table_equals_the_numpy_table(dims):
    nx, ny, nz = dims
    rng = np.random.default_rng(nx * 10000 + ny * 100 + nz)
    tsdf = np.where(rng.random((nz, ny, nx)) < 0.01, -0.5, 0.5).astype(np.float32)      # a few inside voxels: bricks of both kinds
    weight = (rng.random((nz, ny, nx)) < 0.7).astype(np.float32)
    want = rnp.skip_table(tsdf, weight)
    assert want.shape == tuple(1 if n < 2 else (n + 6) // 8 for n in (nz, ny, nx))
    assert 0 < int(want.sum()) and (want.sum() < want.size or want.size <= 2)
    np.testing.assert_array_equal(rhc.skip_table(tsdf, weight), want)
    # the footprint reaches one voxel into the next brick and no further: a single inside voxel at index 8 sets bricks 0 and 1
    if nx > 17:
        one = np.full((nz, ny, nx), 0.5, np.float32)
        one[0, 0, 8] = -0.5
        want = rnp.skip_table(one, np.ones_like(one))
        assert want[0, 0, :3].tolist() == [1, 1, 0] and want.sum() == 2
        np.testing.assert_array_equal(rhc.skip_table(one, np.ones_like(one)), want)
        np.testing.assert_array_equal(rhc.skip_table(one, np.zeros_like(one)), np.zeros_like(want))       # unobserved: no flag


def test_fused_and_wavy_tables_equal_the_numpy_tables():
    vol, _, _, state = rnp.fused_volume()
    want = rnp.skip_table(state.tsdf, state.weight)
    assert want.shape == (2, 3, 3) and 0 < want.sum() < want.size             # 15 x 19 x 23 cells: partial bricks on every axis
    np.testing.assert_array_equal(rhc.skip_table(state.tsdf, state.weight), want)
    tsdf, weight = wavy()[:2]
    want = rnp.skip_table(tsdf, weight)
    assert want.shape == (8, 8, 9) and 0 < want.sum() < want.size
    np.testing.assert_array_equal(rhc.skip_table(tsdf, weight), want)


# ---- what the restatement computes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step, max_deviation, min_dot", ((1.0, 0.0716, 0.99244), (0.5, 0.0593, 0.99355)))
def test_restatement_finds_the_analytic_sphere(step, max_deviation, min_dot):
    """Measured on the restatement: the hit points lie within 0.0716 voxels of the sphere's radius at step 1.0 and 0.0593 at 0.5
    (a trilinear surface of a distance field clipped at +-2 voxels), the normals' dot product with the radial direction is at
    least 0.99244 and 0.99355. Asserted with a margin of 2x on the deviation (from 0 and from 1)."""
    cam, (H, W) = rnp.sphere_camera(), (20, 24)
    r = rnp.raycast(*tnp.sphere_volume(), cam, H, W, step=step)
    row, col = np.nonzero(r.depth[0] > 0)
    assert len(row) == 74
    points = cnp.unproject_pixels(cnp.constants(cam, H, W), row, col, r.depth[0][row, col])
    radial = points - np.array(tnp.SPHERE.centre)
    dist = np.linalg.norm(radial, axis=1)
    deviation = np.abs(dist - tnp.SPHERE.radius).max()
    dots = ((r.normal[:, row, col].T.astype(np.float64) * radial).sum(axis=1) / dist).min()
    print("step", step, "max |r - R|", deviation, "min dot", dots)
    assert deviation < 2 * max_deviation and 1 - dots < 2 * (1 - min_dot)
    assert abs(deviation - max_deviation) < 1e-4 and abs(dots - min_dot) < 1e-5        # and the figures above are these


@pytest.mark.parametrize("view, median, maximum", ((3, 0.0719, 0.1486), (0, 0.0223, None)))
def test_round_trip_on_the_fusion_scene(view, median, maximum):
    """|ray-cast depth - input depth| over the pixels used in the input that the ray-cast hit, from two fused cameras, voxel 0.5,
    measured on the restatement: camera 3 median 0.0719, maximum 0.1486 over 1852 pixels; camera 0 median 0.0223 over 811
    (its maximum, 3.96, is a silhouette of the sphere: a depth edge, not bounded). Asserted with a margin of 2x."""
    vol, views, _, state = rnp.fused_volume()
    v = views[view]
    r = rnp.raycast(*volume_of(state, vol), v.camera, *v.depth.shape)
    both = cnp.used_pixels(v.depth, v.mask) & (r.depth[0] > 0)
    err = np.abs(r.depth[0][both].astype(np.float64) - v.depth[both])
    print("camera", view, "pixels", int(both.sum()), "median", np.median(err), "max", err.max())
    assert int(both.sum()) == (1852 if view == 3 else 811)
    assert np.median(err) < 2 * median and abs(np.median(err) - median) < 1e-4
    if maximum is not None:
        assert err.max() < 2 * maximum and abs(err.max() - maximum) < 1e-4


# ---- branches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BRANCH_SCENES)
def test_branch(name):
    case, cam, H, W, kw, counts = branch_scenes()[name]
    ref, _, _ = both_marches(case, cam, H, W, name, **kw)
    got = {n: rnp.count(ref.code, n) for n in counts}
    assert got == counts, name
    assert any(v > 0 for n, v in counts.items() if n != "hit"), name          # the branch the scene is there for was taken


def test_normals_false_leaves_depth_and_rgb_unchanged():
    vol, views, _, state = rnp.fused_volume()
    case = volume_of(state, vol)
    full = rnp.raycast(*case, views[0].camera, 40, 48)
    for skip in (False, True):
        bare = rhc.raycast(*case, views[0].camera, 40, 48, normals=False, skip=skip)
        assert bare.normal is None and bare.depth.tobytes() == full.depth.tobytes() and bare.rgb.tobytes() == full.rgb.tobytes()
    plain = rhc.raycast(case[0], case[1], None, case[3], case[4], views[0].camera, 40, 48, normals=False, skip=True)
    assert plain.rgb is None and plain.normal is None and plain.depth.tobytes() == full.depth.tobytes()


# ---- header, library, binding ------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfgs.h"
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    declared_version = int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1))
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() == 28         # symbols were added, nothing else moved
    fields = [f for f, _ in L.SfgsTsdfRay._fields_]
    assert fields == ["struct_size", "H", "W", "M", "c", "cx_pix", "cy_pix", "focal_x", "focal_y", "near", "far", "step", "depth",
                      "normal", "rgb"]
    body = re.search(r"typedef struct SfgsTsdfRay \{(.*?)\} SfgsTsdfRay;", hdr, re.S).group(1)
    declared = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields
    src = tmp_path / "ray.c"
    prints = "\n".join(f'  printf("{f} %zu\\n", offsetof(SfgsTsdfRay, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                   f'  printf("sizeof %zu\\n", sizeof(SfgsTsdfRay));\n{prints}\n  return 0;\n}}\n')
    exe = tmp_path / "ray"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SfgsTsdfRay)
    for f in fields:
        assert int(out[f]) == getattr(L.SfgsTsdfRay, f).offset, f
    for word in ("lerp(a, b, f) = a + f * (b - a)", "K = floor((z1 - z0) / step) + 1", "w = vp / (vp - vc)", "8 x 8 x 8 cells"):
        assert word in hdr                                                    # the sequence is stated in words


def test_the_library_refuses_bad_arguments_before_any_gpu_work():
    lib = L.load()
    dummy = C.c_double(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value        # never dereferenced: every call below is refused first

    def refused(rc, what):
        assert rc == E_ARG, what
        assert lib.sfgs_last_error(), what

    def volume(**kw):
        v = L.SfgsTsdfVolume(C.sizeof(L.SfgsTsdfVolume), 8, 8, 8, (C.c_double * 3)(), 0.5, 1.5, 64.0, fp, fp, None)
        for name, val in kw.items():
            setattr(v, name, val)
        return v

    def ray(**kw):
        r = L.SfgsTsdfRay(C.sizeof(L.SfgsTsdfRay), 6, 8, (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_double * 3)(), 4.0, 3.0, 10.0, 10.0,
                          0.0, math.inf, 0.5, fp, fp, None)
        for name, val in kw.items():
            setattr(r, name, val)
        return r

    def cast(v, r, skip=None, nbytes=0):
        return lib.sfgs_tsdf_raycast(None if v is None else C.byref(v), None if r is None else C.byref(r), skip, nbytes, None)

    assert lib.sfgs_tsdf_skip_bytes(8, 8, 8) == 1 and lib.sfgs_tsdf_skip_bytes(9, 10, 18) == 1 * 2 * 3
    assert lib.sfgs_tsdf_skip_bytes(1, 10, 11) == 1 * 2 * 2 and lib.sfgs_tsdf_skip_bytes(2, 2, 2) == 1
    assert lib.sfgs_tsdf_skip_bytes(0, 8, 8) == 0 and lib.sfgs_last_error()
    assert lib.sfgs_tsdf_skip_bytes(1 << 11, 1 << 10, (1 << 9) + 1) == 0
    refused(lib.sfgs_tsdf_skip_build(None, fp, 1, None), "NULL volume")
    refused(lib.sfgs_tsdf_skip_build(C.byref(volume()), None, 1, None), "NULL table")
    refused(lib.sfgs_tsdf_skip_build(C.byref(volume(nx=17)), fp, 1, None), "a table too small")
    refused(lib.sfgs_tsdf_skip_build(C.byref(volume(voxel_size=0.0)), fp, 1, None), "a bad volume")
    refused(lib.sfgs_tsdf_skip_build(C.byref(volume(struct_size=8)), fp, 1, None), "a bad volume size")
    refused(cast(None, ray()), "NULL volume")
    refused(cast(volume(), None), "NULL ray")
    refused(cast(volume(tsdf=None), ray()), "a volume without storage")
    for bad in ({"struct_size": 16}, {"H": 0}, {"W": -3}, {"H": 1 << 16, "W": 1 << 15}, {"step": 0.0}, {"step": -0.5}, {"step": math.nan},
                {"step": math.inf}, {"step": 1e-6}, {"near": -0.1}, {"near": math.nan}, {"near": math.inf}, {"far": 0.0}, {"near": 2.0, "far": 2.0},
                {"far": math.nan}, {"focal_x": 0.0}, {"focal_y": math.nan}, {"cx_pix": math.inf}, {"depth": None}, {"rgb": fp}):
        refused(cast(volume(), ray(**bad)), bad)
    bad_M = ray()
    bad_M.M[4] = math.nan
    refused(cast(volume(), bad_M), "NaN in M")
    refused(cast(volume(rgb=fp), ray()), "a volume with colours, a ray without")
    refused(cast(volume(nx=17), ray(), fp, 1), "a table too small")
    assert b"skip table" in lib.sfgs_last_error()
    # the smallest step the 8^3 volume takes: its diagonal 7 * 0.5 * sqrt(3) over 2^20
    refused(cast(volume(), ray(step=7 * 0.5 * math.sqrt(3) / (1 << 20) * 0.999)), "just too small a step")


def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    from sfgs import tsdf as tm
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    assert set(tm.__all__) >= {"RayView", "RaySkip"}
    cam = types.SimpleNamespace(R=np.eye(3), T=np.zeros(3), focal_x=100.0, focal_y=100.0)

    def volume(colors):                                  # a volume that was never given device memory: no check needs any
        v = object.__new__(tm.TsdfVolume)
        v.dims, v.device, v.voxel_size, v._rgb = (8, 8, 8), torch.device("cuda:0"), 0.5, (torch.zeros(3, 8, 8, 8) if colors else None)
        return v

    plain, coloured = volume(False), volume(True)

    def view(H=6, W=8, normals=True, colors=False):
        return tm.RayView(torch.zeros(1, H, W), torch.zeros(3, H, W) if normals else None, torch.zeros(3, H, W) if colors else None)

    ok = dict(camera=cam, height=6, width=8, out=view())
    for bad in ({"height": 0}, {"width": -1}, {"height": 6.0}, {"width": True}, {"height": None}, {"height": 1 << 16, "width": 1 << 15},
                {"step": 0.0}, {"step": -1.0}, {"step": math.nan}, {"step": math.inf}, {"step": "x"}, {"step": 1e-6},
                {"near": -0.5}, {"near": math.nan}, {"near": math.inf}, {"far": 0.0}, {"far": math.nan}, {"near": 3.0, "far": 3.0},
                {"near": 3.0, "far": 2.0}, {"skip": True}, {"skip": torch.zeros(1, 1, 1, dtype=torch.uint8)},
                {"skip": tm.RaySkip(torch.zeros(1, 1, 2, dtype=torch.uint8), (9, 8, 8))}, {"normals": 1}, {"out": torch.zeros(1, 6, 8)},
                {"out": view(H=7)}, {"out": view(normals=False)}, {"out": view(colors=True)}, {"normals": False},
                {"camera": types.SimpleNamespace(R=np.eye(3))}, {"camera": types.SimpleNamespace(**{**vars(cam), "focal_y": 0.0})},
                {"camera": types.SimpleNamespace(**{**vars(cam), "T": np.zeros(2)})}):
        with pytest.raises(ValueError):
            plain.raycast(**{**ok, **bad})
    with pytest.raises(ValueError):
        coloured.raycast(**ok)                                                # out has no rgb
    # a table on another device than the volume's, and outputs that are not on a GPU: the device checks come last
    with pytest.raises(ValueError, match="device"):
        plain.raycast(**{**ok, "skip": tm.RaySkip(torch.zeros(1, 1, 1, dtype=torch.uint8), (8, 8, 8))})
    with pytest.raises(ValueError, match="GPU"):
        plain.raycast(**ok)
    with pytest.raises(ValueError, match="GPU"):
        coloured.raycast(**{**ok, "out": view(colors=True), "skip": False, "far": 50.0, "near": 1.0, "step": 0.1})
