"""sfgs.transform without a GPU: the SH rotation matrices (group properties, and the convention pinned to the reference's
eval_sh through tests/golden/reference_transform.npz), the Similarity algebra, the satellite frame of readSatelliteInfo
against the reference's own output, render invariance of the float64 restatement (tests/transform_np.py, what the kernel is
held to) through the C oracle, the argument checks, and the agreement of header, library and ctypes binding.
The kernel itself: tests/test_gpu_transform.py."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import parity
import transform_np as tnp
from oracle import oracle as orc
from sfgs import _lib as L
from sfgs import transform as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "reference_transform.npz"))


def random_rotation(seed):
    return tnp.quat_to_matrix(np.random.default_rng(seed).normal(size=4))


# ---- sh_rotation ---------------------------------------------------------------------------------------------------------------
def test_sh_rotation_of_the_identity_is_the_identity():
    for l, D in enumerate(T.sh_rotation(np.eye(3)), start=1):
        assert D.shape == (2 * l + 1, 2 * l + 1) and D.dtype == np.float64
        np.testing.assert_allclose(D, np.eye(2 * l + 1), rtol=0, atol=1e-12)
        # ... and exactly so in the float32 the kernel receives: the identity similarity changes no bit
        np.testing.assert_array_equal(D.astype(np.float32), np.eye(2 * l + 1, dtype=np.float32))
    assert T.sh_rotation(np.eye(3), 0) == [] and len(T.sh_rotation(np.eye(3), 2)) == 2
    with pytest.raises(ValueError):
        T.sh_rotation(np.eye(3), 4)


@pytest.mark.parametrize("seeds", [(1, 2), (3, 4), (5, 6)])
def test_sh_rotation_is_orthogonal_and_a_homomorphism(seeds):
    R1, R2 = random_rotation(seeds[0]), random_rotation(seeds[1])
    for D1, D2, D12 in zip(T.sh_rotation(R1), T.sh_rotation(R2), T.sh_rotation(R1 @ R2)):
        np.testing.assert_allclose(D1 @ D1.T, np.eye(len(D1)), rtol=0, atol=1e-12)
        np.testing.assert_allclose(D1 @ D2, D12, rtol=0, atol=1e-12)


def test_sh_rotation_is_block_diagonal():
    """Fitting all 15 basis functions at once finds no coupling between bands, and the same blocks."""
    R = random_rotation(7)
    d = T._fit_directions(96)
    full = np.linalg.lstsq(T.sh_basis(d), T.sh_basis(d @ R.T), rcond=None)[0].T
    blocks = np.zeros((15, 15))
    for (a, b), D in zip(tnp.BANDS, T.sh_rotation(R)):
        blocks[a:b, a:b] = D
    np.testing.assert_allclose(full, blocks, rtol=0, atol=1e-12)
    assert np.abs(full[blocks == 0]).max() <= 1e-12


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_convention_is_the_reference_eval_sh(deg):
    """The invariant that defines D, with the reference on one side: the oracle's colour of the ROTATED coefficients at R d is
    the reference's eval_sh of the original coefficients at d (+ 0.5, clamped at 0, as the rasterizer's colour is: the fixture's
    colours stay above -0.5, so the clamp is idle). 1e-6 absolute: float32 evaluation of <= 16 terms of magnitude <= 1."""
    R = random_rotation(11)
    K = (deg + 1) ** 2
    dirs, sh = G["sh_dirs"], G["sh_coeffs"].astype(np.float64)            # [64,3], [P,3,16]
    want = G[f"sh_colour_deg{deg}"]
    assert want.min() > -0.5
    want = np.broadcast_to(want, (sh.shape[0], len(dirs), 3)).astype(np.float32) + np.float32(0.5)
    rotated = sh.copy()
    rotated[:, :, 1:] = tnp.features_rest(tnp.constants(T.Similarity(R)), sh[:, :, 1:], "n3k")[0]
    turned = dirs @ R.T
    for p in range(sh.shape[0]):
        km3 = np.repeat(rotated[p, :, :K].T[None], len(dirs), 0)          # [64,K,3]
        got = orc.sh_rgb(deg, km3, turned)
        np.testing.assert_allclose(got, want[p], rtol=0, atol=1e-6)
        if deg > 0:                                                       # ... and the test can fail: unrotated coefficients do not
            plain = orc.sh_rgb(deg, np.repeat(sh[p, :, :K].T[None], len(dirs), 0), turned)
            assert np.abs(plain - want[p]).max() > 1e-3


# ---- Similarity ----------------------------------------------------------------------------------------------------------------
def test_similarity_algebra():
    a = T.Similarity(random_rotation(1), 0.37, (100.0, -50.0, 20.0))
    b = T.Similarity(random_rotation(2), 2.5, (-3.0, 7.0, 0.25))
    np.testing.assert_allclose(a.inverse().compose(a).matrix(), np.eye(4), rtol=0, atol=1e-12)
    np.testing.assert_allclose(a.compose(a.inverse()).matrix(), np.eye(4), rtol=0, atol=1e-12)
    np.testing.assert_allclose(a.compose(b).matrix(), a.matrix() @ b.matrix(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(b.compose(a).matrix(), b.matrix() @ a.matrix(), rtol=0, atol=1e-12)
    back = T.Similarity.from_matrix(a.matrix())
    np.testing.assert_allclose(back.R, a.R, rtol=0, atol=1e-12)
    assert abs(back.s - a.s) <= 1e-12 and np.abs(back.t - a.t).max() <= 1e-12
    np.testing.assert_array_equal(T.Similarity.identity().matrix(), np.eye(4))
    x = np.random.default_rng(0).normal(size=(5, 3))
    np.testing.assert_allclose(a.apply(x), (np.c_[x, np.ones(5)] @ a.matrix().T)[:, :3], rtol=0, atol=1e-12)
    q = T.rotation_quaternion(a.R)
    assert q[0] >= 0 and abs(np.linalg.norm(q) - 1) <= 1e-15
    np.testing.assert_allclose(tnp.quat_to_matrix(q), a.R, rtol=0, atol=1e-14)
    for seed in range(8):                                                # every pivot of the quaternion extraction
        R = random_rotation(100 + seed)
        np.testing.assert_allclose(tnp.quat_to_matrix(T.rotation_quaternion(R)), R, rtol=0, atol=1e-14)
    half_turn = np.diag([-1.0, -1.0, 1.0])
    np.testing.assert_allclose(tnp.quat_to_matrix(T.rotation_quaternion(half_turn)), half_turn, rtol=0, atol=1e-14)


def test_improper_similarities_raise():
    R = random_rotation(1)
    for bad in (dict(R=R * 1.0001), dict(R=R + 1e-6), dict(R=np.diag([1.0, 1.0, -1.0])), dict(R=R, s=0.0), dict(R=R, s=-1.0),
                dict(R=R, s=float("nan")), dict(R=R[:2]), dict(R=R, t=(1.0, 2.0)), dict(R=R, t=(0.0, float("inf"), 0.0))):
        with pytest.raises(ValueError):
            T.Similarity(**bad)
    T.Similarity(R + 1e-11)                                               # inside the 1e-9 allowance
    M = T.Similarity(R, 2.0, (1, 2, 3)).matrix()
    for bad in (M[:3], M * np.array([1, 1, -1, 1.0])[None, :], np.vstack([M[:3], [0, 0, 1e-3, 1]]), M * np.array([[1], [2], [1], [1.0]])):
        with pytest.raises(ValueError):
            T.Similarity.from_matrix(bad)


# ---- the satellite frame against the reference's own loader --------------------------------------------------------------------
def test_satellite_normalisation_and_frame_reproduce_the_reference_loader():
    pts, R_fix, T_fix = G["sat_points"], G["sat_R_fix"], G["sat_T_fix"]
    scale, z_min = T.satellite_normalisation(pts, R_fix, T_fix)
    assert scale == float(G["sat_scale"]) and z_min == float(G["sat_z_min"])
    sim = T.Similarity.from_satellite_frame(R_fix, T_fix, scale, z_min)
    got, want = sim.apply(pts), G["sat_points_normalised"].astype(np.float64)
    # the PLY stores float32: 1e-5 relative
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    assert abs(np.percentile(got[:, 2], 1)) <= 1e-9                       # what the drop is for
    np.testing.assert_allclose(sim.inverse().apply(got), pts, rtol=0, atol=1e-9)


def test_transform_camera_reproduces_the_reference_camera_normalisation():
    """The reference's cameras come from transform_matrix_rotated and take only the scale-and-drop part (:397-457)."""
    part = T.Similarity(np.eye(3), float(G["sat_scale"]), (0.0, 0.0, -float(G["sat_z_min"])))
    assert len(G["sat_cam_R_in"]) == 5
    for R, Tc, R_want, T_want in zip(G["sat_cam_R_in"], G["sat_cam_T_in"], G["sat_cam_R_out"], G["sat_cam_T_out"]):
        for fn in (T.transform_camera, tnp.camera):
            R_new, T_new = fn(R, Tc, part)
            np.testing.assert_allclose(R_new, R_want, rtol=0, atol=1e-9)
            np.testing.assert_allclose(T_new, T_want, rtol=0, atol=1e-9 * max(1.0, np.abs(T_want).max()))
    # a full similarity: camera-space coordinates of transformed points are s times the old ones
    sim = tnp.render_similarity()
    R, Tc = G["sat_cam_R_in"][0], G["sat_cam_T_in"][0]
    R2, T2 = T.transform_camera(R, Tc, sim)
    x = np.random.default_rng(3).normal(size=(6, 3)) * 100
    np.testing.assert_allclose(sim.apply(x) @ R2 + T2, sim.s * (x @ R + Tc), rtol=0, atol=1e-9 * np.abs(Tc).max())


# ---- render invariance of the restatement, through the C oracle ----------------------------------------------------------------
@pytest.mark.parametrize("form", list(tnp.RENDER_FORMS))
def test_restatement_is_render_invariant_through_the_oracle(form):
    sim = tnp.render_similarity()
    frame, g, R, Tc = tnp.render_case(form)
    want = orc.OracleRender(frame, **g)
    assert int((want.radii > 0).sum()) == tnp.RENDER_N and int((want.alpha > 0.01).sum()) > 500       # every splat on screen
    moved = tnp.transform_scene(g, sim)                                   # float64, rounded to float32
    got = orc.OracleRender(tnp.moved_frame(frame, *T.transform_camera(R, Tc, sim)), **moved)
    reps = [parity.assert_image_close("color", got.color, want.color, rtol=parity.RGB_DEPTH_RTOL),
            parity.assert_image_close("alpha", got.alpha, want.alpha, rtol=parity.RGB_DEPTH_RTOL),
            parity.assert_image_close("depth", got.depth / np.float32(sim.s), want.depth, rtol=parity.RGB_DEPTH_RTOL)]
    print(form, reps)
    np.testing.assert_array_equal(got.radii, want.radii)
    if frame["sh_degree"] > 0:                                            # the colour really turns: unrotated SH fail
        lazy = dict(moved, shs=g["shs"].numpy())
        bad = orc.OracleRender(tnp.moved_frame(frame, *T.transform_camera(R, Tc, sim)), **lazy)
        assert parity.image_report("color", bad.color, want.color)["max_rel"] > 10 * parity.RGB_DEPTH_RTOL


# ---- argument checks, before the library is touched ----------------------------------------------------------------------------
def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load", no_library)
    sim = T.Similarity.identity()
    x = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="sim must be a Similarity"):
        T.transform_gaussians(np.eye(4), x)
    with pytest.raises(ValueError, match="at least one tensor"):
        T.transform_gaussians(sim, None)
    with pytest.raises(ValueError, match="rest_layout"):
        T.transform_gaussians(sim, x, rest_layout="kn3")
    with pytest.raises(ValueError, match="xyz must be float32"):
        T.transform_gaussians(sim, x.double())
    with pytest.raises(ValueError, match=r"xyz must be \[5,3\]"):
        T.transform_gaussians(sim, torch.zeros(5, 4))
    with pytest.raises(ValueError, match=r"scaling must be \[5,3\]"):
        T.transform_gaussians(sim, x, scaling=torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"rotation must be \[5,4\]"):
        T.transform_gaussians(sim, x, rotation=torch.zeros(5, 3))
    with pytest.raises(ValueError, match="filter_3D must be"):
        T.transform_gaussians(sim, x, filter_3D=torch.zeros(5, 2))
    for bad in (torch.zeros(5, 4, 3), torch.zeros(5, 3, 15), torch.zeros(5, 45)):
        with pytest.raises(ValueError, match="features_rest must be"):
            T.transform_gaussians(sim, x, features_rest=bad)
    with pytest.raises(ValueError, match="features_rest must be"):
        T.transform_gaussians(sim, x, features_rest=torch.zeros(5, 15, 3), rest_layout="n3k")
    with pytest.raises(ValueError, match="contiguous"):
        T.transform_gaussians(sim, torch.zeros(3, 5).t(), inplace=True)
    with pytest.raises(ValueError, match="xyz must be a GPU tensor"):      # everything right but the device: no fallback
        T.transform_gaussians(sim, x, torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(5, 15, 3), torch.zeros(5, 1))
    model = types.SimpleNamespace(optimizer=object())
    with pytest.raises(ValueError, match="optimizer"):
        T.transform_model(model, sim)
    with pytest.raises(ValueError, match="sim must be a Similarity"):
        T.transform_camera(np.eye(3), np.zeros(3), np.eye(4))


def test_merge_fused_plys_refuses_offsets_together_with_transforms(tmp_path):
    from sfgs import ply
    with pytest.raises(ValueError, match="mutually exclusive"):
        ply.merge_fused_plys([str(tmp_path / "a.ply")], offsets=[(0, 0, 0)], transforms=[T.Similarity.identity()])
    table = np.zeros(3, dtype=[(n, "f4") for n in ("x", "y", "z", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")])
    ply.write_ply(str(tmp_path / "a.ply"), table)
    with pytest.raises(ValueError, match="one transform per file"):
        ply.merge_fused_plys([str(tmp_path / "a.ply")], transforms=[])
    with pytest.raises(ValueError, match="Similarity"):
        ply.merge_fused_plys([str(tmp_path / "a.ply")], transforms=[np.eye(4)])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    m = re.search(r"\bsfgs_similarity_transform\s*\(([^;]*)\)\s*;", hdr)
    assert m, "sfgs_similarity_transform is not declared in include/sfgs.h"
    assert len(m.group(1).split(",")) == len(L.SYMBOLS["sfgs_similarity_transform"][1])
    assert lib.sfgs_similarity_transform is not None
    declared_version = int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1))
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() and L.ABI_VERSION >= 26
    assert "dataset_readers.py:378-390" in hdr
    assert re.search(r"#define SFGS_SIM_SCALING_LOG 1", hdr) and re.search(r"#define SFGS_SIM_REST_N3K 2", hdr)
    assert (L.SIM_SCALING_LOG, L.SIM_REST_N3K) == (1, 2)
    fields = [f for f, _ in L.SfgsSimilarityArgs._fields_]
    body = re.search(r"typedef struct SfgsSimilarityArgs \{(.*?)\} SfgsSimilarityArgs;", hdr, re.S).group(1)
    declared = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields
    src = tmp_path / "layout.c"
    prints = "\n".join(f'  printf("{f} %zu\\n", offsetof(SfgsSimilarityArgs, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                   f'  printf("sizeof %zu\\n", sizeof(SfgsSimilarityArgs));\n{prints}\n  return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SfgsSimilarityArgs)
    for f in fields:
        assert int(out[f]) == getattr(L.SfgsSimilarityArgs, f).offset, f


def test_gpu_free_entry_point_validates_its_arguments():
    lib = L.load()
    dummy = C.c_double(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value

    def args(**kw):
        a = L.SfgsSimilarityArgs()
        a.struct_size, a.n, a.sh_rest_coeffs = C.sizeof(L.SfgsSimilarityArgs), 1000, 15
        a.xyz_in = a.xyz_out = a.sh_rest_in = a.sh_rest_out = fp
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    call = lambda a: lib.sfgs_similarity_transform(C.byref(a), None)
    assert lib.sfgs_similarity_transform(None, None) == -1
    assert call(args(struct_size=8)) == -1 and b"struct_size" in lib.sfgs_last_error()
    # status codes before any HIP call: the pointers are never dereferenced
    for bad in (dict(n=-1), dict(flags=4), dict(flags=-1), dict(sh_rest_coeffs=4), dict(sh_rest_coeffs=24), dict(sh_rest_coeffs=0),
                dict(xyz_out=None), dict(sh_rest_out=None), dict(scaling_in=fp), dict(rotation_in=fp), dict(filter3d_in=fp)):
        assert call(args(**bad)) == -1, bad
    assert call(args(n=1 << 31)) == -4 and b"2^31" in lib.sfgs_last_error()
    # nothing to do: no launch, no device needed
    assert call(args(n=0)) == 0
    assert call(args(xyz_in=None, xyz_out=None, sh_rest_in=None, sh_rest_out=None)) == 0
