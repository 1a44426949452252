"""The rasterizer on the GPU against the CPU oracle under general cameras (tests/camera_cases.py; DESIGN.md section 8.7, "General cameras").

Every other parity test uses the camera of sfgs.synth.scene: at the world origin, identity rotation or an x pitch with
unchanged view coordinates, centred principal point, scale_modifier 1, fx = fy, everything in front of the camera and
inside the guard band of the EWA Jacobian. Under that camera a row / column slip in the view matrix, a dropped PM[8] /
PM[9] term of the mean2D backward, a backward that ignores x_mul / y_mul or the `mod` factor of the scale gradient all
cancel or multiply zeros. Here every case uses a general pose, and each one adds the setting it is named after. The
oracle was first held to the dense float64 autograd render under the same settings (tests/test_camera_cases_cpu.py).

Whole-tensor bars cannot see a minority of rows, so the rows a case exists for (clamped Jacobian, tz just above the near
cull) are also judged on their own, and by the per-Gaussian bound in tests/test_gpu_grad_per_gaussian.py."""
import numpy as np
import pytest
import torch

import camera_cases as cc
import grad_bounds as gb
import parity
import raster_chain_np
from oracle import oracle as orc
from sfgs.synth import upstream_grads
from test_gpu_raster import run_hip

pytestmark = pytest.mark.gpu

_REF, _OUT = {}, {}


def reference(case):
    """oracle forward + backward of a case under the standard (unmasked) upstream gradients, once per process; read-only"""
    if case not in _REF:
        frame, g, reach = cc.case(case)
        R = orc.OracleRender(frame, **g)
        gc, gd = upstream_grads(frame["W"], frame["H"], 0)
        gd = gd.clone()
        gd[torch.from_numpy(np.isnan(R.depth))] = 0
        _REF[case] = dict(frame=frame, g=g, reach=reach, R=R, gc=gc, gd=gd, G=R.backward(gc, gd))
    return _REF[case]


def gpu(case):
    """the same frame on the GPU, once per process; read-only"""
    if case not in _OUT:
        r = reference(case)
        _OUT[case] = run_hip(r["frame"], r["g"], r["gc"], r["gd"])
    return _OUT[case]


def _rel(got, ref, rows):
    return float(np.abs(np.asarray(got, np.float64)[rows] - np.asarray(ref, np.float64)[rows]).max()
                 / max(np.abs(ref[rows]).max(), 1e-30))


@pytest.mark.parametrize("case", list(cc.CASES))
def test_every_output_against_the_oracle(case):
    import hostcheck
    r = reference(case)
    R, G, g = r["R"], r["G"], r["g"]
    out = gpu(case)
    np.testing.assert_array_equal(out["radii"], R.radii)
    assert out["counters"]["num_visible"] == R.num_visible
    assert out["counters"]["num_duplicates_ref"] == R.num_duplicates
    # the product's own 8x8 bins have no oracle counterpart: the host build of raster_math.h bins the same
    h = hostcheck.render(r["frame"], g["means3D"], g["scales"], g["rotations"], g["opacities"], g["colors_precomp"], g["shs"])
    assert out["counters"]["num_duplicates"] == int(h["counters"][0])
    assert out["counters"]["max_tile_list"] == int(h["counters"][3])
    reps = [parity.assert_image_close(name, out[name], getattr(R, name), rtol=parity.RGB_DEPTH_RTOL, borderline_min=4)
            for name in ("color", "alpha", "depth")]
    for k in G:
        reps.append(parity.assert_grad_close(k, out["grads"][k], G[k]))
    with_grad = np.abs(G["means3D"]).max(axis=1) > 0
    print(case, f"visible {R.num_visible}, with a gradient {int(with_grad.sum())}, longest 16x16 list {R.max_tile_list}", reps)
    assert with_grad.sum() >= 0.25 * len(with_grad)


def _minority(case):
    """(rows, what): the Gaussians the case exists for, among those with a reference gradient under the masked upstream"""
    ref = gb.reference(case)
    frame, _, reach = cc.case(case)
    with_grad = gb.has_gradient(case)
    if case == "clamped_jacobian":
        cx, cy = cc.clamped(frame, reach)
        print(case, "clamped in x", int((cx & with_grad).sum()), "in y", int((cy & with_grad).sum()), "in both",
              int((cx & cy & with_grad).sum()))
        assert (cx & with_grad).sum() >= 50 and (cy & with_grad).sum() >= 50 and (cx & cy & with_grad).sum() >= 5
        # the builder's float64 view transform and the oracle's float32 one take the same side of the guard band
        st = ref["R"].chain_state()
        lim = np.float32(cc.GUARD) * np.float32(frame["tanfovx"]), np.float32(cc.GUARD) * np.float32(frame["tanfovy"])
        vis = ref["R"].radii > 0
        for flag, col, l in ((cx, 3, lim[0]), (cy, 4, lim[1])):
            q = st[:, col].astype(np.float32) / st[:, 5].astype(np.float32)
            np.testing.assert_array_equal(flag[vis], (np.abs(q) > l)[vis])
        return (cx | cy) & with_grad
    near, culled = cc.near_band(reach)
    print(case, "0.2 < tz < 0.3 with a gradient", int((near & with_grad).sum()), "culled with 0 < tz <= 0.2", int(culled.sum()))
    assert (near & with_grad).sum() >= 100 and culled.sum() >= 100
    return near & with_grad


@pytest.mark.parametrize("case", ["clamped_jacobian", "near_plane"])
def test_the_minority_rows_on_their_own(case):
    """The clamped rows (x_mul / y_mul = 0, ux / uy clamped) and the rows with a 1 / tz^3 of up to 125 in the backward,
    each within parity.GRAD_RTOL_MAX of the SUBSET's maximum. The upstream gradients are zero on the masked pixels
    (grad_bounds.upstream), so a threshold flip cannot be blamed. For the clamp the test shows that it can fail: the
    float64 chain without x_mul / y_mul, from the oracle's own 2D sums, leaves the bar on these rows (by 0.126 of the rows'
    maximum, 63 bars)."""
    ref = gb.reference(case)
    rows = _minority(case)
    out = run_hip(ref["frame"], ref["g"], ref["gc"], ref["gd"])
    np.testing.assert_array_equal(out["radii"], ref["R"].radii)
    for k in ("means3D", "scales", "rotations", "means2D"):
        got, want = out["grads"][k], ref["G"][k]
        if k == "means2D":
            got, want = got[:, :2], want[:, :2]
        e = _rel(got, want, rows)
        print(f"{case} {k}: {int(rows.sum())} rows within {e:.3g} of their maximum (bar {parity.GRAD_RTOL_MAX:g})")
        assert np.isfinite(got).all() and e <= parity.GRAD_RTOL_MAX, k
    if case == "clamped_jacobian":
        wrong = clamp_ignored(ref)
        sep = _rel(wrong, ref["G"]["means3D"], rows)
        print(f"{case}: without x_mul / y_mul the rows move by {sep:.3g} of their maximum")
        assert sep > parity.GRAD_RTOL_MAX
        assert _rel(out["grads"]["means3D"], wrong, rows) > parity.GRAD_RTOL_MAX      # ... and the GPU is not that chain


def clamp_ignored(ref):
    """means3D gradient of the float64 chain that lets a clamped coordinate pass its gradient on (a defect, on purpose)"""
    f = {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in ref["frame"].items() if v is not None}
    g = ref["g"]
    shs = None if g["shs"] is None else g["shs"].numpy()
    return raster_chain_np.chain(f, g["means3D"].numpy(), g["scales"].numpy(), g["rotations"].numpy(),
                                 g["opacities"].numpy(), shs, ref["R"].chain_state(), ref["R"].radii > 0,
                                 ref["sums"][:, :12], clamp_mul=False)["means3D"]


@pytest.mark.parametrize("case", ["near_plane", "behind_camera", "clamped_jacobian"])
def test_culled_gaussians_get_no_radius_and_exactly_zero_gradients(case):
    """Behind the camera hw is negative, the NDC position is mirrored and pw = 1 / (hw + 1e-7): nothing of that may reach
    a gradient row, as a number or as a NaN."""
    r = reference(case)
    out = gpu(case)
    culled = r["R"].radii == 0
    tz = r["reach"]["tz"]
    print(case, "culled", int(culled.sum()), "of them behind the camera", int((culled & (tz < 0)).sum()),
          "in front of the near cull", int((culled & (tz > 0) & (tz <= cc.NEAR)).sum()))
    want = {"near_plane": 100, "behind_camera": 1600, "clamped_jacobian": 1}[case]
    assert culled.sum() >= want
    if case == "behind_camera":
        assert (tz < 0).sum() == 1600 and culled[tz < 0].all() and r["R"].num_visible == 2400
    assert (out["radii"][culled] == 0).all()
    for k, v in out["grads"].items():
        assert np.isfinite(v).all(), k
        assert (v[culled] == 0).all(), k
    for name in ("color", "alpha"):
        assert np.isfinite(out[name]).all(), name


@pytest.mark.parametrize("case", ["pose_offcentre_sh3", "behind_camera"])
def test_sh_view_direction_under_a_translated_camera(case):
    """campos = (12, -7, 3): the view direction p - campos and its gradient into means3D. The oracle with the SH colours
    it evaluated handed back as precomputed colours renders the same image, and its means3D gradient lacks exactly the
    direction term: that term is above the bar the GPU meets against the oracle with SH, so losing it would be seen."""
    r = reference(case)
    R, G = r["R"], r["G"]
    deg = r["frame"]["sh_degree"]
    assert np.abs(G["shs"][:, deg * deg:]).max() > 0                    # the highest band receives gradients
    g2 = dict(r["g"], shs=None, colors_precomp=torch.from_numpy(R.geom()[:, 7:10].copy()))
    R2 = orc.OracleRender(dict(r["frame"], sh_degree=0), **g2)
    np.testing.assert_array_equal(R2.color, R.color)
    G2 = R2.backward(r["gc"], r["gd"])
    rows = np.abs(G["means3D"]).max(axis=1) > 0
    term = _rel(G2["means3D"], G["means3D"], rows)
    got = parity.grad_report("means3D", gpu(case)["grads"]["means3D"], G["means3D"])
    print(f"{case}: the SH direction term is {term:.3g} of the largest means3D gradient; GPU against the oracle {got}")
    assert term > parity.GRAD_RTOL_MAX
    assert got["rel_max"] <= parity.GRAD_RTOL_MAX and got["rel_l2"] <= parity.GRAD_RTOL_L2
    parity.assert_grad_close("shs, highest band", gpu(case)["grads"]["shs"][:, deg * deg:], G["shs"][:, deg * deg:])
