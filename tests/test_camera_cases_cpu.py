"""General cameras on the CPU (tests/camera_cases.py): the references first, then the product's host build.

1. The C oracle against the dense float64 autograd render (oracle/dense_torch.py) under every camera setting of
   camera_cases.CASES, at a size the dense render can carry (n <= 200, 48x40): a general pose, an off-centre principal
   point, scale_modifier != 1, fx != fy, splats beyond the Jacobian's guard band, depths down to the near cull, points
   behind the camera. Only after this may the oracle judge the kernels under these settings (tests/test_gpu_camera_model.py).
2. The product's math header compiled for the host (tests/hostcheck.py) against the oracle at GPU size: projection, tile
   rectangles and culling without a GPU, and the forward / backward at the standard parity bars.
The per-Gaussian bound of the three cases that tests/grad_bounds.py takes is covered by tests/test_grad_bounds_cpu.py."""
import numpy as np
import pytest
import torch

import camera_cases as cc
import parity
from oracle import oracle as orc
from oracle.dense_torch import render_dense
from sfgs.synth import upstream_grads

SMALL = dict(pose_offcentre_sh3=100, modifier_0p8=100, modifier_1p7_sh1=100, anamorphic=100, clamped_jacobian=200,
             near_plane=200, behind_camera=200)
# forward bar (colour, alpha) of the oracle against the dense render: 1e-5 as in test_oracle_cpu.py where it holds. It
# does not in the two cases with splats at tz < 1, where 1 / tz is steep and the C oracle is float32: measured 4.02e-5
# (near_plane, alpha) and 2.53e-5 (behind_camera, colour; 1.04e-5 with the same depths and nothing behind the camera; the
# dense render in float32 differs from itself in float64 by 5.7e-5 and 1.8e-5 there). Bar = 4 x the measured difference,
# rounded up to one significant digit.
FWD_BAR = dict(near_plane=2e-4, behind_camera=2e-4)


def _dense(frame, g, n, gc, gd):
    gi = {k: (v.double().requires_grad_(True) if v is not None else None) for k, v in g.items()}
    m2 = torch.zeros(n, 3, dtype=torch.float64, requires_grad=True)
    c, d, a, rad = render_dense(frame, gi["means3D"], gi["scales"], gi["rotations"], gi["opacities"],
                                gi["colors_precomp"], gi["shs"], means2D=m2)
    loss = (c * gc.double()).sum() + (torch.where(torch.isnan(d), torch.zeros_like(d), d) * gd.double()).sum()
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in gi.items() if v is not None}
    grads["means2D"] = m2.grad.numpy()
    return c.detach().numpy(), d.detach().numpy(), a.detach().numpy(), rad.numpy(), grads


@pytest.mark.parametrize("case", list(cc.CASES))
def test_c_oracle_matches_dense_float64_autograd_under_general_cameras(case):
    """Measured (oracle against dense, this size): colour / alpha 4.02e-5 in near_plane, 2.53e-5 in behind_camera and
    <= 5.5e-6 in the other five; depth <= 5.8e-5; every gradient tensor within 1.2e-4 of its maximum (modifier_0p8,
    rotations; <= 9.3e-5 otherwise); the 71 clamped rows of clamped_jacobian within 1.1e-6 of those rows' maximum."""
    W, H, n = 48, 40, SMALL[case]
    frame, g, reach = cc.case(case, n=n, W=W, H=H)
    R = orc.OracleRender(frame, **g)
    gc, gd = upstream_grads(W, H, 0)
    gc, gd = gc * W * H, gd * W * H
    c, dn, a, rad, ref = _dense(frame, g, n, gc, gd)
    np.testing.assert_array_equal(R.radii, rad)
    bar = FWD_BAR.get(case, 1e-5)
    ec, ea = np.abs(R.color - c).max(), np.abs(R.alpha - a).max()
    assert (np.isnan(R.depth) == np.isnan(dn)).all()
    fin = np.isfinite(dn)
    ed = np.abs(R.depth - dn)[fin].max()
    print(f"{case}: visible {R.num_visible} of {n}; colour {ec:.2e} alpha {ea:.2e} (bar {bar:g}) depth {ed:.2e}")
    assert ec < bar and ea < bar and ed < 2e-4
    gdm = gd.clone()
    gdm[torch.from_numpy(np.isnan(dn))] = 0
    Gr = R.backward(gc, gdm)
    for k in ("means3D", "scales", "rotations", "opacities", "colors_precomp", "shs"):
        if k in Gr:
            want = ref[k].reshape(Gr[k].shape)
            e = np.abs(Gr[k] - want).max() / np.abs(want).max()
            print(f"{case} {k}: {e:.2e} of the tensor's maximum")
            assert np.isfinite(Gr[k]).all() and e <= 2e-4, k
    want = ref["means2D"][:, :2]
    assert np.abs(Gr["means2D"][:, :2] - want).max() <= 2e-4 * np.abs(want).max()
    # each setting reaches what it is there for
    vis = R.radii > 0
    if case == "clamped_jacobian":
        cx, cy = cc.clamped(frame, reach)
        rows = (cx | cy) & vis & (np.abs(ref["means3D"]).max(axis=1) > 0)
        assert (cx & rows).sum() >= 10 and (cy & rows).sum() >= 10 and (cx & cy & rows).sum() >= 2
        for k in ("means3D", "scales"):       # whole-tensor bars cannot see these rows
            e = np.abs(Gr[k][rows] - ref[k][rows]).max() / np.abs(ref[k][rows]).max()
            print(f"{case} {k}, {int(rows.sum())} clamped rows: {e:.2e} of those rows' maximum")
            assert e <= 2e-4, k
    if case == "near_plane":
        near, culled = cc.near_band(reach)
        assert (near & vis).sum() >= 10 and culled.sum() >= 5 and not (culled & vis).any()
    if case == "behind_camera":
        behind = reach["tz"] < 0
        assert behind.sum() == int(round(0.4 * n)) and not (behind & vis).any() and vis.sum() >= 50
    if frame["sh_degree"] > 0:
        assert np.abs(ref["shs"][:, -(2 * frame["sh_degree"] + 1):]).max() > 0     # the highest band takes part
    for k in Gr:                         # culled Gaussians: zero rows, in the oracle and in autograd
        assert (Gr[k][~vis] == 0).all() and (ref[k].reshape(Gr[k].shape)[~vis] == 0).all(), k


_AT_GPU_SIZE = {}


def at_gpu_size(case):
    """oracle forward + backward of a case at GPU size, once per process: (frame, g, reach, R, gc, gd, G)"""
    if case not in _AT_GPU_SIZE:
        frame, g, reach = cc.case(case)
        R = orc.OracleRender(frame, **g)
        gc, gd = upstream_grads(frame["W"], frame["H"], 0)
        gd = gd.clone()
        gd[torch.from_numpy(np.isnan(R.depth))] = 0
        _AT_GPU_SIZE[case] = (frame, g, reach, R, gc, gd, R.backward(gc, gd))
    return _AT_GPU_SIZE[case]


@pytest.mark.parametrize("case", list(cc.CASES))
def test_host_build_of_the_product_projects_bins_and_renders_as_the_oracle(case):
    """raster_math.h compiled for the host: radii bit-equal, the same Gaussians visible, the same 16x16 tile rectangles
    (their total is the oracle's duplicate count). The host build's own list counters are those of the product's exact 8x8
    bins, which the oracle does not have: they are bounded by the oracle's here (an 8x8 bin's list is part of its 16x16
    tile's) and compared with the GPU for equality in tests/test_gpu_camera_model.py. Forward and backward at the standard
    parity bars; culled Gaussians get exactly zero rows."""
    import hostcheck
    frame, g, reach, R, gc, gd, G = at_gpu_size(case)
    h = hostcheck.render(frame, g["means3D"], g["scales"], g["rotations"], g["opacities"], g["colors_precomp"], g["shs"],
                         gc, gd, None, backward=True)
    np.testing.assert_array_equal(h["radii"], R.radii)
    d_eff, d_ref, n_vis, longest = (int(v) for v in h["counters"])
    assert n_vis == R.num_visible and d_ref == R.num_duplicates
    assert 0 < longest <= R.max_tile_list and d_eff <= 4 * d_ref
    for name in ("color", "alpha", "depth"):
        parity.assert_image_close(name, h[name], getattr(R, name), borderline_min=4)
    for k in G:
        parity.assert_grad_close(k, h["grads"][k], G[k])
        assert (h["grads"][k][R.radii == 0] == 0).all(), k


def test_cases_reach_their_branches_at_gpu_size():
    """The floors the GPU tests rely on, from the oracle (Gaussians with a non-zero means3D gradient)."""
    def with_grad(case):
        return np.abs(at_gpu_size(case)[6]["means3D"]).max(axis=1) > 0
    frame, _, reach, R, *_ = at_gpu_size("clamped_jacobian")
    cx, cy = cc.clamped(frame, reach)
    w = with_grad("clamped_jacobian")
    print("clamped_jacobian: clamped in x", int((cx & w).sum()), "in y", int((cy & w).sum()), "in both", int((cx & cy & w).sum()))
    assert (cx & w).sum() >= 50 and (cy & w).sum() >= 50 and (cx & cy & w).sum() >= 5
    _, _, reach, R, *_ = at_gpu_size("near_plane")
    near, culled = cc.near_band(reach)
    print("near_plane: 0.2 < tz < 0.3 with a gradient", int((near & with_grad("near_plane")).sum()), "culled in front", int(culled.sum()))
    assert (near & with_grad("near_plane")).sum() >= 100 and culled.sum() >= 100 and not (culled & (R.radii > 0)).any()
    _, _, reach, R, *_ = at_gpu_size("behind_camera")
    assert (reach["tz"] < 0).sum() == 1600 and R.num_visible == 2400 and not ((reach["tz"] < 0) & (R.radii > 0)).any()
    for case in ("pose_offcentre_sh3", "modifier_0p8", "modifier_1p7_sh1", "anamorphic"):
        frame, g, _, R, *_ = at_gpu_size(case)
        assert R.num_visible == g["means3D"].shape[0] and with_grad(case).all(), case
    assert at_gpu_size("modifier_1p7_sh1")[0]["W"] % 8 and at_gpu_size("modifier_1p7_sh1")[0]["H"] % 8     # ragged tiles
    f = at_gpu_size("anamorphic")[0]
    assert abs(f["W"] / f["tanfovx"] - f["H"] / f["tanfovy"]) > 0.1 * f["W"] / f["tanfovx"]                # fx != fy
