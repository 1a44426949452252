"""Rasterizer backward on the GPU against the CPU oracle, Gaussian by Gaussian and component by component:

    |got - ref| <= K[case][tensor] * 2^-23 * unit

with the unit, the pixel mask and the K table of tests/grad_bounds.py (all established against references only by
tests/test_grad_bounds_cpu.py). The whole-tensor tolerances of parity.assert_grad_close stay: they cannot see a dropped
record, a wrong live flag, a skipped chunk head or a bad lane of the cooperative sum unless it hits a splat with a large
gradient; this bound sees the loss of any single Gaussian's gradient (test_a_lost_gaussian_violates_the_bound). Every case
asserts that it reaches the path it is named after, and prints its worst Gaussian in units next to K."""
import numpy as np
import pytest
import torch

import grad_bounds as gb
import parity

pytestmark = pytest.mark.gpu


def run_hip(ref):
    """forward + backward of the case on the GPU with loss = sum color gc + depth gd (+ alpha ga)"""
    from diff_gauss import (GaussianRasterizationSettings, GaussianRasterizer, collect_full_counters, last_backward_hints,
                            last_counters)
    frame, g = ref["frame"], ref["g"]
    collect_full_counters(True)
    try:
        dev = torch.device("cuda:0")
        sub = frame.get("subpix")
        settings = GaussianRasterizationSettings(
            image_height=frame["H"], image_width=frame["W"], tanfovx=frame["tanfovx"], tanfovy=frame["tanfovy"],
            kernel_size=frame["kernel_size"], subpixel_offset=None if sub is None else sub.to(dev),
            bg=frame["bg"].to(dev), scale_modifier=frame["scale_modifier"], viewmatrix=frame["view"].to(dev),
            projmatrix=frame["proj"].to(dev), sh_degree=frame["sh_degree"], campos=frame["campos"].to(dev),
            prefiltered=False, debug=True, depth_mode=int(frame.get("depth_mode", 0)))
        t = {k: (v.to(dev).requires_grad_(True) if v is not None else None) for k, v in g.items()}
        means2D = torch.zeros_like(t["means3D"], requires_grad=True)
        color, depth, _, alpha, radii, _ = GaussianRasterizer(settings)(
            means3D=t["means3D"], means2D=means2D, shs=t["shs"], colors_precomp=t["colors_precomp"],
            opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"], cov3Ds_precomp=None)
        out = dict(radii=radii.cpu().numpy(), counters=last_counters())
        loss = (color * ref["gc"].to(dev)).sum() + (torch.nan_to_num(depth, nan=0.0) * ref["gd"].to(dev)).sum()
        if ref["ga"] is not None:
            loss = loss + (alpha * ref["ga"].to(dev)).sum()
        loss.backward()
        out["grads"] = {k: v.grad.cpu().numpy() for k, v in t.items() if v is not None}
        out["grads"]["means2D"] = means2D.grad.cpu().numpy()
        out["bwd_hints"] = last_backward_hints()
    finally:
        collect_full_counters(False)
    return out


def check(case, ref, out, whole_tensor=False):
    np.testing.assert_array_equal(out["radii"], ref["R"].radii)
    assert ref["share"] <= gb.MASK_CAP, ref["share"]
    failures = []
    for k, want in ref["G"].items():
        got = out["grads"][k]
        assert np.isfinite(got).all(), k
        e = gb.in_units(got, want, ref["unit"][k])
        i, K = int(e.argmax()), gb.k_of(case, k)
        print(f"{case} {k}: worst Gaussian {i} at {e[i]:.3g} units, K = {K:g} (masked pixels {ref['share']:.3%})")
        if not e[i] <= K:
            n = int(gb.record_counts(case)[i])
            bad = int((e > K).sum())
            failures.append(f"{k}: Gaussian {i} at {e[i]:.4g} units > K = {K:g}; {n} records, route {gb.route_of(n)}; "
                            f"{bad} Gaussians out of bound; got {got[i].ravel()[:4]} want {want[i].ravel()[:4]}")
        if whole_tensor:
            parity.assert_grad_close(k, got, want)
    assert not failures, "\n".join(failures)


def test_precomp_small_plain_path():
    ref = gb.reference("precomp_small")
    out = run_hip(ref)
    assert out["counters"]["num_big_chunks"] == 0 and out["counters"]["num_huge_splats"] == 0
    assert int(gb.record_counts("precomp_small").max()) <= 2048
    check("precomp_small", ref, out)


def test_sh1_ragged_partial_tiles_and_clamped_colours():
    ref = gb.reference("sh1_ragged")
    W, H = ref["frame"]["W"], ref["frame"]["H"]
    assert W % 16 and H % 16 and W % 8 and H % 8
    clamped = (ref["R"].chain_state()[:, 13:16] != 0).any(axis=1) & (ref["R"].radii > 0)
    with_grad = np.abs(ref["G"]["means3D"]).max(axis=1) > 0
    assert (clamped & with_grad).sum() >= 10       # clamped SH colours among the Gaussians that receive a gradient
    check("sh1_ragged", ref, run_hip(ref))


def test_sh3_jitter_subpixel_offsets_and_band3():
    ref = gb.reference("sh3_jitter")
    assert ref["frame"]["subpix"] is not None and ref["frame"]["sh_degree"] == 3
    assert np.abs(ref["G"]["shs"][:, 9:]).max() > 0      # the band-3 coefficients receive gradients
    check("sh3_jitter", ref, run_hip(ref))


def _dead_share(R):
    """share of the tile-list entries behind their tile's last contributor (oracle, 16x16 tiles)"""
    starts, _ = R.tile_lists()
    nc = R.n_contrib()
    TX = (R.W + 15) // 16
    dead = 0
    for t in range(len(starts) - 1):
        ty, tx = divmod(t, TX)
        dead += int(starts[t + 1] - starts[t]) - int(nc[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].max())
    return dead / max(int(starts[-1]), 1)


@pytest.mark.parametrize("hints", ["off", "prefill_skipped"])
def test_big_splats_dead_entries(hints, monkeypatch):
    """hints off: dupgrad_prefill_kernel runs and puts the frame on live flags (most entries are dead); the hint state
    that skips its launch: composite_bwd writes a zero record for every dead entry instead."""
    import diff_gauss
    ref = gb.reference("big_splats")
    assert _dead_share(ref["R"]) > 0.25
    diff_gauss._hint_state.clear()
    if hints == "off":
        monkeypatch.setenv("SFGS_HINTS", "0")
        out = run_hip(ref)
        assert out["bwd_hints"] & diff_gauss.HINT_NO_PREFILL == 0
    else:
        monkeypatch.setenv("SFGS_HINTS", "1")
        run_hip(ref)                                  # first frame of the stream: creates the hint state
        for hs in diff_gauss._hint_state.values():    # ... which now says: the prefill kernel kept answering no
            hs["prefilled"], hs["prefill_ran"] = 0, False
        out = run_hip(ref)
        assert out["bwd_hints"] & diff_gauss.HINT_NO_PREFILL
    diff_gauss._hint_state.clear()
    check("big_splats", ref, out)


def test_screen_filling_chunk_heads():
    ref = gb.reference("screen_filling")
    d = gb.record_counts("screen_filling")
    assert (d > 2048).sum() >= 20 and ((d > 2048) & (d % 1024 != 0)).any()
    out = run_hip(ref)
    # every Gaussian above BWD_BIG records is listed in ceil(n / BWD_CHUNK) chunks
    assert out["counters"]["num_big_chunks"] == int(((d[d > 2048] + 1023) // 1024).sum())
    check("screen_filling", ref, out)


def test_mixed_sizes_around_the_cooperative_threshold():
    ref = gb.reference("mixed_coop")
    d = gb.record_counts("mixed_coop")[gb.has_gradient("mixed_coop")]      # of the Gaussians that receive a gradient
    assert {31, 32, 33} <= set(d.tolist()) and ((d > 32) & (d <= 2048)).any() and (d > 2048).any()
    out = run_hip(ref)
    d = gb.record_counts("mixed_coop")
    assert out["counters"]["num_duplicates"] == int(d.sum())
    assert out["counters"]["num_big_chunks"] == int(((d[d > 2048] + 1023) // 1024).sum())
    check("mixed_coop", ref, out)


def test_lists_800_deep_lists():
    ref = gb.reference("lists_800")
    assert int(ref["R"].n_contrib().max()) > 256           # the transmittance chain really is deep
    out = run_hip(ref)
    assert 512 < out["counters"]["max_tile_list"] <= 1024
    check("lists_800", ref, out)


def test_clamped_jacobian_rows_beyond_the_guard_band():
    """general pose (tests/camera_cases.py); visible splats beyond 1.3 tanfov: ux / uy clamped, x_mul / y_mul = 0"""
    import camera_cases as cc
    ref = gb.reference("clamped_jacobian")
    frame, _, reach = cc.case("clamped_jacobian")
    cx, cy = cc.clamped(frame, reach)
    w = gb.has_gradient("clamped_jacobian")
    print("clamped_jacobian: with a gradient and clamped in x", int((cx & w).sum()), "in y", int((cy & w).sum()), "in both",
          int((cx & cy & w).sum()))
    assert (cx & w).sum() >= 50 and (cy & w).sum() >= 50 and (cx & cy & w).sum() >= 5
    check("clamped_jacobian", ref, run_hip(ref), whole_tensor=True)


def test_near_plane_depths_down_to_the_cull():
    """general pose; 1 / tz^3 of up to 125 in the backward, and Gaussians on the other side of tz > 0.2 in the same frame"""
    import camera_cases as cc
    ref = gb.reference("near_plane")
    near, culled = cc.near_band(cc.case("near_plane")[2])
    w = gb.has_gradient("near_plane")
    print("near_plane: with a gradient and 0.2 < tz < 0.3", int((near & w).sum()), "culled with 0 < tz <= 0.2", int(culled.sum()))
    assert (near & w).sum() >= 100 and culled.sum() >= 100 and (ref["R"].radii[culled] == 0).all()
    check("near_plane", ref, run_hip(ref), whole_tensor=True)


def test_general_pose_offcentre_principal_point_and_band3():
    """general pose, principal point at (0.12, -0.08) NDC, SH degree 3 seen from campos = (12, -7, 3)"""
    ref = gb.reference("pose_offcentre_sh3")
    f = ref["frame"]
    assert f["sh_degree"] == 3 and float(f["campos"].abs().min()) > 1
    P = f["proj"].numpy()
    assert abs(P[2, 0]) > 0.05 and abs(P[2, 1]) > 0.05                       # the principal-point terms of mean2D
    rot = np.abs(f["view"].numpy()[:3, :3]).ravel()
    assert rot.min() > 0.01 and np.diff(np.sort(rot)).min() > 0.01           # no entry is zero, no two can be swapped
    assert gb.has_gradient("pose_offcentre_sh3").all()
    assert np.abs(ref["G"]["shs"][:, 9:]).max() > 0
    check("pose_offcentre_sh3", ref, run_hip(ref), whole_tensor=True)


@pytest.mark.parametrize("case", ["precomp_small_alpha", "precomp_small_alpha_raw", "big_splats_alpha",
                                  "big_splats_alpha_raw"])
def test_alpha_term_and_raw_depth_mode(case):
    """loss = sum color gc + depth gd + alpha ga, in normalised and in raw depth mode: the per-Gaussian bound and the
    existing whole-tensor tolerances."""
    ref = gb.reference(case)
    assert ref["ga"] is not None and float(ref["ga"].abs().max()) > 0
    assert int(ref["frame"]["depth_mode"]) == (1 if case.endswith("_raw") else 0)
    check(case, ref, run_hip(ref), whole_tensor=True)
