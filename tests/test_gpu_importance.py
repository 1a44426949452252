"""sfgs.importance on the GPU: per-Gaussian blend-weight statistics against the float32 restatement and the oracle's exported
sum (tests/importance_np.py: reference, units and the K table, all established without the implementation by
tests/test_importance_host.py), against the existing backward (sum w = d(sum red) / d colors_precomp[:, 0]), and the bitwise
properties of the integer tables."""
import numpy as np
import pytest
import torch

import grad_bounds as gb
import importance_np as inp
import parity

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _settings(frame, debug=True, **kw):
    from diff_gauss import GaussianRasterizationSettings
    sub = frame.get("subpix")
    return GaussianRasterizationSettings(
        image_height=frame["H"], image_width=frame["W"], tanfovx=frame["tanfovx"], tanfovy=frame["tanfovy"],
        kernel_size=frame["kernel_size"], subpixel_offset=None if sub is None else sub.to(DEV), bg=frame["bg"].to(DEV),
        scale_modifier=frame["scale_modifier"], viewmatrix=frame["view"].to(DEV), projmatrix=frame["proj"].to(DEV),
        sh_degree=frame["sh_degree"], campos=frame["campos"].to(DEV), prefiltered=False, debug=debug,
        depth_mode=int(frame.get("depth_mode", 0)), **kw)


def _inputs(g):
    return {k: (None if v is None else v.to(DEV)) for k, v in g.items()}


def _tables(s):
    torch.cuda.synchronize()
    return dict(q=s.weight_sum_q32.cpu().numpy(), sum=s.weight_sum.cpu().numpy(), max=s.weight_max.cpu().numpy(),
                hits=s.hits.cpu().numpy(), views=s.views.cpu().numpy())


def _same(a, b, keys=("q", "max", "hits", "views")):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _check_against_reference(name, got, w, ref_sum, tol_sum, tol_max):
    assert np.isfinite(got["sum"]).all() and np.isfinite(got["max"]).all()
    np.testing.assert_array_equal(got["hits"], w["hits"])
    never = w["hits"] == 0
    assert not got["q"][never].any() and not got["max"][never].any() and not got["views"][never].any()
    np.testing.assert_array_equal(got["views"], (w["hits"] > 0).astype(np.int32))
    ds, dm = np.abs(got["sum"] - ref_sum), np.abs(got["max"].astype(np.float64) - w["max"])
    with np.errstate(divide="ignore", invalid="ignore"):
        es, em = np.where(ds == 0, 0.0, ds / tol_sum), np.where(dm == 0, 0.0, dm / tol_max)
    print(f"{name}: worst sum at {es.max():.3g} of its bound (Gaussian {int(es.argmax())}), worst max at {em.max():.3g} "
          f"(Gaussian {int(em.argmax())}); {int(never.sum())} of {never.size} never blended")
    assert es.max() <= 1.0, (int(es.argmax()), got["sum"][es.argmax()], ref_sum[es.argmax()])
    assert em.max() <= 1.0, (int(em.argmax()), got["max"][em.argmax()], w["max"][em.argmax()])


# ---- 1. the five cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", inp.CASES)
def test_case_against_restatement_and_oracle(case):
    from sfgs.importance import BlendStats
    r = inp.reference(case)
    assert r["share"] <= gb.MASK_CAP
    s = BlendStats(r["R"].N, DEV)
    color, depth, alpha = s.add(_settings(r["frame"]), pixel_mask=torch.from_numpy(r["keep"]).to(DEV), **_inputs(r["g"]))
    got = _tables(s)
    assert s.num_views == 1
    # the render it returns is the inference frame of the same plan
    parity.assert_image_close("alpha", alpha.cpu().numpy(), r["R"].alpha)
    tol_sum, tol_max = inp.bounds(case)
    _check_against_reference(case, got, r["walk"], r["osum"], tol_sum, tol_max)


# ---- 2. the existing backward ----------------------------------------------------------------------------------------------
def test_sum_equals_the_colour_gradient_of_the_backward():
    from diff_gauss import GaussianRasterizer
    from sfgs.importance import BlendStats
    from sfgs.synth import scene
    frame, g = scene(100_000, 512, 384, seed=5)
    t = _inputs(g)
    settings = _settings(frame, debug=False)
    s = BlendStats(100_000, DEV)
    s.add(settings, **t)
    colors = t["colors_precomp"].clone().requires_grad_(True)
    color = GaussianRasterizer(settings)(means3D=t["means3D"], means2D=None, colors_precomp=colors, opacities=t["opacities"],
                                        scales=t["scales"], rotations=t["rotations"])[0]
    color[0].sum().backward()
    grad = colors.grad[:, 0].double().cpu().numpy()
    got = _tables(s)
    rel = np.linalg.norm(got["sum"] - grad) / np.linalg.norm(grad)
    print(f"weight_sum against colors_precomp.grad[:, 0]: rel-L2 {rel:.3g}; {int((got['hits'] > 0).sum())} of 100000 blended")
    assert rel <= 1e-3
    np.testing.assert_array_equal(got["hits"] > 0, grad != 0)
    assert (got["hits"] > 0).sum() > 10_000 and not colors.grad[:, 1:].any()


# ---- 3. bitwise properties -------------------------------------------------------------------------------------------------
def test_runs_bands_and_views_are_exact():
    from sfgs.importance import BlendStats
    from sfgs.synth import scene
    W, H, n = 200, 120, 3000
    frame, g = scene(n, W, H, seed=7, zrange=(4., 8.), scale_range=(0.01, 0.2))
    frame_b, _ = scene(n, W, H, seed=7, zrange=(4., 8.), scale_range=(0.01, 0.2), fovx_deg=40.0)
    t = _inputs(g)
    a1, a2 = BlendStats(n, DEV), BlendStats(n, DEV)
    img1 = a1.add(_settings(frame), **t)
    img2 = a2.add(_settings(frame), **t)
    A = _tables(a1)
    _same(A, _tables(a2))
    for x, y in zip(img1, img2):
        assert torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
    assert A["hits"].sum() > 0
    # two tile-row bands into one table = the full frame
    rows = (H + 7) // 8
    halves = BlendStats(n, DEV)
    top = halves.add(_settings(frame, tile_rows=(0, 7)), **t)
    bottom = halves.add(_settings(frame, tile_rows=(7, rows)), **t)
    _same(A, _tables(halves), keys=("q", "hits", "max"))
    assert halves.num_views == 2
    assert torch.equal(top[0] + bottom[0], img1[0]) and torch.equal(top[2] + bottom[2], img1[2])   # zero outside a band
    # ... and band by band: sums and hits add, maxima combine by max
    h1, h2 = BlendStats(n, DEV), BlendStats(n, DEV)
    h1.add(_settings(frame, tile_rows=(0, 7)), **t)
    h2.add(_settings(frame, tile_rows=(7, rows)), **t)
    H1, H2 = _tables(h1), _tables(h2)
    np.testing.assert_array_equal(H1["q"] + H2["q"], A["q"])
    np.testing.assert_array_equal(H1["hits"] + H2["hits"], A["hits"])
    np.testing.assert_array_equal(np.maximum(H1["max"], H2["max"]), A["max"])
    # a second, different view
    b = BlendStats(n, DEV)
    b.add(_settings(frame_b), **t)
    B = _tables(b)
    assert (B["hits"] != A["hits"]).any()
    a1.add(_settings(frame_b), **t)
    AB = _tables(a1)
    assert a1.num_views == 2 and set(np.unique(AB["views"])) <= {0, 1, 2}
    np.testing.assert_array_equal(AB["views"], (A["hits"] > 0).astype(np.int32) + (B["hits"] > 0))
    np.testing.assert_array_equal(AB["q"], A["q"] + B["q"])
    np.testing.assert_array_equal(AB["hits"], A["hits"] + B["hits"])
    np.testing.assert_array_equal(AB["max"], np.maximum(A["max"], B["max"]))
    a1.reset()
    Z = _tables(a1)
    assert a1.num_views == 0 and not any(Z[k].any() for k in Z)


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------
def test_edges_empty_scene_behind_camera_zero_mask():
    from sfgs.importance import BlendStats
    from sfgs.synth import scene
    W, H, n = 64, 40, 500
    frame, g = scene(n, W, H, seed=3, zrange=(4., 8.), scale_range=(0.05, 0.3))
    t = _inputs(g)
    empty = {k: (None if v is None else v[:0]) for k, v in t.items()}
    s0 = BlendStats(0, DEV)
    color, depth, alpha = s0.add(_settings(frame), **empty)
    torch.cuda.synchronize()
    assert s0.num_views == 1 and s0.hits.numel() == 0 and s0.weight_sum.numel() == 0 and not alpha.any()
    assert s0.keep_mask(min_hits=1).numel() == 0
    behind = dict(t, means3D=t["means3D"] * torch.tensor([1.0, 1.0, -1.0], device=DEV))
    sb = BlendStats(n, DEV)
    _, _, alpha = sb.add(_settings(frame), **behind)
    Z = _tables(sb)
    assert not any(Z[k].any() for k in Z) and not alpha.any() and sb.num_views == 1
    s = BlendStats(n, DEV)
    img = s.add(_settings(frame), **t)
    before = _tables(s)
    assert before["hits"].sum() > 0
    masked = s.add(_settings(frame), pixel_mask=torch.zeros(H, W, dtype=torch.uint8, device=DEV), **t)
    _same(before, _tables(s))                      # nothing counted; the masked pixels still composite
    assert s.num_views == 2 and torch.equal(torch.nan_to_num(img[0]), torch.nan_to_num(masked[0]))
    ones = BlendStats(n, DEV)
    ones.add(_settings(frame), pixel_mask=torch.ones(1, H, W, dtype=torch.bool, device=DEV), **t)
    _same(before, _tables(ones))
    with pytest.raises(ValueError, match="set up for"):
        BlendStats(n + 1, DEV).add(_settings(frame), **t)


def test_a_9_by_5_image():
    """One ragged tile in each direction. K is measured on this very scene, between references (the restatement under the
    oracle's exponential jitter against the plain one), as importance_np does for its cases."""
    from oracle import oracle as orc
    from sfgs.importance import BlendStats
    from sfgs.synth import scene
    frame, g = scene(60, 9, 5, seed=1, zrange=(4., 8.), scale_range=(0.05, 0.4))
    R = orc.OracleRender(frame, **g)
    keep = ~gb.pixel_mask(R)
    w = inp.walk(R, None, keep)
    j = inp.walk(R, None, keep, exp_jitter=2)
    np.testing.assert_array_equal(w["hits"], j["hits"])
    assert w["hits"].sum() > 45
    K = gb.choose_k(max(inp.in_units(j["sum"], w["sum"], w["unit_sum"]).max(),
                        inp.in_units(j["max"], w["max"], w["unit_max"]).max(), 1.0))
    s = BlendStats(60, DEV)
    s.add(_settings(frame), pixel_mask=torch.from_numpy(keep).to(DEV), **_inputs(g))
    _check_against_reference(f"9x5 (K = {K:g})", _tables(s), w, w["sum"], K * gb.EPS * w["unit_sum"] + w["hits"] * 2.0 ** -32,
                             K * gb.EPS * w["unit_max"])


# ---- 5. pruning ------------------------------------------------------------------------------------------------------------
def test_thresholds_tables_and_recording():
    from diff_gauss import GaussianRasterizer
    from sfgs import importance
    from sfgs.synth import scene
    W, H, n = 160, 96, 2000
    frame, g = scene(n, W, H, seed=11, zrange=(4., 8.), scale_range=(0.01, 0.2), xy_fill=1.4)   # a third outside the frustum
    t = _inputs(g)
    settings = _settings(frame)
    s = importance.BlendStats(n, DEV)
    s.add(settings, **t)
    T = _tables(s)
    assert 0 < (T["hits"] > 0).sum() < n
    for kw, want in ((dict(), np.ones(n, bool)),
                     (dict(min_hits=1), T["hits"] >= 1),
                     (dict(min_weight_max=0.05), T["max"] >= np.float32(0.05)),
                     (dict(min_weight_sum=0.5), T["sum"] >= 0.5),
                     (dict(min_views=1), T["views"] >= 1),
                     (dict(min_weight_max=0.05, min_hits=20), (T["max"] >= np.float32(0.05)) & (T["hits"] >= 20))):
        keep = s.keep_mask(**kw)
        assert keep.dtype == torch.bool and keep.device.type == "cuda"
        np.testing.assert_array_equal(keep.cpu().numpy(), want & ((T["hits"] > 0) | (not kw)), err_msg=str(kw))
    rows = np.zeros(n, dtype=[("x", "f4"), ("opacity", "f4")])
    rows["x"] = np.arange(n)
    keep = s.keep_mask(min_hits=1)
    np.testing.assert_array_equal(importance.prune_table(rows, keep)["x"], np.nonzero(T["hits"] > 0)[0].astype(np.float32))

    class Model:
        def __init__(self):
            self._xyz = t["means3D"]

        def prune_points(self, mask):
            self._xyz = self._xyz[~mask]
    m = Model()
    assert importance.prune(m, s, min_hits=1) == int((T["hits"] == 0).sum()) and m._xyz.shape[0] == int((T["hits"] > 0).sum())

    # recording(): a direct rasterizer call feeds the statistics, and is itself unchanged
    rec = importance.BlendStats(n, DEV)
    raster = GaussianRasterizer(settings)
    kw = dict(means3D=t["means3D"], means2D=None, colors_precomp=t["colors_precomp"], opacities=t["opacities"],
              scales=t["scales"], rotations=t["rotations"])
    plain = raster(**kw)
    with importance.recording(rec):
        wrapped = raster(**kw)
    after = raster(**kw)
    _same(T, _tables(rec))
    assert rec.num_views == 1
    for x, y, z in zip(plain[:5], wrapped[:5], after[:5]):
        assert torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(z))
    _same(T, _tables(rec))                         # the call after the context added nothing
    masked = importance.BlendStats(n, DEV)
    half = torch.zeros(H, W, dtype=torch.bool, device=DEV)
    half[:, : W // 2] = True
    with importance.recording(masked, pixel_mask=half):
        raster(**kw)
    direct = importance.BlendStats(n, DEV)
    direct.add(settings, pixel_mask=half, **t)
    _same(_tables(direct), _tables(masked))
    assert 0 < _tables(masked)["hits"].sum() < T["hits"].sum()
