"""sfgs.transform on the GPU: the kernel (csrc/transform.hip) against the float64 restatement of tests/transform_np.py fed with
the same float32-rounded constants, at sizes on both sides of its 256-row block; identity and round trip; render invariance
on the HIP path; merge_fused_plys(transforms=...) end to end; transform_model.

The bound: every output component lies within 8 * 2^-24 * sum |term_i| of the float64 value -- the standard bound of a
float32 dot product of at most 7 terms summed in index order, plus the final product / add -- with the sum of absolute terms
taken from the restatement. Log-scales and filter_3D are one float32 operation: bit for bit numpy's."""
import functools
import types

import numpy as np
import pytest
import torch

import parity
import transform_np as tnp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK = 256                                  # csrc/transform.hip: TF_BLOCK
SIZES = (1, BLOCK + 1, 70001)                # one lane; one past a block; many blocks and a ragged tail (70001 = 273 * 256 + 113)
GUARD = 3                                    # rows of sentinel around every tensor: a stray write shows


def _sim():
    return tnp.render_similarity()           # a general rotation, s = 0.37, t = (100, -50, 20)


@functools.lru_cache(maxsize=None)
def _inputs(N, kr, layout):
    """float32 numpy inputs of one size, fixed by (N, kr, layout); never modified."""
    rng = np.random.default_rng(1000 * kr + N + (7 if layout == "n3k" else 0))
    rest_shape = (N, kr, 3) if layout == "nk3" else (N, 3, kr)
    d = dict(xyz=rng.normal(size=(N, 3)) * 100.0, scaling=rng.normal(size=(N, 3)) - 1.0, rotation=rng.normal(size=(N, 4)),
             features_rest=rng.normal(size=rest_shape) * 0.3, filter_3D=rng.uniform(0.01, 2.0, size=(N, 1)))
    d = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in d.items()}
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _expected(N, kr, layout):
    """The restatement with the float32-rounded constants: name -> (float64 value, sum of absolute terms). Computed once per
    (N, kr, layout) and shared."""
    c, d = tnp.constants(_sim(), np.float32), _inputs(N, kr, layout)
    return dict(xyz=tnp.xyz(c, d["xyz"]), scaling_log=tnp.scaling(c, d["scaling"], True),
                scaling_act=tnp.scaling(c, np.exp(d["scaling"]), False), rotation=tnp.rotation(c, d["rotation"]),
                features_rest=tnp.features_rest(c, d["features_rest"], layout), filter_3D=tnp.filter_3d(c, d["filter_3D"]))


def _guarded(a, shift):
    """`a` on the device as a contiguous view into a larger buffer of sentinels; shift = 1 also moves its start off a 16-byte
    boundary by another row. -> (view, buffer, first row of the view in the buffer)."""
    row = a.shape[1:]
    buf = torch.full((a.shape[0] + 2 * GUARD,) + row, -77.0, dtype=torch.float32, device=DEV)
    lo = GUARD - shift
    view = buf[lo:lo + a.shape[0]]
    view.copy_(torch.tensor(a))
    return view, buf, lo


def _within(name, got, want):
    value, abs_sum = want
    err = np.abs(got.astype(np.float64) - value)
    bound = tnp.BOUND_FACTOR * abs_sum
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} components outside the bound, worst {worst:.3f} x bound"
    return worst


# (K - 1, rest layout, log scales, in place, names passed)
ALL = ("xyz", "scaling", "rotation", "features_rest", "filter_3D")
CONFIGS = [
    (15, "nk3", True, False, ALL), (15, "nk3", True, True, ALL), (15, "n3k", True, False, ALL), (15, "n3k", False, True, ALL),
    (8, "nk3", False, False, ALL), (8, "n3k", True, True, ALL), (3, "nk3", True, True, ALL), (3, "n3k", False, False, ALL),
    (0, "nk3", True, False, ALL), (0, "n3k", False, True, ALL),
    # each optional tensor absent, and each alone
    (15, "nk3", True, False, ("scaling", "rotation", "features_rest", "filter_3D")),
    (15, "nk3", False, True, ("xyz", "rotation", "features_rest", "filter_3D")),
    (15, "n3k", True, False, ("xyz", "scaling", "features_rest", "filter_3D")),
    (15, "nk3", True, True, ("xyz", "scaling", "rotation", "filter_3D")),
    (8, "nk3", True, False, ("xyz", "scaling", "rotation", "features_rest")),
    (15, "nk3", True, False, ("xyz",)), (3, "n3k", True, True, ("features_rest",)), (0, "nk3", True, False, ("rotation",)),
    (0, "nk3", False, True, ("scaling",)), (0, "nk3", True, False, ("filter_3D",)),
]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kr,layout,is_log,inplace,names", CONFIGS,
                         ids=[f"k{c[0]}-{c[1]}-{'log' if c[2] else 'act'}-{'in' if c[3] else 'out'}-{'+'.join(n[:3] for n in c[4])}"
                              for c in CONFIGS])
def test_kernel_against_the_restatement(N, kr, layout, is_log, inplace, names):
    from sfgs import transform as T
    sim, d, want = _sim(), _inputs(N, kr, layout), _expected(N, kr, layout)
    host = {k: (np.exp(v) if k == "scaling" and not is_log else v) for k, v in d.items()}
    held = {k: _guarded(host[k], shift=1 if inplace else 0) for k in names}
    given = {k: (held[k][0] if k in held else None) for k in ALL}
    out = T.transform_gaussians(sim, given["xyz"], given["scaling"], given["rotation"], given["features_rest"],
                                given["filter_3D"], scaling_is_log=is_log, rest_layout=layout, inplace=inplace)
    torch.cuda.synchronize()
    out = dict(zip(ALL, out))
    c32 = tnp.constants(sim, np.float32)
    worst = {}
    for k in ALL:
        if k not in names:
            assert out[k] is None
            continue
        view, buf, lo = held[k]
        if inplace:
            assert out[k] is view
        else:
            assert out[k] is not view and out[k].shape == view.shape
            np.testing.assert_array_equal(view.cpu().numpy(), host[k])        # the input is left alone
        # nothing outside the tensor was written
        assert bool((buf[:lo] == -77.0).all()) and bool((buf[lo + N:] == -77.0).all()), k
        got = out[k].cpu().numpy()
        if k == "scaling":
            worst[k] = _within(k, got, want["scaling_log" if is_log else "scaling_act"])
            one = host[k] + np.float32(c32["log_s"]) if is_log else host[k] * np.float32(c32["s"])
            assert one.dtype == np.float32
            np.testing.assert_array_equal(got.view(np.uint32), one.view(np.uint32))
        elif k == "filter_3D":
            worst[k] = _within(k, got, want[k])
            np.testing.assert_array_equal(got.view(np.uint32), (host[k] * np.float32(c32["s"])).view(np.uint32))
        elif k == "features_rest" and kr == 0:
            assert got.size == 0
        else:
            worst[k] = _within(k, got, want[k])
    print(N, kr, layout, {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("layout", ["nk3", "n3k"])
def test_identity_changes_no_bit_and_round_trip_returns_the_input(N, layout):
    """sim then sim.inverse(): within twice the bound, with the sum of absolute terms of the second step (the larger one:
    (x' - t) / s cancels the translation) taken from the restatement of both steps."""
    from sfgs import transform as T
    d = _inputs(N, 15, layout)
    dev = {k: torch.tensor(v, device=DEV) for k, v in d.items()}
    args = lambda t: (t["xyz"], t["scaling"], t["rotation"], t["features_rest"], t["filter_3D"])
    same = T.transform_gaussians(T.Similarity.identity(), *args(dev), rest_layout=layout)
    for k, t in zip(ALL, same):
        assert t is not dev[k]
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), d[k].view(np.uint32), err_msg=k)
    sim = _sim()
    there = dict(zip(ALL, T.transform_gaussians(sim, *args(dev), rest_layout=layout)))
    back = dict(zip(ALL, T.transform_gaussians(sim.inverse(), *args(there), rest_layout=layout)))
    c1, c2 = tnp.constants(sim, np.float32), tnp.constants(sim.inverse(), np.float32)
    steps = dict(xyz=lambda c, v: tnp.xyz(c, v), scaling=lambda c, v: tnp.scaling(c, v, True),
                 rotation=lambda c, v: tnp.rotation(c, v), features_rest=lambda c, v: tnp.features_rest(c, v, layout),
                 filter_3D=lambda c, v: tnp.filter_3d(c, v))
    for k in ALL:
        _, abs_sum = steps[k](c2, steps[k](c1, d[k])[0])
        err = np.abs(back[k].cpu().numpy().astype(np.float64) - d[k])
        assert (err <= 2 * tnp.BOUND_FACTOR * abs_sum).all(), (k, float((err / (tnp.BOUND_FACTOR * abs_sum)).max()))
        assert float(err.max()) > 0 or k == "filter_3D" or N == 1           # a real round trip, not two no-ops


# ---- render invariance on the HIP path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(tnp.RENDER_FORMS))
def test_render_invariance_on_the_hip_path(form):
    from sfgs import transform as T
    from test_gpu_raster import run_hip
    sim = _sim()
    frame, g, R, Tc = tnp.render_case(form)
    want = run_hip(frame, g, backward=False)
    assert int((want["radii"] > 0).sum()) == tnp.RENDER_N and int((want["alpha"] > 0.01).sum()) > 500   # every splat on screen
    rest = None if g["shs"] is None else g["shs"][:, 1:].contiguous().to(DEV)
    xyz, scales, rots, rest, _ = T.transform_gaussians(sim, g["means3D"].to(DEV), g["scales"].to(DEV), g["rotations"].to(DEV),
                                                       rest, None, scaling_is_log=False, rest_layout="nk3")
    moved = dict(g, means3D=xyz.cpu(), scales=scales.cpu(), rotations=rots.cpu())
    if rest is not None:
        moved["shs"] = torch.cat([g["shs"][:, :1], rest.cpu()], 1).contiguous()
    got = run_hip(tnp.moved_frame(frame, *T.transform_camera(R, Tc, sim)), moved, backward=False)
    reps = [parity.assert_image_close("color", got["color"], want["color"], rtol=parity.RGB_DEPTH_RTOL),
            parity.assert_image_close("alpha", got["alpha"], want["alpha"], rtol=parity.RGB_DEPTH_RTOL),
            parity.assert_image_close("depth", got["depth"] / np.float32(sim.s), want["depth"], rtol=parity.RGB_DEPTH_RTOL)]
    print(form, reps)
    # a ceil on a boundary can flip after the float32 transform: by 1, on at most 2 of the 3000 (the oracle pair has none)
    diff = np.abs(got["radii"].astype(np.int64) - want["radii"].astype(np.int64))
    assert diff.max() <= 1 and int((diff > 0).sum()) <= 2, (int(diff.max()), int((diff > 0).sum()))


# ---- merge_fused_plys(transforms=...) ------------------------------------------------------------------------------------------
MW, MH = 160, 96


def _scene_model(seed, n):
    """A model as save_fused_ply reads it (tests/test_gpu_joint_render.py writes its own the same way), SH degree 3."""
    g = torch.Generator().manual_seed(seed)
    m = types.SimpleNamespace(appearance_enabled=False, max_sh_degree=3)
    m._xyz = torch.randn(n, 3, generator=g) * torch.tensor([6.0, 4.0, 3.0])
    m._features_dc = torch.randn(n, 1, 3, generator=g)
    m._features_rest = torch.randn(n, 15, 3, generator=g) * 0.3
    m._opacity = torch.randn(n, 1, generator=g)
    m._scaling = torch.log(torch.rand(n, 3, generator=g) * 0.25 + 0.02)
    m._rotation = torch.randn(n, 4, generator=g)
    m.get_opacity_with_3D_filter = torch.sigmoid(m._opacity)
    m.get_scaling_with_3D_filter = torch.exp(m._scaling)
    return m


def _render(xyz, f_dc, f_rest_nk3, opacity, scaling, rotation):
    """float32 tensors as load_standard_ply leaves them -> (color, alpha, depth) numpy, camera at the origin looking down +z."""
    import math
    from diff_gauss import GaussianRasterizationSettings, GaussianRasterizer
    from sfgs.camera import fovy_from_fovx, make_frame
    fovx = math.radians(60.0)
    frame = make_frame(np.eye(3), np.zeros(3), fovx, fovy_from_fovx(fovx, MW, MH), MW, MH, kernel_size=0.1, sh_degree=3)
    settings = GaussianRasterizationSettings(MH, MW, frame["tanfovx"], frame["tanfovy"], 0.1, None, frame["bg"].to(DEV), 1.0,
                                             frame["view"].to(DEV), frame["proj"].to(DEV), 3, frame["campos"].to(DEV),
                                             False, False)
    with torch.no_grad():
        color, depth, _, alpha, radii, _ = GaussianRasterizer(settings)(
            means3D=xyz, means2D=None, opacities=torch.sigmoid(opacity), shs=torch.cat([f_dc, f_rest_nk3], 1).contiguous(),
            scales=torch.exp(scaling), rotations=torch.nn.functional.normalize(rotation))
    assert int((radii > 0).sum()) > 0.5 * len(xyz) and float(alpha.mean()) > 0.01    # not an empty frame
    return color.cpu().numpy(), alpha.cpu().numpy(), depth.cpu().numpy()


def test_merge_with_transforms_renders_like_the_restatement(tmp_path):
    from sfgs import ply
    from sfgs import transform as T
    sims = [T.Similarity(tnp.quat_to_matrix(np.random.default_rng(21).normal(size=4)), 0.8, (-7.0, 0.5, 40.0)),
            T.Similarity(tnp.quat_to_matrix(np.random.default_rng(22).normal(size=4)), 1.3, (8.0, -1.0, 48.0))]
    paths = []
    for i, n in enumerate((1500, 1901)):
        paths.append(str(tmp_path / f"scene{i}.ply"))
        ply.save_fused_ply(_scene_model(30 + i, n), paths[-1])
    out = str(tmp_path / "joint.ply")
    merged = ply.merge_fused_plys(paths, transforms=sims, out_path=out, device=DEV)
    assert len(merged) == 3401 and merged.dtype.names == ply.read_ply(paths[0])[0][1].dtype.names
    model = types.SimpleNamespace(max_sh_degree=ply.detect_sh_degree(out))
    assert model.max_sh_degree == 3
    ply.load_standard_ply(model, out, device=DEV)
    got = _render(*(t.detach() for t in (model._xyz, model._features_dc, model._features_rest, model._opacity, model._scaling,
                                         model._rotation)))
    # the same two parts, each moved by the restatement (float32-rounded constants, float64 arithmetic), concatenated
    parts = []
    for p, sim in zip(paths, sims):
        part = types.SimpleNamespace(max_sh_degree=3)
        ply.load_standard_ply(part, p, device="cpu")
        c = tnp.constants(sim, np.float32)
        num = lambda t: t.detach().numpy()
        f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)
        parts.append((f32(tnp.xyz(c, num(part._xyz))[0]), part._features_dc.detach().to(DEV),
                      f32(tnp.features_rest(c, num(part._features_rest), "nk3")[0]), part._opacity.detach().to(DEV),
                      f32(tnp.scaling(c, num(part._scaling), True)[0]), f32(tnp.rotation(c, num(part._rotation))[0])))
    want = _render(*(torch.cat(ts, 0).contiguous() for ts in zip(*parts)))
    for name, a, b in zip(("color", "alpha", "depth"), got, want):
        print(parity.assert_image_close(name, a, b, rtol=parity.RGB_DEPTH_RTOL))
    # untouched columns are the files' bytes
    both = np.concatenate([ply.read_ply(p)[0][1] for p in paths])
    for name in ("nx", "f_dc_0", "f_dc_2", "opacity"):
        np.testing.assert_array_equal(merged[name].view(np.uint32), both[name].view(np.uint32))
    assert np.abs(merged["x"] - both["x"]).max() > 1 and np.abs(merged["f_rest_7"] - both["f_rest_7"]).max() > 0.01


def test_merge_with_identity_transforms_is_the_plain_merge_byte_for_byte(tmp_path):
    from sfgs import ply
    from sfgs import transform as T
    paths = []
    for i, n in enumerate((300, 557)):
        paths.append(str(tmp_path / f"scene{i}.ply"))
        ply.save_fused_ply(_scene_model(40 + i, n), paths[-1])
    plain = ply.merge_fused_plys(paths)
    same = ply.merge_fused_plys(paths, transforms=[T.Similarity.identity(), T.Similarity.identity()], device=DEV)
    assert same.dtype == plain.dtype and same.tobytes() == plain.tobytes()


# ---- transform_model -----------------------------------------------------------------------------------------------------------
def _model(n, filter_dtype):
    m = _scene_model(50, n)
    for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        setattr(m, name, torch.nn.Parameter(getattr(m, name).to(DEV).requires_grad_(True)))
    m.filter_3D = (torch.rand(n, 1, generator=torch.Generator().manual_seed(51)) + 0.01).to(DEV, filter_dtype)
    m._embeddings = torch.randn(n, 8, generator=torch.Generator().manual_seed(52)).to(DEV)
    m.optimizer = None
    return m


@pytest.mark.parametrize("filter_dtype", [torch.float32, torch.float64])
def test_transform_model_changes_the_parameters_as_transform_gaussians_says(filter_dtype):
    from sfgs import transform as T
    sim, n = _sim(), 777
    m = _model(n, filter_dtype)
    before = {k: getattr(m, k).detach().clone() for k in ("_xyz", "_scaling", "_rotation", "_features_rest", "filter_3D",
                                                          "_features_dc", "_opacity", "_embeddings")}
    params = {k: getattr(m, k) for k in ("_xyz", "_scaling", "_rotation", "_features_rest")}
    want = T.transform_gaussians(sim, before["_xyz"], before["_scaling"], before["_rotation"], before["_features_rest"],
                                 before["filter_3D"].float(), scaling_is_log=True, rest_layout="nk3")
    assert T.transform_model(m, sim) is m
    for k, w in zip(("_xyz", "_scaling", "_rotation", "_features_rest"), want):
        assert getattr(m, k) is params[k] and isinstance(getattr(m, k), torch.nn.Parameter) and getattr(m, k).requires_grad
        assert torch.equal(getattr(m, k).detach(), w) and not torch.equal(w, before[k]), k
    assert m.filter_3D.dtype == filter_dtype
    if filter_dtype == torch.float32:
        assert torch.equal(m.filter_3D, want[4])
    else:
        assert torch.equal(m.filter_3D, before["filter_3D"] * sim.s)
    for k in ("_features_dc", "_opacity", "_embeddings"):
        assert torch.equal(getattr(m, k).detach(), before[k]), k
    m.optimizer = torch.optim.Adam([m._xyz], lr=1e-3)
    with pytest.raises(ValueError, match="optimizer"):
        T.transform_model(m, sim)
    assert torch.equal(m._xyz.detach(), want[0])                           # and nothing was touched
