"""tests/model_ops_ref.py pinned on the CPU, before anything on a GPU relies on it: the float64 references against the
goldens of the REAL reference project and against the oracles, the K table against a second seed, and the CPU half of the
GPU tests' conditions (what the generated inputs contain, on which side of each threshold the filter3d probes lie)."""
import os

import numpy as np
import pytest
import torch

import model_ops_ref as R
from oracle.adam_np import adam_step
from oracle.filter3d_np import compute_3D_filter as oracle_filter
from oracle.prepass_torch import prepass_reference

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLD, "reference_helpers.npz"))
SHG = np.load(os.path.join(GOLD, "reference_sh_grad.npz"))
SH4 = np.load(os.path.join(GOLD, "reference_sh4.npz"))


def _golden_prepass(tag):
    g = lambda k: G[f"prepass_{tag}_{k}"]
    return dict(scaling=g("scaling"), opacity=g("opacity"), rotation=g("rotation"), filt=g("filter"),
                g_scales=g("w_scales"), g_opacity=g("w_opacity"), g_rotation=g("w_rotation"))


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_prepass_reference_matches_the_real_getters(tag):
    x = _golden_prepass(tag)
    ref, unit = R.prepass_ref(**x)
    for k, key in (("scales", "out_scales"), ("opacity", "out_opacity"), ("rotation", "out_rotation")):
        e = R.worst(G[f"prepass_{tag}_{key}"], ref[k], unit[k])
        assert e <= R.k_of("prepass", k), (k, e)
    for k, key in (("g_scaling", "g_scaling"), ("g_opacity", "g_opacity"), ("g_rotation", "g_rotation")):
        want = G[f"prepass_{tag}_{key}"]
        assert np.abs(ref[k] - want).max() <= 1e-6 * np.abs(want).max(), k      # test_prepass.py's tolerance


@pytest.mark.parametrize("route", range(4))
def test_prepass_reference_matches_the_torch_oracle_on_the_wide_inputs(route):
    ft, ot = R.ROUTES[route]
    x = R.prepass_inputs(4099, 3, ft, ot)
    ref, unit = R.prepass_ref(**x)
    got = prepass_reference(*(torch.tensor(x[k]) for k in ("scaling", "opacity", "rotation", "filt")))
    for k, t in zip(("scales", "opacity", "rotation"), got):
        e = R.worst(t.numpy(), ref[k], unit[k])
        print(f"prepass_torch route {route} {k}: {e:.3g} units")
        assert e <= R.k_of("prepass", k), (k, e)


def test_prepass_absent_upstream_gradients_give_exact_zeros():
    x = R.prepass_inputs(257, 4)
    only_o = R.prepass_ref(x["scaling"], x["opacity"], x["rotation"], x["filt"], g_opacity=x["g_opacity"])[0]
    assert not only_o["g_rotation"].any() and only_o["g_scaling"].any() and only_o["g_opacity"].any()
    only_s = R.prepass_ref(x["scaling"], x["opacity"], x["rotation"], x["filt"], g_scales=x["g_scales"])[0]
    assert not only_s["g_rotation"].any() and not only_s["g_opacity"].any() and only_s["g_scaling"].any()
    only_r = R.prepass_ref(x["scaling"], x["opacity"], x["rotation"], x["filt"], g_rotation=x["g_rotation"])[0]
    assert not only_r["g_scaling"].any() and not only_r["g_opacity"].any() and only_r["g_rotation"].any()


def test_prepass_rotation_gradient_matches_autograd_through_normalize():
    """the closed form of F.normalize's gradient, clamp included, against torch autograd in float64"""
    q = torch.tensor(R.quaternion_cases(), dtype=torch.float64, requires_grad=True)
    g = torch.tensor(R.prepass_inputs(q.shape[0], 5)["g_rotation"], dtype=torch.float64)
    (torch.nn.functional.normalize(q, eps=R.NORM_EPS) * g).sum().backward()
    n = q.shape[0]
    z = np.zeros((n, 3), np.float32)
    ref, unit = R.prepass_ref(z, np.zeros((n, 1), np.float32), R.quaternion_cases(), np.ones((n, 1)), g_rotation=g.numpy())
    assert R.worst(q.grad.numpy(), ref["g_rotation"], unit["g_rotation"], R.EPS64) <= 16


@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_eval_sh_reference_matches_the_real_eval_sh(deg):
    z = {k: SH4[k] for k in SH4.files} if deg == 4 else {k[5:]: SHG[k] for k in SHG.files if k.startswith(f"shg{deg}_")}
    ref, unit = R.eval_sh_ref(deg, z["sh"], z["dirs"], z["w"])
    for k in R.SH_TENSORS:
        e = R.worst(z[k], ref[k], unit[k])
        assert e <= R.k_of("eval_sh", k), (k, e)
    m = (deg + 1) ** 2
    assert not ref["g_sh"][:, :, m:].any() and not z["g_sh"][:, :, m:].any()


def test_sh_magnitudes_bound_the_basis():
    d = R.sh_inputs(500, 25, 9, unit_dirs=False)["dirs"]
    B, dB = R.sh_basis(4, d)
    Bm, dBm = R.sh_basis(4, d, magnitude=True)
    assert (np.abs(B) <= Bm * (1 + 1e-12)).all() and (np.abs(dB) <= dBm * (1 + 1e-12)).all()
    h = 1e-6
    for w in range(3):     # the derivative table against central differences of the value table
        dp, dm = d.astype(np.float64).copy(), d.astype(np.float64).copy()
        dp[:, w] += h
        dm[:, w] -= h
        num = (R.sh_basis(4, dp)[0] - R.sh_basis(4, dm)[0]) / (2 * h)
        assert np.abs(num - dB[:, :, w]).max() <= 1e-6 * max(1.0, np.abs(dB).max())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_adam_reference_matches_adam_step(dtype):
    eps = R.EPS32 if dtype is np.float32 else R.EPS64
    for i, t in enumerate(R.ADAM_STEPS):
        h = R.adam_hyper(i + 1, t)
        p, g, m, v = R.adam_inputs(4097, 20 + i, dtype, zeros=2 if h["weight_decay"] == 0 else 0)
        ref, unit = R.adam_ref(p, g, m, v, **h)
        if dtype is np.float32:
            got = adam_step(p.copy(), g, m.copy(), v.copy(), t, h["lr"], eps=h["eps"], weight_decay=h["weight_decay"])
        else:
            got = R.adam_f64(p, g, m, v, t, h["lr"], eps=h["eps"], weight_decay=h["weight_decay"])
        for k, a in zip(R.ADAM_TENSORS, got):
            e = R.in_units_ld(a, ref[k], unit[k], eps).max()
            assert e <= R.k_of("adam", k), (k, t, e)
        if h["weight_decay"] == 0:     # g = m = v = 0: the parameter stays, bit for bit
            assert (got[0][:2] == p[:2]).all() and (ref["p"][:2] == p[:2]).all()


def test_adam_reference_matches_torch_adam():
    """the long double step against torch.optim.Adam itself (CPU, float64), from an injected state"""
    h = R.adam_hyper(4, 10)
    p, g, m, v = R.adam_inputs(1000, 31, np.float64)
    ref, unit = R.adam_ref(p, g, m, v, **h)
    tp = torch.nn.Parameter(torch.tensor(p))
    tp.grad = torch.tensor(g)
    opt = torch.optim.Adam([tp], lr=h["lr"], eps=h["eps"], weight_decay=h["weight_decay"])
    opt.state[tp] = dict(step=torch.tensor(float(h["t"] - 1)), exp_avg=torch.tensor(m), exp_avg_sq=torch.tensor(v))
    opt.step()
    st = opt.state[tp]
    assert float(st["step"]) == h["t"]
    for k, a in (("p", tp.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
        assert R.in_units_ld(a.numpy(), ref[k], unit[k], R.EPS64).max() <= R.k_of("adam", k), k


def test_densify_stats_reference_matches_the_golden():
    n = G["dstats_denom"].shape[0]
    bufs = {k: np.zeros((n, 1), np.float32) for k in R.STATS}
    for step in range(2):
        ref = R.densify_stats_ref(bufs, G[f"dstats_grad{step}"], G[f"dstats_filter{step}"])
        bufs = {k: v.astype(np.float32) for k, v in ref.items()}      # the buffers are float32 between the calls
    for k in R.STATS:
        assert (np.abs(bufs[k] - G["dstats_" + k]) <= 2 * R.ulp32(G["dstats_" + k])).all(), k
    no_max = R.densify_stats_ref({k: v for k, v in bufs.items() if k != "xyz_gradient_accum_abs_max"}, G["dstats_grad0"],
                                 G["dstats_filter0"])
    assert "xyz_gradient_accum_abs_max" not in no_max


def test_k_table_is_what_the_module_measures_and_covers_a_second_seed():
    """K = 4 x the committed maximum, as a power of two; the committed maxima are what this host measures (to 5 %: numpy's
    vectorised expf is not the same on every CPU); a second seed's maxima leave the kernels the same factor-two share of K
    at least (a factor of two of the four is what the device's own rounding gets in the worst case)."""
    first, second = R.measured_table(R.MEASURE_SEED), R.measured_table(R.SECOND_SEED)
    for op, rows in R.K_TABLE.items():
        for k, row in rows.items():
            print(op, k, "committed", row, "measured", first[op][k], "second seed", second[op][k])
            assert row[-1] == R.choose_k(max(row[:-1]))
            assert len(first[op][k]) == len(row)
            assert all(a <= 1.05 * b and b <= 1.05 * a for a, b in zip(first[op][k][:-1], row[:-1])), (op, k, first[op][k])
            assert 2 * max(second[op][k][:-1]) <= row[-1], (op, k, second[op][k])


def test_generated_prepass_inputs_are_what_the_gpu_tests_assume():
    for n in R.BLOCK_NS + (R.MEASURE_N,):
        for ft, ot in R.ROUTES:
            x = R.prepass_inputs(n, R.MEASURE_SEED, ft, ot)
            assert x["filt"].dtype == ft and x["opacity"].dtype == ot
            assert all(np.isfinite(v).all() for v in x.values())
            d1 = R.det1_f32(x["scaling"])
            assert d1.dtype == np.float32 and (d1 >= R.F32_TINY).all() and np.isfinite(d1).all()     # no denormal det1
            ref, unit = R.prepass_ref(**x)
            assert all(np.isfinite(v).all() for v in ref.values()) and all(np.isfinite(v).all() for v in unit.values())
            assert (ref["scales"].astype(np.float32) < np.inf).all()


def test_quaternion_cases_are_as_intended():
    q = R.quaternion_cases()
    assert q.dtype == np.float32
    n = np.linalg.norm(q.astype(np.float64), axis=1)
    assert (q[0] == 0).all() and n[0] == 0                                     # exact zero
    assert ((n[1:5] > 0.5e-13) & (n[1:5] < 2e-13)).all()                       # below the clamp of 1e-12
    assert not ((n > 1e-12 * 0.5) & (n < 1e-12 * 2)).any()                     # nothing NEAR the clamp: no ambiguous side
    assert n[5:30].min() < 1.1e-3 and n[5:30].max() > 0.9e3
    dom = np.abs(q[30:]).max(axis=1) / np.maximum(np.sort(np.abs(q[30:]), axis=1)[:, -2], 1e-30)
    assert dom.shape[0] == 12 and (dom > 1e3).all()
    sq = (q.astype(np.float32) ** 2).sum(axis=1)
    assert ((sq == 0) | (sq >= R.F32_TINY)).all()                              # |q|^2 is never denormal in float32
    assert (R.prepass_inputs(4099, 1)["rotation"][:q.shape[0]] == q).all()
    assert (R.prepass_inputs(1, 1)["rotation"] == q[:1]).all()


@pytest.mark.parametrize("test", R.FILTER_TESTS)
@pytest.mark.parametrize("inside", [True, False])
def test_filter3d_probes_lie_on_the_intended_side(test, inside):
    xyz, cams, seen = R.filter3d_threshold_case(test, inside)
    m = R.filter3d_margins(xyz, cams[0])
    j = R.FILTER_TESTS.index(test)
    assert (m[1] > 0.01).all()                                          # the anchor passes every test by far
    assert (np.delete(m[0], j) > 0.01).all()                            # the probe passes the four other tests by far
    assert (m[0, j] >= 1e-9) if inside else (m[0, j] <= -1e-9)
    assert abs(m[0, j]) <= 2e-9
    out = oracle_filter(xyz, cams)[:, 0]
    anchor = (50.0 + cams[0]["T"][2]) / cams[0]["focal_x"] * R.SQRT02
    assert out[1] == anchor
    assert (out[0] < anchor) if inside else (out[0] == anchor)          # unseen: takes the largest seen distance


@pytest.mark.parametrize("last", [True, False])
def test_filter3d_reduce_case_has_its_maximum_where_intended(last):
    xyz, cams, far = R.filter3d_reduce_case(last)
    n = xyz.shape[0]
    assert n == 262_444 and (n + 255) // 256 == 1026
    assert far // 256 == (1025 if last else 0)
    out = oracle_filter(xyz, cams)[:, 0]
    unseen = np.zeros(n, bool)
    unseen[::41] = True
    assert not unseen[far]
    assert (out[unseen] == out[far]).all() and out[far] == out.max()
    assert (np.delete(out, np.r_[np.flatnonzero(unseen), far]) < 0.5 * out[far]).all()
    assert unseen[1025 * 256:].any() and unseen[:256].any()


def _share_noticed(ref, unit, k, eps=R.EPS32):
    """of the elements with a non-zero reference value, the share whose bound a zero in their place would violate"""
    L = np.longdouble
    ref, unit = np.abs(np.asarray(ref).astype(L)).ravel(), np.asarray(unit).astype(L).ravel()
    nz = ref > 0
    return float((ref[nz] > k * L(eps) * unit[nz]).mean())


def test_the_bounds_notice_a_dropped_element():
    """What the whole-tensor tolerances could not see: an element that is simply zero (a skipped row, a wrong table entry)
    violates its own bound for more than 99.8 % of the elements of every tensor, on the GPU tests' inputs."""
    x = R.prepass_inputs(R.MEASURE_N, 7, np.float64, np.float64)
    ref, unit = R.prepass_ref(**x)
    for k in R.PREPASS_TENSORS:
        assert _share_noticed(ref[k], unit[k], R.k_of("prepass", k)) > 0.998, k
    whole = 2e-6 * np.abs(ref["g_scaling"]).max()              # test_prepass.py's tolerance on the same tensor
    assert (np.abs(ref["g_scaling"]) <= whole).mean() > 0.2    # ... lets a fifth of these gradients be 100 % wrong
    for unit_dirs in (True, False):
        y = R.sh_inputs(4099, 25, 7, unit_dirs)
        ref, unit = R.eval_sh_ref(4, **y)
        for k in R.SH_TENSORS:
            assert _share_noticed(ref[k], unit[k], R.k_of("eval_sh", k)) > 0.998, k
    for dt, eps in ((np.float32, R.EPS32), (np.float64, R.EPS64)):
        p, g, m, v = R.adam_inputs(8193, 7, dt)
        h = R.adam_hyper(2, 1000)
        ref, unit = R.adam_ref(p, g, m, v, **h)
        for k in R.ADAM_TENSORS:
            assert _share_noticed(ref[k], unit[k], R.k_of("adam", k), eps) > 0.998, k


def test_the_adam_bound_notices_another_tensors_scalars():
    """every tensor of the multi-tensor cases has its own lr, weight_decay and step: a step computed with a neighbour's
    scalars (a block that read another table entry) leaves the bound"""
    for i in range(50):
        h = R.adam_hyper(i)
        p, g, m, v = R.adam_inputs(4097, 500 + i, np.float32)
        ref, unit = R.adam_ref(p, g, m, v, **h)
        for j in (i - 1, i + 1, (i + 24) % 50, (i + 48) % 50):
            o = R.adam_hyper(j % 50)
            assert (o["lr"], o["weight_decay"], o["t"]) != (h["lr"], h["weight_decay"], h["t"])
            got = adam_step(p.copy(), g, m.copy(), v.copy(), o["t"], o["lr"], eps=o["eps"], weight_decay=o["weight_decay"])
            e = max(R.in_units_ld(a, ref[k], unit[k], R.EPS32).max() / R.k_of("adam", k) for k, a in zip(R.ADAM_TENSORS, got))
            assert e > 10, (i, j, e)
