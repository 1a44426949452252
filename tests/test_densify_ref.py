"""tests/densify_ref.py (the plain CPU restatement of the whole densify_and_prune surgery, used as the reference by
tests/test_gpu_densify_edges.py) against the REAL method's outputs, tests/golden/reference_densify_full.npz; and the
input generator's guarantees: decision margins, populated levels, and that the 2e-6 bar of the computed child rows is
not tighter than float32 itself allows on the generated inputs."""
import json
import os

import numpy as np
import pytest
import torch

import densify_ref as DR
import densify_rule

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_densify_full.npz")
GOLD_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "embeddings")
SIZES = (0, 1, 255, 256, 257, 2049, 262144, 262145, 524289)


def test_surgery_reproduces_the_real_method():
    z = np.load(GOLD)
    cfg = json.loads(str(z["config"]))
    t = lambda k: torch.from_numpy(z[k])
    params = {n: t("in_" + n) for n in GOLD_GROUPS}
    moments = {n: (t("in_m_" + n), t("in_v_" + n)) for n in GOLD_GROUPS if "in_m_" + n in z.files}
    assert 0 < len(moments) < len(GOLD_GROUPS)
    out = DR.surgery(params, moments, t("in_xyz_gradient_accum"), t("in_xyz_gradient_accum_abs"), t("in_denom"),
                     torch.exp(params["scaling"]), torch.sigmoid(params["opacity"]), cfg["max_grad"], cfg["min_opacity"],
                     cfg["extent"], cfg["max_screen_size"], cfg["percent_dense"], t("samples"))
    assert tuple(out.ret) == tuple(int(v) for v in z["ret"])
    child = out.is_child.numpy()
    assert 0 < child.sum() < child.size
    checked = {"config", "samples", "ret"}
    for n in GOLD_GROUPS:
        got, ref = out.params[n].numpy(), z["out_" + n]
        assert got.shape == ref.shape and got.dtype == ref.dtype, n
        if n in ("xyz", "scaling"):
            np.testing.assert_array_equal(got[~child], ref[~child], err_msg=n)
            np.testing.assert_allclose(got[child], ref[child], rtol=DR.CHILD_RTOL, atol=DR.CHILD_ATOL, err_msg=n)
        else:
            np.testing.assert_array_equal(got, ref, err_msg=n)
        checked.add("out_" + n)
        if "out_m_" + n in z.files:
            np.testing.assert_array_equal(out.moments[n][0].numpy(), z["out_m_" + n], err_msg=n)
            np.testing.assert_array_equal(out.moments[n][1].numpy(), z["out_v_" + n], err_msg=n)
            assert not out.moments[n][0].numpy()[child].any() and not out.moments[n][1].numpy()[child].any()
            checked.update(("out_m_" + n, "out_v_" + n))
        else:
            assert n not in out.moments
    for k in ("denom", "xyz_gradient_accum", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max", "max_radii2D"):
        assert z["out_" + k].shape[0] == child.size and not z["out_" + k].any()     # reset: zeros of the new length
        checked.add("out_" + k)
    assert checked >= {k for k in z.files if not k.startswith(("in_", "lr_"))}


@pytest.mark.parametrize("n", SIZES)
def test_generated_inputs_keep_their_margins(n):
    inp = DR.generate(n)                      # asserts the margins and the rank's distance from the end of a run itself
    DR.check_margins(inp, full_levels=n >= 2049)
    if n == 0:
        return
    sc, op = DR.activated(inp)
    d = densify_rule.decisions(inp.xyz_gradient_accum.clone(), inp.xyz_gradient_accum_abs.clone(), inp.denom.clone(), sc,
                               op, inp.max_grad, **_kw(inp))
    m1, m2 = densify_rule.margins(inp.xyz_gradient_accum, inp.xyz_gradient_accum_abs, inp.denom, inp.max_grad, d["Q"])
    assert m1 > 0                              # max_grad lies between two values of the grid
    if n >= 2049:                              # a grid: Q is one of its values, with a mass of exact ties
        assert m2 == 0.0
        assert 0 < int(d["clone"].sum()) and 0 < int(d["split"].sum()) and 0 < int(d["prune"].sum()) < d["prune"].numel()


def _kw(inp, max_screen_size=20):
    c = inp.cfg
    return dict(min_opacity=c["min_opacity"], extent=c["extent"], max_screen_size=max_screen_size,
                percent_dense=c["percent_dense"])


@pytest.mark.parametrize("outcome", DR.OUTCOMES)
@pytest.mark.parametrize("n", (2049, 262145))
def test_generated_outcomes_are_what_they_say(n, outcome):
    inp = DR.generate(n, outcome=outcome)
    out, _, _ = DR.reference(inp)
    d, (n_clone, n_split, n_pruned) = out.decisions, out.ret
    new_n = out.params["xyz"].shape[0]
    assert new_n == n + n_clone + n_split - n_pruned
    if outcome == "mixed":
        assert n_clone > 0 and n_split > 0 and 0 < n_pruned and 0 < int(out.is_child.sum()) < new_n
    elif outcome == "max_only":
        assert n_clone + n_split == 1
    elif outcome == "all_zero_denom":
        assert float(d["Q"]) == 0.0 and n_clone + n_split == n and n_clone > 0 and n_split > 0
    elif outcome == "clones_only":
        assert n_clone > 0 and n_split == 0
    elif outcome == "splits_only":
        assert n_clone == 0 and n_split > 0
    elif outcome == "all_split_children_pruned":
        assert n_split == n and n_clone == 0 and new_n == 0
    elif outcome == "all_pruned":
        assert new_n == 0 and n_clone > 0 and n_split > 0


def test_inf_in_the_abs_statistic_selects_the_fixed_threshold():
    inp = DR.generate(2049, inf_abs=True)
    out, _, _ = DR.reference(inp)
    assert float(out.decisions["Q"]) == 0.99 and out.ret[0] + out.ret[1] > 1


@pytest.mark.parametrize("n", (257, 2049, 262145))
def test_float32_child_rows_are_within_the_bar_of_the_float64_reference(n):
    """The bar (rtol = atol = 2e-6) is not tighter than float32 allows: a float32 torch evaluation of the same formulas
    meets it on the generated inputs (|xyz| <= 10, samples = scaling * z)."""
    inp = DR.generate(n, outcome="splits_only")
    sc, _ = DR.activated(inp)
    g = torch.Generator().manual_seed(5)
    samples = sc * torch.randn(sc.shape, generator=g)
    x64, s64 = DR.child_rows(inp.params["xyz"], inp.params["rotation"], sc, samples, torch.float64)
    x32, s32 = DR.child_rows(inp.params["xyz"], inp.params["rotation"], sc, samples, torch.float32)
    ex = ((x32.double() - x64).abs() / (DR.CHILD_ATOL + DR.CHILD_RTOL * x64.abs())).max()
    es = ((s32.double() - s64).abs() / (DR.CHILD_ATOL + DR.CHILD_RTOL * s64.abs())).max()
    print(f"float32 error / bar: xyz {float(ex):.3f} scaling {float(es):.3f}")
    assert float(ex) <= 1.0 and float(es) <= 1.0


def test_stats_step_reproduces_the_real_methods_statistics():
    """densify_ref.stats_step (float64, rounded once per step) against the golden of tests/test_densify_stats.py."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_helpers.npz"))
    names = ("xyz_gradient_accum", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max", "denom")
    acc = {k: np.zeros((G["dstats_denom"].shape[0], 1), np.float32) for k in names}
    for step in range(2):
        DR.stats_step(acc, G[f"dstats_grad{step}"], G[f"dstats_filter{step}"])
    for k in names:
        np.testing.assert_allclose(acc[k], G["dstats_" + k], rtol=1e-6, atol=1e-7)
