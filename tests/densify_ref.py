"""Plain CPU reference of the whole densify_and_prune surgery, and a generator of inputs whose decisions cannot depend
on rounding -- TEST INFRASTRUCTURE for tests/test_gpu_densify_edges.py.

`surgery()` performs scene/gaussian_model.py:707-742 on plain tensors in the reference's statement order -- clone, append
(zero moments for the new rows), split with zero-padded gradients, append, prune the parents, final prune -- with ordinary
boolean indexing, `repeat` and `cat`. The decisions come from tests/densify_rule.py (pinned to masks captured inside the
real methods); the two computed tensors (child rows of xyz and raw scaling) are formed in float64 from the float32
inputs. tests/test_densify_ref.py ties it to the real method's outputs (tests/golden/reference_densify_full.npz).

`generate()` builds a model's worth of inputs on a grid: gradient statistics are small integers times 2^-16 over a
power-of-two denom (quotient, square and square root exact in any libm), thresholds sit between grid values, raw
scaling and opacity come from a few discrete levels far from every threshold. The margins are asserted, not assumed."""
import types

import numpy as np
import torch

import densify_rule

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "embeddings")
ROW_SHAPES = dict(xyz=(3,), f_dc=(1, 3), f_rest=(15, 3), opacity=(1,), scaling=(3,), rotation=(4,), embeddings=(32,))
CHILD_RTOL = CHILD_ATOL = 2e-6      # the project's bar for the computed child rows (tests/test_gpu_densify.py)


def rotation_matrices(q):
    """[M,4] raw quaternions (w, x, y, z) -> [M,3,3], normalised first (build_rotation)."""
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1)
    return R.reshape(-1, 3, 3)


def child_rows(xyz, rotation, scaling_act, samples, dtype=torch.float64):
    """Child rows of the SELECTED parents (already `repeat`ed twice): xyz + R(q / |q|) sample and log(scaling * 0.625),
    evaluated in `dtype` from the float32 inputs."""
    R = rotation_matrices(rotation.to(dtype))
    new_xyz = torch.bmm(R, samples.to(dtype).unsqueeze(-1)).squeeze(-1) + xyz.to(dtype)
    new_scaling = torch.log(scaling_act.to(dtype) * 0.625)
    return new_xyz, new_scaling


def surgery(params, moments, xyz_gradient_accum, xyz_gradient_accum_abs, denom, scaling_act, opacity_act, max_grad,
            min_opacity, extent, max_screen_size, percent_dense, samples):
    """params: {group: float tensor [N, ...]}; moments: {group: (exp_avg, exp_avg_sq)} for the groups that have Adam
    state (the others are "absent"); scaling_act / opacity_act = get_scaling / get_opacity; samples [2 * n_split, 3].
    Returns SimpleNamespace(params, moments, ret=(n_cloned, n_split, n_pruned), is_child[new_n], decisions)."""
    d = densify_rule.decisions(xyz_gradient_accum.clone(), xyz_gradient_accum_abs.clone(), denom.clone(), scaling_act,
                               opacity_act, max_grad, min_opacity, extent, max_screen_size, percent_dense)
    clone, split, prune = d["clone"], d["split"], d["prune"]
    n = clone.shape[0]
    P = {k: v.clone() for k, v in params.items()}
    M = {k: (m.clone(), v.clone()) for k, (m, v) in moments.items()}
    is_child = torch.zeros(n, dtype=torch.bool)

    def append(new):
        for k in P:
            P[k] = torch.cat([P[k], new[k]])
            if k in M:
                M[k] = tuple(torch.cat([t, torch.zeros(new[k].shape, dtype=t.dtype)]) for t in M[k])

    def keep_rows(mask):
        for k in P:
            P[k] = P[k][mask]
            if k in M:
                M[k] = tuple(t[mask] for t in M[k])

    # densify_and_clone
    append({k: v[clone] for k, v in P.items()})
    scaling_act = torch.cat([scaling_act, scaling_act[clone]])
    is_child = torch.cat([is_child, torch.zeros(int(clone.sum()), dtype=torch.bool)])
    # densify_and_split (the decision used gradients zero-padded for the clones)
    n_split = int(split.sum())
    assert tuple(samples.shape) == (2 * n_split, 3)
    rep = lambda t: t[split].repeat(2, *([1] * (t.dim() - 1)))
    new = {k: rep(v) for k, v in P.items()}
    new_xyz, new_scaling = child_rows(rep(P["xyz"]), rep(P["rotation"]), rep(scaling_act), samples)
    new["xyz"], new["scaling"] = new_xyz.to(P["xyz"].dtype), new_scaling.to(P["scaling"].dtype)
    append(new)
    is_child = torch.cat([is_child, torch.ones(2 * n_split, dtype=torch.bool)])
    # prune the parents, then the final prune
    not_parent = torch.cat([~split, torch.ones(2 * n_split, dtype=torch.bool)])
    keep_rows(not_parent)
    is_child = is_child[not_parent]
    assert prune.shape[0] == is_child.shape[0]
    keep_rows(~prune)
    is_child = is_child[~prune]
    ret = (int(clone.sum()), n_split, int(prune.sum()))
    return types.SimpleNamespace(params=P, moments=M, ret=ret, is_child=is_child, decisions=d)


# ---- inputs on a grid ---------------------------------------------------------------------------------------------------
EXTENT, PERCENT_DENSE, MIN_OPACITY = 5.0, 0.01, 0.005
# largest activated scale of a Gaussian. Thresholds: percent_dense * extent = 0.05 (clone | split), 0.1 * extent = 0.5
# (a row is pruned as too big), 0.1 * extent / 0.625 = 0.8 (its children are too)
SCALE_LEVELS = (0.02, 0.04, 0.08, 0.3, 0.6, 1.2)
OPACITY_LEVELS = (-7.0, -6.0, -4.0, 0.0, 2.0)       # raw; sigmoid = 9.1e-4, 2.5e-3 | 1.8e-2, 0.5, 0.88
OUTCOMES = ("mixed", "max_only", "all_zero_denom", "clones_only", "splits_only", "all_split_children_pruned",
            "all_pruned")
GRID = 2.0 ** -16


def _quantile_is_robust(gnorm, gabs, max_grad):
    """The CPU forms ratio = count / n, the device count * (1 / n): the rank may differ by an ulp or two. Q must not."""
    n = gabs.numel()
    count = int((gnorm >= max_grad).sum())
    if count in (0, n) or n == 1:
        return True                    # ratio is exactly 0 or 1 on both
    srt = torch.sort(gabs).values.double()
    rank = float(((1 - (gnorm >= max_grad).float().mean()) * (n - 1)).to(torch.float32))
    qs = set()
    for ulps in range(-8, 9):
        r = min(max(rank * (1 + ulps * 2.0 ** -23), 0.0), n - 1.0)
        lo, hi = int(np.floor(r)), int(np.ceil(r))
        qs.add(float(srt[lo] + (r - lo) * (srt[hi] - srt[lo])))
    return len(qs) == 1


def grid_statistics(n, g, levels=None):
    """(accum, accum_abs) as integers < 2^11 (to be scaled by 2^-16) and a power-of-two denom with some zeros."""
    ri = lambda hi, *shape: torch.randint(0, hi, shape, generator=g)
    if levels is None:
        levels = min(2 ** 11, max(8, n // 32))      # few distinct values: long runs of exact ties at every n
    table = torch.sort(torch.randperm(2 ** 11, generator=g)[:levels]).values
    acc_i, abs_i = table[ri(levels, n)], table[ri(levels, n)]
    den = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 1.0, 2.0, 4.0, 1.0, 2.0, 4.0, 1.0, 2.0, 4.0])[ri(16, n)]
    return acc_i, abs_i, den


def generate(n, seed=0, outcome="mixed", opacity_dtype=torch.float32, inf_abs=False, levels=None):
    """-> SimpleNamespace(params{group: [n, ...]}, xyz_gradient_accum, xyz_gradient_accum_abs, denom, max_grad, cfg).
    outcome "max_only": the reference always selects the rows that hold the maximum of grads_abs (Q = quantile(., 1) and
    the test is >=), so "nothing selected" means exactly one row, the unique maximum."""
    assert outcome in OUTCOMES
    g = torch.Generator().manual_seed(1000003 * seed + n)
    ri = lambda hi, *shape: torch.randint(0, hi, shape, generator=g)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    acc_i, abs_i, den = grid_statistics(n, g, levels)
    if outcome in ("all_zero_denom", "all_split_children_pruned"):
        den = torch.zeros(n)
    if outcome == "max_only" and n > 0:
        abs_i = abs_i.clamp(max=2 ** 11 - 2)
        j = n // 3
        abs_i[j], den[j] = 2 ** 11 - 1, 1.0
    if n > 0 and outcome not in ("max_only", "all_zero_denom", "all_split_children_pruned"):
        acc_i[-1], den[-1] = 2 ** 11 - 1, 1.0      # the LAST row is selected (LAST_ROW_FATE): the largest value of the grid
    acc_i[den == 0], abs_i[den == 0] = 0, 0        # never visible: 0 / 0 = NaN -> 0 (x / 0 would be inf: the Q = 0.99 route)
    accum = (acc_i.float() * GRID).reshape(n, 1)
    accum_abs = (abs_i.float() * GRID).reshape(n, 1)
    denom = den.reshape(n, 1)
    if inf_abs:
        j = (2 * n) // 3
        accum_abs[j], denom[j] = float("inf"), 2.0
    gnorm = (accum / denom).nan_to_num(0.0).norm(dim=-1)
    gabs = (accum_abs / denom).nan_to_num(0.0, posinf=0.0).norm(dim=-1)
    # max_grad: half a grid step (the quotients are multiples of 2^-18) above a value of the grid
    max_grad = 1.0
    if outcome != "max_only":
        vals = torch.unique(gnorm)
        for frac in (0.8, 0.75, 0.85, 0.7, 0.9, 0.65, 0.6, 0.5):
            max_grad = (float(vals[int(frac * (vals.numel() - 1))]) if n else 0.0) + 2.0 ** -19
            if _quantile_is_robust(gnorm, gabs, max_grad):
                break
        else:
            raise AssertionError("no max_grad with a rank inside a run of ties")
    assert n == 0 or float(((gnorm - max_grad).abs()).min()) >= 2.0 ** -19 or outcome == "max_only"
    assert _quantile_is_robust(gnorm, gabs, max_grad)
    # ---- raw scaling and opacity from discrete levels --------------------------------------------------------------
    sl = {"clones_only": SCALE_LEVELS[:2], "splits_only": SCALE_LEVELS[2:],
          "all_split_children_pruned": SCALE_LEVELS[5:]}.get(outcome, SCALE_LEVELS)
    ol = OPACITY_LEVELS[:2] if outcome == "all_pruned" else OPACITY_LEVELS
    smax = torch.tensor(sl)[ri(len(sl), n)]
    opacity_raw = torch.tensor(ol)[ri(len(ol), n)]
    if n > 0:       # the last row is the only one behind the scan carry at n = 262 145 and alone in its workgroup at 257, 2 049
        smax[-1] = {"splits_only": 0.08, "all_split_children_pruned": 1.2}.get(outcome, 0.04)
        opacity_raw[-1] = OPACITY_LEVELS[0] if outcome == "all_pruned" else OPACITY_LEVELS[-1]
    axes = torch.tensor([1.0, 0.7, 0.45])[torch.argsort(torch.rand(n, 3, generator=g), dim=1)]   # the largest: any axis
    scaling = torch.log(smax.reshape(n, 1) * axes)
    opacity = opacity_raw.to(opacity_dtype).reshape(n, 1)
    params = dict(xyz=(torch.rand(n, 3, generator=g) * 20 - 10), f_dc=rn(n, 1, 3), f_rest=rn(n, 15, 3), opacity=opacity,
                  scaling=scaling, rotation=rn(n, 4) + torch.tensor([0.5, 0, 0, 0]), embeddings=rn(n, 32))
    cfg = dict(min_opacity=MIN_OPACITY, extent=EXTENT, percent_dense=PERCENT_DENSE)
    out = types.SimpleNamespace(params=params, xyz_gradient_accum=accum, xyz_gradient_accum_abs=accum_abs, denom=denom,
                                max_grad=max_grad, cfg=cfg, outcome=outcome, n=n)
    check_margins(out, full_levels=(outcome == "mixed" and n >= 2049))
    return out


def check_margins(inp, full_levels=False):
    """No decision of these inputs lies near a threshold: asserted here, on the CPU, for every generated input."""
    sm = torch.exp(inp.params["scaling"]).max(dim=1).values.double()
    op = torch.sigmoid(inp.params["opacity"]).double().reshape(-1)
    ext, pd, mo = inp.cfg["extent"], inp.cfg["percent_dense"], inp.cfg["min_opacity"]
    thresholds = (pd * ext, 0.1 * ext, 0.1 * ext / 0.625)
    for thr in thresholds:
        assert not bool(((sm - thr).abs() <= 1e-4 * thr).any()), thr
    assert not bool(((op - mo).abs() <= 1e-3 * mo).any())
    assert bool((inp.params["xyz"].abs() <= 10).all())
    if full_levels:     # both sides of every threshold are populated
        for thr in thresholds:
            assert bool((sm < thr).any()) and bool((sm > thr).any()), thr
        assert bool((op < mo).any()) and bool((op > mo).any())
        assert bool((inp.denom == 0).any())


# what becomes of the last row (n >= 255), per outcome: (cloned, split, original kept, clone kept, children kept). Between
# "mixed" and "splits_only" the one row behind the carry at n = 262 145 feeds every category of the scan.
LAST_ROW_FATE = dict(mixed=(1, 0, 1, 1, 0), clones_only=(1, 0, 1, 1, 0), all_zero_denom=(1, 0, 1, 1, 0),
                     splits_only=(0, 1, 0, 0, 1), max_only=(0, 0, 1, 0, 0), all_pruned=(1, 0, 0, 0, 0),
                     all_split_children_pruned=(0, 1, 0, 0, 0))


def last_row_fate(d, n):
    """(cloned, split, original kept, clone kept, children kept) of row n - 1 from densify_rule.decisions' masks, whose
    prune mask lives in the final row order [originals not split | clones | children x 2]."""
    clone, split, kept = d["clone"], d["split"][:n], ~d["prune"]
    n_o, n_c, n_s = int((~split).sum()), int(clone.sum()), int(split.sum())
    c, s = bool(clone[-1]), bool(split[-1])
    orig = (not s) and bool(kept[n_o - 1])
    cl = c and bool(kept[n_o + n_c - 1])
    ch = s and bool(kept[n_o + n_c + n_s - 1]) and bool(kept[n_o + n_c + 2 * n_s - 1])
    return tuple(int(v) for v in (c, s, orig, cl, ch))


def activated(inp):
    """get_scaling / get_opacity of the generated model, on the CPU."""
    return torch.exp(inp.params["scaling"]), torch.sigmoid(inp.params["opacity"])


def make_samples(inp, decisions, seed=0):
    """samples [2 * n_split, 3] = scaling * z in the reference's layout: child k of the parent with split rank r at row
    k * n_split + r."""
    g = torch.Generator().manual_seed(77 + seed)
    n = inp.n
    split = decisions["split"][:n]
    assert not bool(decisions["split"][n:].any())       # a clone is never split in the same pass
    std = torch.exp(inp.params["scaling"])[split].repeat(2, 1)
    return std * torch.randn(std.shape, generator=g)


def moments_for(inp, which="some", seed=0):
    """Adam moments for `which` in ("all", "none", "some") groups; non-zero random bits so that a wrong row shows."""
    g = torch.Generator().manual_seed(4242 + seed)
    names = dict(all=GROUPS, none=(), some=("f_dc", "f_rest", "opacity", "scaling", "embeddings"))[which]
    return {k: (torch.randn(inp.params[k].shape, generator=g).to(inp.params[k].dtype),
                (torch.rand(inp.params[k].shape, generator=g) + 0.5).to(inp.params[k].dtype)) for k in names}


def reference(inp, max_screen_size=20, moments=None, samples_seed=0):
    """Decisions + samples + surgery for generated inputs. -> (surgery result, samples, moments)."""
    sc, op = activated(inp)
    c = inp.cfg
    d = densify_rule.decisions(inp.xyz_gradient_accum.clone(), inp.xyz_gradient_accum_abs.clone(), inp.denom.clone(), sc,
                               op, inp.max_grad, c["min_opacity"], c["extent"], max_screen_size, c["percent_dense"])
    if inp.n >= 255:
        assert last_row_fate(d, inp.n) == LAST_ROW_FATE[inp.outcome], (inp.outcome, last_row_fate(d, inp.n))
    samples = make_samples(inp, d, samples_seed)
    moments = moments_for(inp, "some") if moments is None else moments
    out = surgery(inp.params, moments, inp.xyz_gradient_accum, inp.xyz_gradient_accum_abs, inp.denom, sc, op,
                  inp.max_grad, c["min_opacity"], c["extent"], max_screen_size, c["percent_dense"], samples)
    return out, samples, moments


# ---- add_densification_stats ----------------------------------------------------------------------------------------------
def stats_step(acc, g, f):
    """One add_densification_stats (scene/gaussian_model.py:744-749) on numpy float32 buffers acc[name] [n,1], in place:
    the statements of tests/test_densify_stats.py's restatement, evaluated in float64 and rounded once. g [n,3] float32,
    f bool [n]; xyz_gradient_accum_abs_max is skipped when acc does not hold it."""
    g64 = g.astype(np.float64)
    add = lambda k, v: (acc[k][f].astype(np.float64) + v).astype(np.float32)
    na = np.linalg.norm(g64[f, 2:], axis=-1, keepdims=True)
    acc["xyz_gradient_accum"][f] = add("xyz_gradient_accum", np.linalg.norm(g64[f, :2], axis=-1, keepdims=True))
    acc["xyz_gradient_accum_abs"][f] = add("xyz_gradient_accum_abs", na)
    if "xyz_gradient_accum_abs_max" in acc:
        acc["xyz_gradient_accum_abs_max"][f] = np.maximum(acc["xyz_gradient_accum_abs_max"][f].astype(np.float64),
                                                          na).astype(np.float32)
    acc["denom"][f] = add("denom", 1.0)
