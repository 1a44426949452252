"""Densification kernels (csrc/densify.hip, csrc/densify_stats.hip) at the sizes, shapes and outcomes where they can go
wrong without today's golden tests noticing:

  * the whole surgery (decide -> scan -> index -> gather -> children, sfgs.densify.densify_and_prune) against the plain
    CPU restatement tests/densify_ref.py (itself pinned to the real method by tests/test_densify_ref.py), with the real
    row shapes (f_rest 45 words), across partial workgroups, one and two rounds of the 1 024-block scan carry, degenerate
    outcomes, float64 opacity, no / partial Adam state, a column-major xyz and the Q = 0.99 route;
  * decide_masks against tests/densify_rule.py bit for bit at the same sizes;
  * sfgs_densify_gather through the C ABI: row widths around and beyond the 2 048-word chunk, more tensors than one
    launch's table holds, zero-byte rows, guard words around every destination;
  * sfgs_select_kth against a sort, bit for bit, at the corners of the radix select;
  * densify_stats row by row.

The inputs lie on a grid (tests/densify_ref.py: generate): no decision depends on a libm."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import densify_ref as DR
import densify_rule

pytestmark = pytest.mark.gpu
GROUPS = DR.GROUPS
ATTR = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
            rotation="_rotation", embeddings="_embeddings")
SIZES = (0, 1, 255, 256, 257, 2049, 262144, 262145, 524289)
STATS = ("xyz_gradient_accum", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max", "denom")


def _dev():
    return torch.device("cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _assert_same_bits(got, ref, msg):
    assert got.shape == ref.shape and got.dtype == ref.dtype, msg
    np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg=str(msg))


class _Model(types.SimpleNamespace):
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_opacity = property(lambda self: torch.sigmoid(self._opacity))


@functools.lru_cache(maxsize=4)
def _inputs(n, outcome="mixed", f64=False, inf_abs=False):
    """Generated once per combination; every user clones what it changes."""
    return DR.generate(n, outcome=outcome, opacity_dtype=torch.float64 if f64 else torch.float32, inf_abs=inf_abs)


def _model(inp, moments, dev, xyz_column_major=False):
    """As tests/test_gpu_densify.py::_model: a namespace with the reference's attribute names plus FusedAdam."""
    from sfgs.adam import FusedAdam
    m = _Model(appearance_enabled=True, percent_dense=inp.cfg["percent_dense"])
    groups = []
    for name in GROUPS:
        t = inp.params[name].to(dev)
        if name == "xyz" and xyz_column_major:       # create_from_pcd: torch.tensor(np.vstack([x, y, z]).T) (tests/test_adam.py)
            t = inp.params[name].t().contiguous().to(dev).t()
            assert t.shape[0] < 2 or not t.is_contiguous()
        p = torch.nn.Parameter(t)
        setattr(m, ATTR[name], p)
        groups.append(dict(params=[p], lr=1e-3, name=name))
    groups.append(dict(params=[torch.nn.Parameter(torch.zeros(7, device=dev))], lr=1e-3, name="appearance_mlp"))
    m.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
    for name, (ea, eas) in moments.items():
        m.optimizer.state[getattr(m, ATTR[name])] = dict(step=torch.tensor(3.0), exp_avg=ea.to(dev), exp_avg_sq=eas.to(dev))
    m.xyz_gradient_accum = inp.xyz_gradient_accum.to(dev)
    m.xyz_gradient_accum_abs = inp.xyz_gradient_accum_abs.to(dev)
    m.denom = inp.denom.to(dev)
    m.xyz_gradient_accum_abs_max = torch.ones_like(m.denom)
    m.max_radii2D = torch.ones(inp.n, device=dev)
    return m


# ---- the surgery -----------------------------------------------------------------------------------------------------------
def _case(n, outcome="mixed", mss=20, adam="some", f64=False, colmajor=False, inf_abs=False):
    tag = f"n{n}-{outcome}" + (f"-mss{mss}" if mss != 20 else "") + (f"-adam_{adam}" if adam != "some" else "") + \
        ("-opacity_f64" if f64 else "") + ("-xyz_colmajor" if colmajor else "") + ("-inf_abs" if inf_abs else "")
    return pytest.param(dict(n=n, outcome=outcome, mss=mss, adam=adam, f64=f64, colmajor=colmajor, inf_abs=inf_abs), id=tag)


SURGERY_CASES = [_case(n) for n in SIZES] + \
    [_case(n, o) for n in (2049, 262145) for o in DR.OUTCOMES if o != "mixed"] + \
    [_case(2049, f64=True), _case(2049, mss=None), _case(2049, mss=0), _case(2049, adam="all"), _case(2049, adam="none"),
     _case(2049, colmajor=True), _case(2049, inf_abs=True)]


@pytest.mark.parametrize("case", SURGERY_CASES)
def test_surgery_matches_the_plain_reference(case):
    from sfgs import densify
    dev = _dev()
    inp = _inputs(case["n"], case["outcome"], case["f64"], case["inf_abs"])
    ref, samples, moments = DR.reference(inp, case["mss"], moments=DR.moments_for(inp, case["adam"]))
    if case["inf_abs"]:
        assert float(ref.decisions["Q"]) == 0.99
    if case["outcome"] in ("all_split_children_pruned", "all_pruned"):
        assert ref.params["xyz"].shape[0] == 0
    m = _model(inp, moments, dev, case["colmajor"])
    old = {name: getattr(m, ATTR[name]) for name in GROUPS}
    mlp = m.optimizer.param_groups[-1]["params"][0]
    ret = densify.densify_and_prune(m, inp.max_grad, inp.cfg["min_opacity"], inp.cfg["extent"], case["mss"],
                                    samples=samples.clone())
    assert tuple(int(v) for v in ret) == tuple(ref.ret)
    child = ref.is_child.numpy()
    new_n = child.size
    groups = {g["name"]: g for g in m.optimizer.param_groups}
    assert groups["appearance_mlp"]["params"][0] is mlp and len(m.optimizer.param_groups) == len(GROUPS) + 1
    for name in GROUPS:
        p = getattr(m, ATTR[name])
        # optimizer re-keying: a new nn.Parameter in the group, the state moved to it
        assert groups[name]["params"][0] is p and p is not old[name], name
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_contiguous(), name
        assert old[name] not in m.optimizer.state, name
        got, want = p.detach().cpu().numpy(), ref.params[name].numpy()
        assert got.shape == want.shape == (new_n,) + DR.ROW_SHAPES[name] and got.dtype == want.dtype, name
        if name in ("xyz", "scaling"):
            _assert_same_bits(got[~child], want[~child], name)                 # survivors and clones: copies
            err = np.abs(got[child].astype(np.float64) - want[child]) / (DR.CHILD_ATOL + DR.CHILD_RTOL * np.abs(want[child]))
            print(f"{name}: {int(child.sum())} child rows, worst error / bar {float(err.max()) if err.size else 0.0:.3f}")
            np.testing.assert_allclose(got[child], want[child], rtol=DR.CHILD_RTOL, atol=DR.CHILD_ATOL, err_msg=name)
        else:
            _assert_same_bits(got, want, name)
        st = m.optimizer.state.get(p, None)
        if name in ref.moments:
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0, name
            for key, want_m in zip(("exp_avg", "exp_avg_sq"), ref.moments[name]):
                got_m = st[key].cpu().numpy()
                _assert_same_bits(got_m, want_m.numpy(), (name, key))      # the reference holds zeros for clones and children
                assert not _bits(got_m[child]).any(), (name, key)
        else:
            assert not st, name
    for k in STATS + ("max_radii2D",):
        t = getattr(m, k)
        assert tuple(t.shape) == ((new_n,) if k == "max_radii2D" else (new_n, 1)) and t.dtype == torch.float32, k
        assert t.device == dev and not _bits(t.cpu().numpy()).any(), k


@pytest.mark.parametrize("n", SIZES)
def test_decide_masks_equal_the_rule_bit_for_bit(n):
    from sfgs import densify
    dev = _dev()
    inp = _inputs(n)
    sc, op = DR.activated(inp)
    c = inp.cfg
    d = densify_rule.decisions(inp.xyz_gradient_accum.clone(), inp.xyz_gradient_accum_abs.clone(), inp.denom.clone(), sc,
                               op, inp.max_grad, c["min_opacity"], c["extent"], 20, c["percent_dense"])
    assert n < 255 or DR.last_row_fate(d, n) == DR.LAST_ROW_FATE["mixed"]
    m = _Model(_xyz=inp.params["xyz"].to(dev), _scaling=inp.params["scaling"].to(dev),
               _opacity=inp.params["opacity"].to(dev), xyz_gradient_accum=inp.xyz_gradient_accum.to(dev),
               xyz_gradient_accum_abs=inp.xyz_gradient_accum_abs.to(dev), denom=inp.denom.to(dev),
               percent_dense=c["percent_dense"])
    clone, split, keep, Q = densify.decide_masks(m, inp.max_grad, c["min_opacity"], c["extent"], 20)
    clone, split, keep = clone.cpu().numpy(), split.cpu().numpy(), keep.cpu().numpy()
    if n:
        assert float(Q) == float(d["Q"])
    rc, rs, kept = d["clone"].numpy(), d["split"].numpy()[:n], ~d["prune"].numpy()
    assert not d["split"].numpy()[n:].any()
    np.testing.assert_array_equal(clone, rc)
    np.testing.assert_array_equal(split, rs)
    # the reference's prune mask lives in its final row order [originals not split | clones | children x 2]
    n_o, n_c = int((~rs).sum()), int(rc.sum())
    np.testing.assert_array_equal(keep[:, 0][~rs], kept[:n_o])
    np.testing.assert_array_equal(keep[:, 1][rc], kept[n_o:n_o + n_c])
    ch = keep[:, 2][rs]
    np.testing.assert_array_equal(np.concatenate([ch, ch]), kept[n_o + n_c:])
    assert not keep[:, 0][rs].any() and not keep[:, 1][~rc].any() and not keep[:, 2][~rs].any()


# ---- the gather through the C ABI -------------------------------------------------------------------------------------------
SENTINEL = 0xA5C3F00D
GATHER_WIDTHS = {2049: [1, 2, 3, 7, 45, 2047, 2048, 2049, 5000, 1, 45, 2048, 3, 2, 7, 2049, 1, 3, 2047, 5000, 0, 0] +
                       [7, 2, 1, 3, 45, 1, 2, 3, 7, 1, 2, 3, 45, 7, 1, 2, 3, 1, 2, 7, 45],
                 262145: [1, 2, 3, 7, 45, 1, 2, 3, 7, 1, 2, 3, 1, 2, 3, 7, 1, 2, 3, 1, 0, 0] +
                         [2, 3, 7, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 7, 45]}


def _decide_raw(inp, dev, select):
    """sfgs_densify_decide with a host-side Q (Q_dev = NULL). -> (scratch, totals, clone, split, keep) as numpy masks."""
    from sfgs import _lib as L
    lib = L.load()
    n, c = inp.n, inp.cfg
    sc, op = DR.activated(inp)
    d = densify_rule.decisions(inp.xyz_gradient_accum.clone(), inp.xyz_gradient_accum_abs.clone(), inp.denom.clone(), sc,
                               op, inp.max_grad, c["min_opacity"], c["extent"], 20, c["percent_dense"])
    max_grad, Q = (inp.max_grad, float(d["Q"])) if select == "rule" else (1.0, 1.0)     # "none": nothing is selected
    gnorm = (inp.xyz_gradient_accum / inp.denom).nan_to_num(0.0).norm(dim=-1).to(dev)    # exact on the grid
    gabs = (inp.xyz_gradient_accum_abs / inp.denom).nan_to_num(0.0).norm(dim=-1).to(dev)
    scaling, opacity = torch.exp(inp.params["scaling"].to(dev)), torch.sigmoid(inp.params["opacity"].to(dev)).reshape(-1)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    totals = (C.c_int64 * 5)()
    scratch = torch.empty(lib.sfgs_densify_scratch_bytes(n), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(lib.sfgs_densify_decide(n, L.ptr(gnorm), L.ptr(gabs), L.ptr(scaling), L.ptr(opacity), 0, None, Q, max_grad,
                                    c["min_opacity"], f32(c["percent_dense"] * c["extent"]), f32(0.1 * c["extent"]), 1,
                                    L.ptr(scratch), scratch.numel(), totals, stream))
    clone = torch.empty(n, dtype=torch.uint8, device=dev)
    split = torch.empty(n, dtype=torch.uint8, device=dev)
    keep = torch.empty(n, 3, dtype=torch.uint8, device=dev)
    L.check(lib.sfgs_densify_masks(n, L.ptr(scratch), L.ptr(clone), L.ptr(split), L.ptr(keep), stream))
    clone, split, keep = (t.cpu().numpy().astype(bool) for t in (clone, split, keep))
    if select == "rule":
        np.testing.assert_array_equal(clone, d["clone"].numpy())
        np.testing.assert_array_equal(split, d["split"].numpy()[:n])
    else:
        assert not clone.any() and not split.any() and 0 < keep[:, 0].sum() < n
    # the last row (alone behind the scan carry at n = 262 145, alone in its workgroup at 2 049) reaches the output
    assert keep[-1].tolist() == ([True, True, False] if select == "rule" else [True, False, False])
    assert [int(v) for v in totals] == [int(keep[:, 0].sum()), int(keep[:, 1].sum()), int(keep[:, 2].sum()),
                                        int(clone.sum()), int(split.sum())]
    return scratch, totals, keep


@pytest.mark.parametrize("n,select", [(2049, "rule"), (2049, "none"), (262145, "rule"), (262145, "none")])
def test_gather_places_every_word_and_no_other(n, select):
    from sfgs import _lib as L
    lib = L.load()
    dev = _dev()
    inp = _inputs(n)
    scratch, totals, keep = _decide_raw(inp, dev, select)
    n_orig, n_clone, n_child = (int(totals[k]) for k in range(3))
    new_n = n_orig + n_clone + 2 * n_child
    assert new_n > 0 and (select == "none" or (n_clone > 0 and n_child > 0))
    widths = GATHER_WIDTHS[n]
    assert len(widths) == 43 and sum(1 for w in widths if w) > 40 and widths[20] == widths[21] == 0
    rng = np.random.default_rng(n)
    recs, held = [], []
    for t, ru in enumerate(widths):
        zero_new = t % 2
        if ru == 0:
            recs.append(L.SfgsDensifyTensor(None, None, 0, zero_new, 0))
            held.append(None)
            continue
        src = rng.integers(0, 2 ** 32, size=(n, ru), dtype=np.uint32)
        guard = 2 * ru + 64                                   # words before and after the destination
        src_d = torch.from_numpy(src.view(np.int32)).to(dev)
        buf = torch.full((new_n * ru + 2 * guard,), SENTINEL - 2 ** 32, dtype=torch.int32, device=dev)
        recs.append(L.SfgsDensifyTensor(src_d.data_ptr(), buf.data_ptr() + 4 * guard, 4 * ru, zero_new, 0))
        held.append((src, src_d, buf, guard, zero_new))
    arr = (L.SfgsDensifyTensor * len(recs))(*recs)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(lib.sfgs_densify_gather(n, L.ptr(scratch), totals, arr, len(recs), stream))
    torch.cuda.synchronize(dev)
    for t, h in enumerate(held):
        if h is None:
            continue
        src, _, buf, guard, zero_new = h
        new = (lambda a: np.zeros_like(a)) if zero_new else (lambda a: a)
        want = np.concatenate([src[keep[:, 0]], new(src[keep[:, 1]]), new(src[keep[:, 2]]), new(src[keep[:, 2]])])
        pad = np.full(guard, SENTINEL, dtype=np.uint32)
        want = np.concatenate([pad, want.reshape(-1), pad])
        got = buf.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"tensor {t}, row width {widths[t]} words, zero_new_rows {zero_new}: {bad.size} wrong words, "
                               f"first at word {int(bad[0]) - guard} of {want.size - 2 * guard}")


# ---- radix select against a sort --------------------------------------------------------------------------------------------
SELECT_SIZES = (1, 2, 4095, 4096, 4097, 8193, 100003)
VALUE_SETS = ("random_bits", "all_equal", "two_values_bits_9_0", "two_values_bits_20_10", "two_values_bits_31_21", "grid")


@functools.lru_cache(maxsize=None)
def _values(kind, n):
    """-> uint32 bit patterns of n non-negative floats."""
    rng = np.random.default_rng(n * 31 + VALUE_SETS.index(kind))
    if kind == "random_bits":        # zeros, denormals, the whole exponent range, FLT_MAX and +inf
        v = rng.integers(0, 0x7f800001, size=n, dtype=np.uint32)
        if n >= 4095:
            v[::7] = v[0]                                     # duplicates inside
            v[3], v[10], v[11], v[12], v[13] = 0, 1, 0x007fffff, 0x7f7fffff, 0x7f800000
            v[20] = v[21] = v.max()                           # ... and a duplicated maximum
    elif kind == "all_equal":
        v = np.full(n, 0x3e99999a, dtype=np.uint32)
    elif kind.startswith("two_values"):
        a, b = {"two_values_bits_9_0": (0x3f800000, 0x3f800155), "two_values_bits_20_10": (0x3f800123, 0x3f8aa923),
                "two_values_bits_31_21": (0x3f812345, 0x40012345)}[kind]
        assert {"two_values_bits_9_0": (a ^ b) < 2 ** 10, "two_values_bits_20_10": (a ^ b) % 2 ** 10 == 0 and (a ^ b) < 2 ** 21,
                "two_values_bits_31_21": (a ^ b) % 2 ** 21 == 0}[kind]
        v = np.where(rng.random(n) < 0.3, np.uint32(a), np.uint32(b)).astype(np.uint32)
        if n >= 2:
            v[0], v[1] = a, b
    else:                            # the tie-heavy grid of the densification inputs
        _, abs_i, den = DR.grid_statistics(n, torch.Generator().manual_seed(n), levels=min(2 ** 11, max(8, n // 8)))
        v = (abs_i.float() * DR.GRID / den).nan_to_num(0.0, posinf=0.0).numpy().view(np.uint32).copy()
    v.setflags(write=False)
    return v


def _ranks(srt):
    """Ranks that exercise every branch of the last kernel, chosen from the sorted values."""
    n = srt.size
    r = {0.0, float(n - 1), float(n // 2), 0.37 * (n - 1), 0.5 * (n - 1), 0.9137 * (n - 1), (n - 1) / 3.0,
         n - 1 + 0.5}                                         # beyond the end: clamped, the maximum has no successor
    vals, first, count = np.unique(srt, return_index=True, return_counts=True)
    dup = np.flatnonzero(count >= 2)
    for j in (dup[:1], dup[len(dup) // 2: len(dup) // 2 + 1]):
        for i in j:
            s, e = int(first[i]), int(first[i] + count[i] - 1)
            r.add(e + 0.5)          # floor = the LAST copy: the upper neighbour is the successor (or, at the end, none)
            r.add(float(e))
            r.add(s + 0.5)          # floor = an earlier copy: the upper neighbour is the same value
    if count[-1] >= 2:
        r.add(n - 1 - 0.5)          # fractional, inside the run of the maximum
    return sorted(x for x in r if x >= 0)


@pytest.mark.parametrize("kind", VALUE_SETS)
@pytest.mark.parametrize("n", SELECT_SIZES)
def test_select_kth_equals_a_sort_bit_for_bit(n, kind):
    from sfgs import _lib as L
    lib = L.load()
    dev = _dev()
    bits = _values(kind, n)
    srt = np.sort(bits)                 # non-negative floats order like their bit patterns
    ranks = np.array(_ranks(srt), dtype=np.float32)
    v = torch.from_numpy(bits.view(np.float32).copy()).to(dev)
    rk = torch.from_numpy(ranks).to(dev)
    out = torch.full((ranks.size, 2), float("nan"), device=dev)
    scratch = torch.empty(lib.sfgs_select_scratch_bytes(), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for i in range(ranks.size):
        L.check(lib.sfgs_select_kth(L.ptr(v), n, C.c_void_p(rk.data_ptr() + 4 * i), C.c_void_p(out.data_ptr() + 8 * i),
                                    L.ptr(scratch), scratch.numel(), stream))
    got = out.cpu().numpy().view(np.uint32)
    lo = np.minimum(np.floor(ranks).astype(np.int64), n - 1)
    hi = np.minimum(np.ceil(ranks).astype(np.int64), n - 1)
    want = np.stack([srt[lo], srt[hi]], axis=1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(float(ranks[i]), [hex(x) for x in got[i]], [hex(x) for x in want[i]]) for i in bad[:8]]


@pytest.mark.parametrize("kind", VALUE_SETS)
@pytest.mark.parametrize("n", SELECT_SIZES)
def test_quantile_linear_equals_torch_quantile_on_the_cpu(n, kind):
    from sfgs.densify import quantile_linear
    dev = _dev()
    bits = _values(kind, n)
    if kind == "random_bits":           # finite value sets only: +inf goes
        bits = np.where(bits == 0x7f800000, np.uint32(0x7f7fffff), bits)
    v = torch.from_numpy(bits.view(np.float32).copy())
    vd = v.to(dev)
    for q in (0.0, 1.0, 0.5, 0.25, 0.9137, 1.0 / 3.0):
        qt = torch.tensor(q, dtype=torch.float32)
        want, got = torch.quantile(v, qt), quantile_linear(vd, qt.to(dev)).cpu()
        assert float(got) == float(want), (q, float(got), float(want))


# ---- densify_stats ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_abs_max", (True, False))
@pytest.mark.parametrize("filter_dtype", ("bool", "uint8"))
@pytest.mark.parametrize("filter_kind", ("all_true", "all_false", "random"))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 100003))
def test_densify_stats_row_by_row(n, filter_kind, filter_dtype, with_abs_max):
    from sfgs import densify_stats
    dev = _dev()
    rng = np.random.default_rng(n * 7 + len(filter_kind))
    names = [k for k in STATS if with_abs_max or k != "xyz_gradient_accum_abs_max"]
    acc = {k: (rng.random((n, 1)) + 0.5).astype(np.float32) for k in names}       # random non-zero previous contents
    acc["denom"] = rng.integers(1, 9, size=(n, 1)).astype(np.float32)
    m = types.SimpleNamespace(**{k: torch.from_numpy(v.copy()).to(dev) for k, v in acc.items()})
    for step in range(3):
        g = (rng.standard_normal((n, 3)) * 1e-2).astype(np.float32)
        f = {"all_true": np.ones(n, bool), "all_false": np.zeros(n, bool), "random": rng.random(n) < 0.5}[filter_kind]
        if not f.all():     # NaN / inf gradients of rows outside the filter must not reach the buffers
            off = np.flatnonzero(~f)
            g[off[::3], 0], g[off[1::3], 2], g[off[2::3], 1] = np.nan, np.inf, -np.inf
        ft = torch.from_numpy(f if filter_dtype == "bool" else f.astype(np.uint8)).to(dev)
        before = {k: getattr(m, k).cpu().numpy() for k in names}
        densify_stats.add_densification_stats(m, types.SimpleNamespace(grad=torch.from_numpy(g).to(dev)), ft)
        # scene/gaussian_model.py:744-749 as tests/test_densify_stats.py restates it, in float64, rounded once per step
        DR.stats_step(acc, g, f)
        for k in names:
            got = getattr(m, k).cpu().numpy()
            _assert_same_bits(got[~f], before[k][~f], (k, step, "rows outside the filter"))
            if k == "xyz_gradient_accum":
                np.testing.assert_allclose(got, acc[k], rtol=1e-6, atol=0, err_msg=f"{k} step {step}")
            else:
                _assert_same_bits(got, acc[k], (k, step))
