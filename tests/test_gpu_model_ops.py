"""The kernels that sfgs.*.install() hooks into the model (prepass / act_math.h, sh_eval, adam, compact, filter3d,
densify_stats, and the brute-force distCUDA2) against float64 references, element by element: every output and gradient
element within K * eps * unit of tests/model_ops_ref.py (K measured there against references only), data movement bit for
bit. Shapes are the smallest that reach the code in question; each test says which launch or loop round that is.
Every comparison prints its largest error in units (`UNITS <op> <tensor> <value>`; run with -s)."""
import numpy as np
import pytest
import torch

import model_ops_ref as R
from oracle import oracle as orc
from oracle.filter3d_np import compute_3D_filter as oracle_filter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_TORCH = {np.float32: torch.float32, np.float64: torch.float64}


def _bound(op, tensor, got, ref, unit, eps=R.EPS32, where=""):
    e = R.in_units_ld(got, np.asarray(ref).astype(np.longdouble), np.asarray(unit).astype(np.longdouble), eps)
    w = float(e.max()) if e.size else 0.0
    print(f"UNITS {op} {tensor} {w:.4g} {where}")
    assert w <= R.k_of(op, tensor), (op, tensor, where, w, int(e.argmax()) if e.size else -1)
    return w


def _dev(a, grad=False):
    return torch.tensor(a, device=DEV).requires_grad_(grad)


# ---- prepass ---------------------------------------------------------------------------------------------------------
def _prepass_run(x, use=("scales", "opacity", "rotation")):
    from sfgs.prepass import fused_activations
    a, b, c = _dev(x["scaling"], True), _dev(x["opacity"], True), _dev(x["rotation"], True)
    sc, op, ro = fused_activations(a, b, c, _dev(x["filt"]))
    loss = 0
    if "scales" in use:
        loss = loss + (sc * _dev(x["g_scales"])).sum()
    if "opacity" in use:
        loss = loss + (op * _dev(x["g_opacity"])).sum()
    if "rotation" in use:
        loss = loss + (ro * _dev(x["g_rotation"])).sum()
    loss.backward()
    assert b.grad.dtype == b.dtype and a.grad.dtype == torch.float32 and c.grad.dtype == torch.float32
    assert sc.dtype == op.dtype == ro.dtype == torch.float32
    n = lambda t: t.detach().cpu().numpy()
    return dict(scales=n(sc), opacity=n(op), rotation=n(ro), g_scaling=n(a.grad), g_opacity=n(b.grad), g_rotation=n(c.grad))


@pytest.mark.parametrize("route", range(4))
def test_prepass_every_element_on_every_dtype_route(route):
    """The four (filter_3D dtype, raw opacity dtype) branches of SFGS_ACT_DISPATCH, forward and backward, one partial block
    (N = 1, 255), one full block (256), two blocks (257) and 17 blocks (4 099); the quaternion cases are the first rows."""
    ft, ot = R.ROUTES[route]
    for n in R.BLOCK_NS:
        x = R.prepass_inputs(n, R.MEASURE_SEED + n, ft, ot)
        ref, unit = R.prepass_ref(**x)
        got = _prepass_run(x)
        assert got["g_opacity"].dtype == ot            # the raw opacity's gradient has its parameter's dtype
        for k in R.PREPASS_TENSORS:
            _bound("prepass", k, got[k], ref[k], unit[k], where=f"route {route} N {n}")


@pytest.mark.parametrize("use", ["scales", "opacity", "rotation"])
def test_prepass_loss_on_one_output_only(use):
    """A loss that reads one of the three outputs: the gradients of the inputs the others feed are exactly the reference's
    zeros, the rest stays within the bound (autograd hands the op zero tensors for the unused outputs)."""
    x = R.prepass_inputs(257, 17, np.float64, np.float64)
    key = dict(scales="g_scales", opacity="g_opacity", rotation="g_rotation")[use]
    ref, unit = R.prepass_ref(x["scaling"], x["opacity"], x["rotation"], x["filt"], **{key: x[key]})
    got = _prepass_run(x, use=(use,))
    for k in ("g_scaling", "g_opacity", "g_rotation"):
        _bound("prepass", k, got[k], ref[k], unit[k], where=f"only {use}")
        if not ref[k].any():
            assert not got[k].any(), k


@pytest.mark.parametrize("absent", ["g_scales", "g_opacity", "g_rotation"])
@pytest.mark.parametrize("route", [0, 3])
def test_prepass_backward_with_a_null_upstream_gradient(absent, route):
    """sfgs_prepass_backward's `g_scales`, `g_opacities`, `g_rotations == NULL` branches, through the C entry (the autograd
    wrapper materialises zeros instead): the same values as with the reference's absent term."""
    from sfgs import _call, _lib as L
    from sfgs.prepass import f64_mask
    ft, ot = R.ROUTES[route]
    n = 257
    x = R.prepass_inputs(n, 23, ft, ot)
    x[absent] = None
    ref, unit = R.prepass_ref(**x)
    t = {k: (None if v is None else _dev(v)) for k, v in x.items()}
    gs, gr = torch.full((n, 3), 7.0, device=DEV), torch.full((n, 4), 7.0, device=DEV)
    go = torch.full((n, 1), 7.0, device=DEV, dtype=_TORCH[ot])
    dev = torch.device(DEV)
    with torch.cuda.device(dev):
        L.check(L.load().sfgs_prepass_backward(n, L.ptr(t["scaling"]), L.ptr(t["opacity"]), L.ptr(t["rotation"]),
                                               L.ptr(t["filt"]), f64_mask(t["filt"], t["opacity"]), L.ptr(t["g_scales"]),
                                               L.ptr(t["g_opacity"]), L.ptr(t["g_rotation"]), L.ptr(gs), L.ptr(go), L.ptr(gr),
                                               _call.stream(dev)))
    for k, g in (("g_scaling", gs), ("g_opacity", go), ("g_rotation", gr)):
        _bound("prepass", k, g.cpu().numpy(), ref[k], unit[k], where=f"NULL {absent} route {route}")
    if absent == "g_rotation":
        assert not gr.cpu().numpy().any()
    if absent == "g_opacity":
        assert not go.cpu().numpy().any()


def test_prepass_quaternion_edges():
    """exact zero and |q| = 1e-13 (F.normalize's clamped denominator, forward and backward), |q| from 1e-3 to 1e3, one
    component dominating: quaternion_cases() alone, at a size of its own"""
    q = R.quaternion_cases()
    x = R.prepass_inputs(q.shape[0], 29)
    assert (x["rotation"] == q).all()
    ref, unit = R.prepass_ref(**x)
    got = _prepass_run(x)
    assert not got["rotation"][0].any() and (got["g_rotation"][0] == x["g_rotation"][0] * np.float32(1e12)).all()
    for k in ("rotation", "g_rotation"):
        _bound("prepass", k, got[k], ref[k], unit[k], where="quaternion cases")
    free = np.linalg.norm(q.astype(np.float64), axis=1) > 1e-3 * 0.5
    assert np.abs(np.linalg.norm(got["rotation"][free].astype(np.float64), axis=1) - 1).max() < 1e-6


# ---- eval_sh ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_eval_sh_every_element(deg):
    """sh_eval_fwd / sh_eval_bwd at K = (deg+1)^2 (the zero-fill loop `for k = M; k < K` runs zero times), at 16 and 25 and
    at an odd count, with unit directions and with norms 0.1 .. 10, around the 256-thread block; and the g_dirs == NULL
    launch (dirs without requires_grad), whose g_sh must be the same bits."""
    from sfgs.sh import eval_sh
    m = (deg + 1) ** 2
    for kk in R.sh_coeff_counts(deg):
        for n in R.BLOCK_NS:
            for unit_dirs in (True, False):
                x = R.sh_inputs(n, kk, 1000 * deg + 10 * kk + n, unit_dirs)
                ref, unit = R.eval_sh_ref(deg, **x)
                sh, dirs = _dev(x["sh"], True), _dev(x["dirs"], True)
                out = eval_sh(deg, sh, dirs)
                (out * _dev(x["g_out"])).sum().backward()
                where = f"deg {deg} K {kk} N {n} unit {unit_dirs}"
                g_sh = sh.grad.cpu().numpy()
                _bound("eval_sh", "out", out.detach().cpu().numpy(), ref["out"], unit["out"], where=where)
                _bound("eval_sh", "g_sh", g_sh, ref["g_sh"], unit["g_sh"], where=where)
                _bound("eval_sh", "g_dirs", dirs.grad.cpu().numpy(), ref["g_dirs"], unit["g_dirs"], where=where)
                assert not g_sh[:, :, m:].any()                      # exact zeros in the unused coefficients
                sh2 = _dev(x["sh"], True)
                out2 = eval_sh(deg, sh2, _dev(x["dirs"]))            # g_dirs == NULL
                (out2 * _dev(x["g_out"])).sum().backward()
                assert torch.equal(out2, out) and torch.equal(sh2.grad.view(torch.int32), sh.grad.view(torch.int32))


# ---- Adam ------------------------------------------------------------------------------------------------------------
_SIZES = (1, 4095, 4096, 4097, 8191, 8193)      # around ADAM_CHUNK = 4 096 elements: one block, tail blocks, whole blocks


def _adam_case(count, t_single=None):
    """`count` tensors that reach the kernel, each in a group of its own with its own lr, weight_decay (every third 0), step
    count, size and dtype (every fourth float64), every other one a view offset by one element (not 16-byte aligned: the
    scalar loop instead of the float4 path); interleaved with zero-element tensors and parameters without a gradient."""
    groups, items = [], []
    for i in range(count):
        h = R.adam_hyper(i, t_single)
        dt = np.float64 if i % 4 == 3 else np.float32
        n = _SIZES[i % len(_SIZES)] if t_single is None else 8193
        p, g, m, v = R.adam_inputs(n, 500 + i, dt, zeros=5 if h["weight_decay"] == 0 else 0)
        off = i % 2

        def put(a):
            buf = torch.zeros(n + 4, dtype=_TORCH[dt], device=DEV)
            view = buf[off:off + n]
            view.copy_(torch.tensor(a))
            assert view.data_ptr() % 16 == (0 if off == 0 else a.itemsize)
            return view
        tp = put(p).requires_grad_(True)
        tp.grad = put(g)
        items.append(dict(kind="real", p=tp, h=h, np=(p, g, m, v), state=dict(
            step=torch.tensor(float(h["t"] - 1)), exp_avg=put(m), exp_avg_sq=put(v)), dt=dt))
        if i % 5 == 1:      # a zero-element tensor with a gradient: skipped by the launch, its step still counts
            e = torch.zeros(0, 3, device=DEV, requires_grad=True)
            e.grad = torch.zeros(0, 3, device=DEV)
            items.append(dict(kind="empty", p=e, h=h, state=dict(step=torch.tensor(4.0), exp_avg=torch.zeros(0, 3, device=DEV),
                                                                 exp_avg_sq=torch.zeros(0, 3, device=DEV))))
        if i % 5 == 3:      # a parameter without a gradient: untouched, no step
            q = torch.randn(33, device=DEV, generator=torch.Generator(DEV).manual_seed(i)).requires_grad_(True)
            items.append(dict(kind="nograd", p=q, h=h, keep=q.detach().clone(), state=dict(
                step=torch.tensor(6.0), exp_avg=torch.ones(33, device=DEV), exp_avg_sq=torch.ones(33, device=DEV))))
    for it in items:
        groups.append(dict(params=[it["p"]], lr=it["h"]["lr"], weight_decay=it["h"]["weight_decay"]))
    return groups, items


def _adam_check(items, where):
    worst = {k: 0.0 for k in R.ADAM_TENSORS}
    for j, it in enumerate(items):
        st = it["state"]
        if it["kind"] == "nograd":
            assert float(st["step"]) == 6.0 and torch.equal(it["p"].detach(), it["keep"])
            assert torch.equal(st["exp_avg"], torch.ones(33, device=DEV))
            continue
        if it["kind"] == "empty":
            assert float(st["step"]) == 5.0            # torch.optim.Adam counts the step of an empty parameter too
            continue
        p, g, m, v = it["np"]
        h = it["h"]
        assert float(st["step"]) == float(h["t"])      # as torch's: incremented once
        ref, unit = R.adam_ref(p, g, m, v, **h)
        eps = R.EPS64 if it["dt"] is np.float64 else R.EPS32
        got = dict(p=it["p"].detach().cpu().numpy(), m=st["exp_avg"].cpu().numpy(), v=st["exp_avg_sq"].cpu().numpy())
        for k in R.ADAM_TENSORS:
            assert got[k].dtype == it["dt"]
            e = R.in_units_ld(got[k], ref[k], unit[k], eps)
            worst[k] = max(worst[k], float(e.max()))
            assert e.max() <= R.k_of("adam", k), (where, j, k, float(e.max()), int(e.argmax()), h, got[k].size)
        if h["weight_decay"] == 0:                     # g = m = v = 0: a Gaussian no camera saw does not move
            assert (got["p"][:5] == p[:5]).all() and not got["m"][:5].any() and not got["v"][:5].any()
    for k, w in worst.items():
        print(f"UNITS adam {k} {w:.4g} {where}")


@pytest.mark.parametrize("t", R.ADAM_STEPS)
def test_adam_one_step_from_an_injected_state(t):
    """one tensor (8 193 elements = two whole blocks and a one-element tail), float32 aligned; and the same as float64"""
    from sfgs.adam import FusedAdam
    for i in (0, 3, 1):      # float32 aligned without weight decay; float64; float32 offset by one element with weight decay
        h = R.adam_hyper(i, t)
        dt = np.float64 if i == 3 else np.float32
        p, g, m, v = R.adam_inputs(8193, 40 + t % 97 + i, dt, zeros=5 if h["weight_decay"] == 0 else 0)
        buf = [torch.zeros(8193 + 4, dtype=_TORCH[dt], device=DEV)[i % 2:i % 2 + 8193].copy_(torch.tensor(a)) for a in (p, g, m, v)]
        tp = buf[0].requires_grad_(True)
        tp.grad = buf[1]
        opt = FusedAdam([tp], lr=h["lr"], eps=h["eps"], weight_decay=h["weight_decay"])
        st = dict(step=torch.tensor(float(t - 1)), exp_avg=buf[2], exp_avg_sq=buf[3])
        opt.state[tp] = st
        opt.step()
        _adam_check([dict(kind="real", p=tp, h=h, np=(p, g, m, v), state=st, dt=dt)], f"t {t} tensor {i}")


@pytest.mark.parametrize("count", [24, 25, 49, 50])
def test_adam_many_tensors_each_with_its_own_scalars(count):
    """ADAM_MAX_TENSORS = 24 table entries per launch: 24 tensors fill one table exactly, 25 take a second launch with one
    entry, 49 a third launch with one entry, 50 a third with two. Every tensor has its own scalars and size, so a block that
    takes another tensor's table entry (block_end, the pointers, vec_ok) or another launch's fails its bound."""
    from sfgs.adam import FusedAdam
    groups, items = _adam_case(count)
    assert sum(it["kind"] == "real" for it in items) == count and -(-count // 24) == {24: 1, 25: 2, 49: 3, 50: 3}[count]
    opt = FusedAdam(groups, lr=1.0, eps=1e-15)
    for it in items:
        opt.state[it["p"]] = it["state"]
    opt.step()
    _adam_check(items, f"{count} tensors")


# ---- compact ---------------------------------------------------------------------------------------------------------
def _same_bits(o, want):
    assert o.shape == want.shape and o.dtype == want.dtype
    return torch.equal(o.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))


@pytest.mark.parametrize("mask", ["random", "low", "high"])
def test_compact_block_scan_second_round(mask):
    """N = 4 194 304 + 4 097 = 4 198 401 rows = 1 026 blocks of CP_CHUNK = 4 096 rows: scan_sums_kernel (csrc/scan.h) scans 1 024
    block sums per round, so blocks 1 024 and 1 025 are placed by the second round from the carry of the first. With
    everything kept below row 4 194 304 the carry is all there is; with everything kept above it, it must be zero."""
    from sfgs.compact import compact_rows
    n, cut = 4_194_304 + 4_097, 4_194_304
    assert -(-n // 4096) == 1026
    g = torch.Generator(DEV).manual_seed(3)
    if mask == "random":
        keep = torch.rand(n, device=DEV, generator=g) < 0.5
    else:
        keep = torch.arange(n, device=DEV) < cut
        if mask == "high":
            keep = ~keep
    a = torch.randint(0, 255, (n,), device=DEV, dtype=torch.uint8, generator=g)
    b = torch.arange(n, device=DEV, dtype=torch.float32)
    oa, ob = compact_rows(keep, [a, b])
    assert _same_bits(oa, a[keep]) and _same_bits(ob, b[keep])


@pytest.mark.parametrize("count", [49, 97])
def test_compact_more_tensors_than_one_table(count):
    """CP_MAX_TENSORS = 48 table entries per gather launch: 49 tensors with rows take a second launch with one entry, 97 a
    third; [N, 0] tensors in between take no entry. Every tensor has its own content and row size."""
    from sfgs.compact import compact_rows
    n = 777
    g = torch.Generator(DEV).manual_seed(count)
    keep = torch.rand(n, device=DEV, generator=g) < 0.6
    ts = []
    for i in range(count):
        ts.append(torch.randn(n, 1 + i % 7, device=DEV, generator=g) + 100.0 * i)
        if i % 10 == 4:
            ts.append(torch.zeros(n, 0, device=DEV))
    assert sum(t.numel() > 0 for t in ts) == count
    outs = compact_rows(keep, ts)
    assert len(outs) == len(ts)
    for t, o in zip(ts, outs):
        assert _same_bits(o, t[keep])


@pytest.mark.parametrize("ru", [1, 2, 3, 5, 7, 45, 2047, 2048, 2049])
def test_compact_word_rows(ru):
    """compact_gather_kernel's row of a word: one 64-bit division per block, then a float estimate with one correction. Rows
    of `ru` 4-byte units at N = 1 301, so that a block's 2 048 units start inside a row (1 301 ru is no multiple of 2 048
    for any of these but 2 048 itself)."""
    from sfgs.compact import compact_rows
    n = 1301
    assert (n * ru) % 2048 != 0 or ru == 2048      # (a row of 2 048 units IS a block's chunk: every block starts a row)
    g = torch.Generator(DEV).manual_seed(ru)
    keep = torch.rand(n, device=DEV, generator=g) < 0.5
    t = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, ru), device=DEV, dtype=torch.int32, generator=g)
    f = torch.randn(n, ru, device=DEV, generator=g)
    ot, of = compact_rows(keep, [t, f])
    assert _same_bits(ot, t[keep]) and _same_bits(of, f[keep])


@pytest.mark.parametrize("rb", [1, 3, 6, 2049])
def test_compact_byte_rows(rb):
    """the byte-unit instantiation (a row size that is no multiple of 4 switches the whole call to it)"""
    from sfgs.compact import compact_rows
    n = 1301
    assert (n * rb) % 2048 != 0
    g = torch.Generator(DEV).manual_seed(rb)
    keep = torch.rand(n, device=DEV, generator=g) < 0.5
    t = torch.randint(0, 255, (n, rb), device=DEV, dtype=torch.uint8, generator=g)
    f = torch.randn(n, 3, device=DEV, generator=g)       # a 12-byte row rides along in byte units
    ot, of = compact_rows(keep, [t, f])
    assert _same_bits(ot, t[keep]) and _same_bits(of, f[keep])


def test_compact_row_size_limit():
    """sfgs_compact_rows promises rows below 2^22 bytes and an error (SFGS_E_ARG through L.check) from there on. The largest
    allowed row (2^20 - 1 words) at N = 3 is gathered bit for bit; a row of exactly 2^22 bytes raises and returns nothing."""
    from sfgs.compact import compact_rows
    g = torch.Generator(DEV).manual_seed(1)
    keep = torch.tensor([True, False, True], device=DEV)
    t = torch.randn(3, 2 ** 20 - 1, device=DEV, generator=g)
    (o,) = compact_rows(keep, [t])
    assert _same_bits(o, t[keep])
    big = torch.randn(3, 2 ** 20, device=DEV, generator=g)
    out = None
    with pytest.raises(RuntimeError, match="bad row size"):
        out = compact_rows(keep, [big])
    assert out is None


# ---- filter3d --------------------------------------------------------------------------------------------------------
def _filter(xyz, cams):
    from types import SimpleNamespace
    from sfgs.filter3d import compute_3D_filter
    out = compute_3D_filter(torch.tensor(xyz, device=DEV), [SimpleNamespace(**c) for c in cams])
    assert out.dtype == torch.float64 and out.shape == (xyz.shape[0], 1)
    return out.cpu().numpy()


@pytest.mark.parametrize("far_last", [True, False])
def test_filter3d_reduce_second_round(far_last):
    """N = 262 144 + 300 = 262 444 points = 1 026 entries of block_max: filter3d_reduce_kernel's 1 024 threads take entries
    1 024 and 1 025 in the second round of their strided loop. The farthest seen point lies in the last block (entry 1 025),
    then in block 0; the unseen points of every block must take its distance."""
    xyz, cams, far = R.filter3d_reduce_case(far_last)
    ref = oracle_filter(xyz, cams)
    got = _filter(xyz, cams)
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    assert (got[::41] == got[far]).all() and got[far] == got.max()


def test_filter3d_camera_counts_and_last_camera():
    """one camera; and a point that only the last of four cameras sees (the loop must not stop early or skip its end)"""
    rng = np.random.default_rng(8)
    n = 257
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, :2] = rng.uniform(-0.5, 0.5, size=(n, 2))
    xyz[:, 2] = rng.uniform(2.0, 9.0, size=n)
    xyz[100] = (40.0, 0.0, 3.0)                      # far off to the side: out of the first three cameras' screens
    cams = [R.camera(T=(0.1 * i, 0.0, 0.2 * i), focal=600.0 + 50 * i) for i in range(3)]
    one = [cams[1]]
    np.testing.assert_allclose(_filter(xyz, one), oracle_filter(xyz, one), rtol=1e-12)
    cams.append(R.camera(T=(-40.0, 0.0, 4.0), focal=500.0))     # looks at that point (depth 7), sees none of the others
    m = [R.filter3d_margins(xyz, c).min(axis=1) > 0 for c in cams]
    assert not m[0][100] and not m[1][100] and not m[2][100] and m[3][100] and m[3].sum() == 1
    ref = oracle_filter(xyz, cams)
    assert ref[100, 0] == 7.0 / 700.0 * R.SQRT02                  # nearest seen depth over the largest focal_x
    np.testing.assert_allclose(_filter(xyz, cams), ref, rtol=1e-12)


@pytest.mark.parametrize("test", R.FILTER_TESTS)
def test_filter3d_thresholds(test):
    """a point a relative 1.5e-9 inside and one outside each of the five tests (z > 0.2, the four 15 % screen margins); never
    ON a threshold, where a fused multiply-add may legitimately fall either way (test_model_ops_ref_cpu.py checks the sides)"""
    for inside in (True, False):
        xyz, cams, seen = R.filter3d_threshold_case(test, inside)
        ref = oracle_filter(xyz, cams)
        got = _filter(xyz, cams)
        np.testing.assert_allclose(got, ref, rtol=1e-12)
        assert (got[0, 0] < got[1, 0]) == seen and (seen or got[0, 0] == got[1, 0])


def test_filter3d_invalid_depths_and_unseen_points():
    """z in (0.001, 0.2): an invalid depth that is projected as it is; z < 0.001 and z < 0: projected with the clamp 0.001;
    all unseen, among seen points whose largest distance they take"""
    xyz = np.asarray([[0.0, 0.0, 5.0], [0.0, 0.0, 0.1], [0.0001, 0.0, 0.0005], [0.0, 0.0, -3.0], [0.01, 0.01, 0.19],
                      [0.3, -0.2, 9.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0009], [1e5, 0.0, 2.0]], np.float32)
    cams = [R.camera(focal=500.0), R.camera(T=(0.0, 0.0, 0.05), focal=450.0)]
    ref = oracle_filter(xyz, cams)
    got = _filter(xyz, cams)
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    assert (got[[1, 2, 3, 6, 7, 8], 0] == got[5, 0]).all() and got[5, 0] == 9.0 / 500.0 * R.SQRT02


def test_filter3d_no_point_seen_by_any_camera():
    """The reference raises here (max of an empty tensor); filter3d_finish_kernel documents the reference's initial distance
    1e8 for every point instead: 1e8 / focal * sqrt(0.2)"""
    xyz = np.asarray([[0.0, 0.0, -1.0], [0.0, 0.0, 0.1], [50.0, 0.0, 1.0]] * 100, np.float32)
    cams = [R.camera(focal=500.0), R.camera(focal=640.0)]
    with pytest.raises(ValueError):
        oracle_filter(xyz, cams)
    got = _filter(xyz, cams)
    assert (got == 1e8 / 640.0 * 0.4472135954999579).all()


# ---- densify_stats ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_max", [True, False])
def test_densify_stats_every_element(with_max):
    """two consecutive calls with different filters at every N of BLOCK_NS; rows with a false filter keep all four buffers
    bit for bit (NaN payloads included), the others are within 2 float32 ulp of the float64 result"""
    from types import SimpleNamespace
    from sfgs.densify_stats import add_densification_stats
    names = [k for k in R.STATS if with_max or k != "xyz_gradient_accum_abs_max"]
    worst = 0.0
    for n in R.BLOCK_NS:
        rng = np.random.default_rng(n)
        bits = (rng.integers(0, 2 ** 22, size=(len(names), n, 1)) | 0x7FC00000).astype(np.uint32)     # NaNs with payloads
        pre = {k: (np.abs(rng.normal(size=(n, 1))) * 10.0 ** rng.uniform(-6, 2) + i).astype(np.float32)
               for i, k in enumerate(names)}
        never = rng.random(n) < 0.2                       # rows no call touches: distinct NaN payloads
        for i, k in enumerate(names):
            pre[k][never] = bits[i][never].view(np.float32)
        model = SimpleNamespace(**{k: torch.tensor(v, device=DEV) for k, v in pre.items()})
        cur = {k: v.copy() for k, v in pre.items()}
        for call in range(2):
            f = (rng.random(n) < 0.5) & ~never
            grad = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-8, 0, size=(n, 1))).astype(np.float32)
            add_densification_stats(model, SimpleNamespace(grad=torch.tensor(grad, device=DEV)), torch.tensor(f, device=DEV))
            ref = R.densify_stats_ref(cur, grad, f)
            for k in names:
                got = getattr(model, k).cpu().numpy()
                assert (got[~f].view(np.uint32) == cur[k][~f].view(np.uint32)).all(), (k, n, call)
                err = np.abs(got[f].astype(np.float64) - ref[k][f]) / R.ulp32(ref[k][f])
                worst = max(worst, float(err.max()) if err.size else 0.0)
                assert (err <= 2).all(), (k, n, call, float(err.max()))
                cur[k] = got.copy()
        assert (getattr(model, names[0]).cpu().numpy()[never].view(np.uint32) == bits[0][never]).all()
    print(f"UNITS densify_stats ulp {worst:.4g} with_max {with_max}")


# ---- distCUDA2, the brute-force kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1023, 1024, 1025, 2049, 32768])
def test_distcuda2_brute_force_tile_edges(n):
    """knn_dist2_kernel stages KNN_TILE = 1 024 points per round and excludes the query by its index `i - base` inside the
    tile: one partial tile, one full tile, a second tile of one point, a third of one point, and KNN_BRUTE_MAX = 32 768 (32
    whole tiles), the largest n the kernel is chosen for. The duplicate points straddle a tile edge: distance 0 counts."""
    from simple_knn._C import distCUDA2
    rng = np.random.default_rng(n)
    pts = rng.normal(size=(n, 3)).astype(np.float32) * 3
    if n > 1024:
        pts[1024] = pts[1023]
        pts[n - 1] = pts[0]
    got = distCUDA2(torch.tensor(pts, device=DEV)).cpu().numpy()
    ref = orc.knn_dist2(pts)
    assert got.shape == (n,)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-9)
