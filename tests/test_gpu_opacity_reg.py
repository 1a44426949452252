"""GPU tests of sfgs.loss.opacity_entropy (csrc/opacity_reg.hip) and of sfgs.opacity_reg: the opacity regulariser of
train.py:236-242 against the reference's own run (tests/golden/make_golden_opacity_reg.py) and against R64, the formula in
float64 on the CPU:

    o = sigmoid(x), c = min(max(o, lo), hi), inside = (lo <= o <= hi), lo / hi rounded to x's dtype
    value = mean -(c log c + (1 - c) log(1 - c));  dvalue/dx = (log(1 - c) - log c) * inside * o (1 - o) / N

The bars. float32: the fused result may be at most TWICE as far from R64 as torch's own float32 spelling of the three
statements, run on the GPU on the same input (and no closer than 2^-23 relative has to be asked of either) -- for the value
|v - R64| <= 2 max(|v_torch - R64|, 2^-23 |R64|), for the gradient the same with max-norms. The factor 2: the two sides use
different but equally good exp / log. float64: value and gradient within 1e-12 relative of R64 (the gradient relative to
max |grad|). Inputs stay 0.01 away from the clamp's thresholds |x| = 6.906755, where the gradient jumps and the side an
element falls on is not reproducible between two exp implementations; the one test that goes there accepts either side."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sfgs import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_opacity_reg.npz")
LO, HI = 1.0e-3, 1.0 - 1.0e-3
THRESHOLD = math.log(HI / LO)   # 6.906755
BAND = 0.01
EPS32 = 2.0 ** -23
DTYPES = {"f32": torch.float32, "f64": torch.float64}
KERNELS = ("opacity_entropy_fwd", "opacity_entropy_final", "opacity_entropy_bwd")


# ---- references ------------------------------------------------------------------------------------------------------------
def r64(x, lo=LO, hi=HI, inside_everywhere=False):
    """The formula in float64 on the CPU. x: a tensor of the dtype under test. -> (value, gradient as a float64 array)"""
    lo, hi = (torch.tensor(v, dtype=x.dtype).item() for v in (lo, hi))
    x = x.detach().cpu().double().reshape(-1)
    o = torch.sigmoid(x)
    c = torch.minimum(torch.maximum(o, torch.tensor(lo, dtype=torch.float64)), torch.tensor(hi, dtype=torch.float64))
    inside = torch.ones_like(o) if inside_everywhere else ((o >= lo) & (o <= hi)).double()
    value = -(c * torch.log(c) + (1.0 - c) * torch.log1p(-c)).mean()
    grad = (torch.log1p(-c) - torch.log(c)) * inside * o * (1.0 - o) / x.numel()
    return value.item(), grad.numpy()


def torch_spelling(x, weight=1.0):
    """train.py:239-242 as torch runs them on the GPU, on a copy of x -> (value, gradient)"""
    x = x.detach().clone().requires_grad_(True)
    opacity = torch.sigmoid(x).clamp(LO, HI)
    opacity_loss = F.binary_cross_entropy(opacity, opacity)
    (weight * opacity_loss).backward()
    return opacity_loss.detach(), x.grad


def raw_opacities(n, dtype, seed):
    """[n] raw opacities as in the fixture: uniform [-12, 12] and a normal bulk, none within BAND of the thresholds."""
    g = torch.Generator().manual_seed(seed)

    def draw():
        u = torch.rand(n, generator=g, dtype=dtype) * 24.0 - 12.0
        z = torch.randn(n, generator=g, dtype=dtype) * 2.5
        return torch.where(torch.arange(n) % 2 == 0, u, z)
    x = draw()
    while True:
        bad = (x.abs() - THRESHOLD).abs() < BAND
        if not bad.any():
            return x
        x = torch.where(bad, draw(), x)


def fused(x, weight=None):
    """opacity_entropy on x (made a leaf here) -> (value, gradient)"""
    from sfgs.loss import opacity_entropy
    x = x.detach().requires_grad_(True)
    value = opacity_entropy(x)
    (value if weight is None else weight * value).backward()
    return value.detach(), x.grad


def check_against_bars(tag, x, value, grad, v_other, g_other, skip=None):
    """value / grad: the fused result; v_other / g_other: torch's float32 spelling on the GPU (or the reference's recorded
    run) on the same input. Prints every figure, then asserts the bars of the module text. skip: elements left out."""
    v64, g64 = r64(x)
    keep = np.ones(g64.shape, bool) if skip is None else ~skip
    assert value.dtype == x.dtype and grad.dtype == x.dtype and grad.shape == x.shape and value.dim() == 0
    v, g = float(value), grad.detach().cpu().double().numpy().reshape(-1)
    vo, go = float(v_other), np.asarray(g_other, dtype=np.float64).reshape(-1)
    ev, evo = abs(v - v64), abs(vo - v64)
    eg, ego = np.abs(g - g64)[keep].max(), np.abs(go - g64)[keep].max()
    gmax = np.abs(g64).max()
    print(f"{tag}: value err {ev:.3e} (other {evo:.3e}, |R64| {abs(v64):.3e});  grad err {eg:.3e} (other {ego:.3e}, "
          f"max|R64| {gmax:.3e})")
    if x.dtype == torch.float32:
        assert ev <= 2.0 * max(evo, EPS32 * abs(v64)), (tag, ev, evo)
        assert eg <= 2.0 * max(ego, EPS32 * gmax), (tag, eg, ego)
    else:
        assert ev <= 1e-12 * abs(v64), (tag, ev)
        assert eg <= 1e-12 * gmax, (tag, eg)
    return v64, g64


def launches(fn):
    """-> (fn(), {kernel: launches} of the library's kernels while it ran)"""
    L.profile_enable(True)
    try:
        L.profile_collect()
        res = fn()
        return res, {k: v[1] for k, v in L.profile_collect().items()}
    finally:
        L.profile_enable(False)


# ---- 1. the reference's own run (golden) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_golden(tag):
    G = np.load(GOLDEN)
    x = torch.tensor(G[f"{tag}_x"], device=DEV)
    assert x.dtype == DTYPES[tag] and tuple(x.shape) == (4099, 1)
    value, grad = fused(x)
    check_against_bars(f"golden {tag}", x, value, grad, G[f"{tag}_value"], G[f"{tag}_grad"])


# ---- 2. sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("column", [False, True], ids=["N", "Nx1"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 1025, 100_003, 2_000_000])
def test_sweep(n, tag, column, misaligned):
    dtype = DTYPES[tag]
    if misaligned:                                   # base[1:]: 4 or 8 bytes past a 16-byte boundary -> the scalar path
        base = torch.cat([torch.zeros(1, dtype=dtype), raw_opacities(n, dtype, seed=n + 1)]).to(DEV)
        x = base[1:]
        assert x.data_ptr() % 16 != 0
    else:
        x = raw_opacities(n, dtype, seed=n).to(DEV)
        assert x.data_ptr() % 16 == 0
    if column:
        x = x.view(n, 1)
    value, grad = fused(x)
    v_torch, g_torch = torch_spelling(x)
    check_against_bars(f"sweep n={n} {tag} {'Nx1' if column else 'N'} {'misaligned' if misaligned else 'aligned'}", x, value,
                       grad, v_torch, g_torch.cpu().numpy())


# ---- 3. upstream gradient, and no backward launch when nothing needs one -----------------------------------------------------------
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_upstream_gradient_is_honoured(tag):
    x = raw_opacities(100_003, DTYPES[tag], seed=5).to(DEV)
    _, g1 = fused(x)
    _, g75 = fused(x, weight=7.5)
    _, g64 = r64(x)
    _, g75_torch = torch_spelling(x, weight=7.5)
    err = np.abs(g75.cpu().double().numpy() - 7.5 * g64).max()
    err_torch = np.abs(g75_torch.cpu().double().numpy() - 7.5 * g64).max()
    gmax = 7.5 * np.abs(g64).max()
    print(f"upstream 7.5 {tag}: err {err:.3e} (torch {err_torch:.3e}), max {gmax:.3e}")
    assert err <= (2.0 * max(err_torch, EPS32 * gmax) if tag == "f32" else 1e-12 * gmax)
    # and against the library's own unit-gradient result: one more rounding of each side
    rel = 2.0 ** -22 if tag == "f32" else 2.0 ** -51
    assert float((g75 - 7.5 * g1).abs().max()) <= rel * gmax


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_no_backward_kernel_without_a_gradient_to_compute(tag):
    from sfgs.loss import opacity_entropy
    x = raw_opacities(100_003, DTYPES[tag], seed=6).to(DEV)
    v64, _ = r64(x)
    want, _ = fused(x)
    for how in ("no_grad", "requires_grad_false"):
        if how == "no_grad":
            leaf = x.clone().requires_grad_(True)
            with torch.no_grad():
                value, counts = launches(lambda: opacity_entropy(leaf))
        else:
            value, counts = launches(lambda: opacity_entropy(x))
        assert counts == {"opacity_entropy_fwd": 1, "opacity_entropy_final": 1}, how
        assert not value.requires_grad and value.grad_fn is None
        assert torch.equal(value, want) and abs(float(value) - v64) <= 2.0 * EPS32 * abs(v64)
    # a graph in which the regulariser's input needs no gradient but another term does
    w = torch.ones((), dtype=x.dtype, device=DEV, requires_grad=True)
    total = opacity_entropy(x) * w
    _, counts = launches(total.backward)
    assert counts == {} and torch.equal(w.grad, want)


# ---- 4. bit-reproducible -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_bit_reproducible(tag):
    x = raw_opacities(2_000_000, DTYPES[tag], seed=9).to(DEV)
    v0, g0 = fused(x)
    for _ in range(3):
        v, g = fused(x)
        assert torch.equal(v, v0) and torch.equal(g, g0)
        assert v.view(torch.int32 if tag == "f32" else torch.int64).item() == \
            v0.view(torch.int32 if tag == "f32" else torch.int64).item()


# ---- 5. launch counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("n", [3, 2_000_000])
def test_launch_counts(n, tag):
    from sfgs.loss import opacity_entropy
    x = raw_opacities(n, DTYPES[tag], seed=2).to(DEV).requires_grad_(True)
    value, fwd = launches(lambda: opacity_entropy(x))
    _, bwd = launches(value.backward)
    assert fwd == {"opacity_entropy_fwd": 1, "opacity_entropy_final": 1}
    assert bwd == {"opacity_entropy_bwd": 1}


# ---- 6. no host synchronisation ----------------------------------------------------------------------------------------------------
def test_opacity_entropy_does_not_synchronise_the_host():
    from sfgs.loss import opacity_entropy
    x32 = raw_opacities(2_000_000, torch.float32, seed=3).to(DEV).requires_grad_(True)
    x64 = raw_opacities(2_000_000, torch.float64, seed=4).to(DEV).requires_grad_(True)
    big = torch.randn(8192, 8192, device=DEV)
    for x in (x32, x64):                                            # warm-up: library load, allocator
        (10.0 * opacity_entropy(x)).backward()
    big @ big
    x32.grad = x64.grad = None
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    honoured = False
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(40):                                           # a long queue in front of the regulariser
            big @ big
        for x in (x32, x64):
            value = opacity_entropy(x)
            (10.0 * value).backward()
        done.record()
        returned_early = not done.query()       # the calls came back while the queue in front of them was still running
        try:
            value.item()
        except RuntimeError:
            honoured = True                     # this build raises on a synchronising call: the block above made none
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    print(f"sync debug mode honoured by this torch build: {honoured}; returned before the queue drained: {returned_early}")
    assert returned_early
    assert torch.isfinite(value) and torch.isfinite(x32.grad).all() and torch.isfinite(x64.grad).all()


# ---- 7. the threshold band -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_threshold_band_elements_take_either_branch(tag):
    """4 096 values within +-0.01 of +-6.906755 among ordinary ones. Which side of the clamp such an element falls on is
    decided by the last bits of exp, so each one's gradient has to be, within the bar, either 0 (outside) or the inside
    branch's value; every other element, and the value (h is continuous across the threshold), meet the usual bars."""
    dtype = DTYPES[tag]
    n, k = 20_000, 4096
    g = torch.Generator().manual_seed(77)
    x = raw_opacities(n, dtype, seed=7)
    where = torch.randperm(n, generator=g)[:k]
    sign = torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0).to(dtype)
    offs = (torch.rand(k, generator=g, dtype=dtype) * 2.0 - 1.0) * BAND
    offs[:64] = offs[:64] * 1e-5                                      # some of them within a few ulps of the threshold
    x[where] = sign * (THRESHOLD + offs)
    band = np.zeros(n, bool)
    band[where.numpy()] = True
    x = x.to(DEV)
    value, grad = fused(x)
    v_torch, g_torch = torch_spelling(x)
    _, g64 = check_against_bars(f"band {tag}", x, value, grad, v_torch, g_torch.cpu().numpy(), skip=band)
    _, g_inside = r64(x, inside_everywhere=True)
    got, gt = grad.cpu().double().numpy(), g_torch.cpu().double().numpy()
    gmax = np.abs(g64).max()
    if tag == "f32":
        bar = 2.0 * max(np.abs(gt - g64)[~band].max(), EPS32 * gmax)
    else:
        bar = 1e-12 * gmax
    d_out, d_in = np.abs(got[band]), np.abs(got[band] - g_inside[band])
    n_in = int((d_in <= bar).sum())
    print(f"band {tag}: bar {bar:.3e}; of {k} band elements {n_in} took the inside branch, "
          f"{int((d_out <= bar).sum())} the outside one; worst distance to the nearer {np.minimum(d_out, d_in).max():.3e}")
    assert (np.minimum(d_out, d_in) <= bar).all()
    assert 0 < n_in < k                                               # the band straddles the threshold: both occur


# ---- 8. NaN and +-Inf ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_nan_and_inf_inputs(tag):
    """+-Inf: compared with torch's spelling on the GPU. NaN: torch's spelling cannot be run on it -- its
    binary_cross_entropy kernel asserts 0 <= input <= 1 on the device, and on ROCm a failed device assertion aborts the
    kernel (a GPU fault, not a NaN; the CPU kernel raises "all elements of input should be between 0 and 1"). So WHERE the
    NaNs must be is taken from R64 (the value; the gradient elements of the NaN inputs and no others), and torch's own error
    for the finite gradient elements is measured on the same input with the NaN elements replaced by 0 (an element's
    gradient depends on its own x and on N only)."""
    dtype = DTYPES[tag]
    n = 10_007
    x = raw_opacities(n, dtype, seed=8)
    nan_at, pinf_at, ninf_at = [5, 4099, n - 1], [0, 777, 4100], [1, 6000]
    x_inf = x.clone()
    x_inf[pinf_at], x_inf[ninf_at] = float("inf"), float("-inf")
    x_nan = x_inf.clone()
    x_nan[nan_at] = float("nan")
    # +-Inf only: a finite value within the bar, zero gradient there
    xd = x_inf.to(DEV)
    value, grad = fused(xd)
    v_torch, g_torch = torch_spelling(xd)
    assert torch.isfinite(v_torch) and torch.isfinite(g_torch).all()
    check_against_bars(f"inf {tag}", xd, value, grad, v_torch, g_torch.cpu().numpy())
    assert torch.isfinite(value) and (grad[pinf_at + ninf_at] == 0).all()
    # with NaN
    xd = x_nan.to(DEV)
    value, grad = fused(xd)
    v64, g64 = r64(xd)
    is_nan = np.zeros(n, bool)
    is_nan[nan_at] = True
    assert math.isnan(v64) and (np.isnan(g64) == is_nan).all()
    assert torch.isnan(value)
    assert (torch.isnan(grad).cpu().numpy() == is_nan).all()
    assert not torch.isinf(grad).any()
    _, g_torch = torch_spelling(torch.nan_to_num(x_nan, nan=0.0, posinf=float("inf"), neginf=float("-inf")).to(DEV))
    got, gt = grad.cpu().double().numpy(), g_torch.cpu().double().numpy()
    gmax = np.abs(g64[~is_nan]).max()
    err, err_torch = np.abs(got - g64)[~is_nan].max(), np.abs(gt - g64)[~is_nan].max()
    print(f"nan {tag}: finite grad err {err:.3e} (torch {err_torch:.3e}), max {gmax:.3e}")
    assert err <= (2.0 * max(err_torch, EPS32 * gmax) if tag == "f32" else 1e-12 * gmax)


# ---- 9. sfgs.opacity_reg.install on a stand-in GaussianModel --------------------------------------------------------------------
def make_model_class():
    from oracle.prepass_torch import prepass_reference

    class GaussianModel:   # the attribute / property names of scene/gaussian_model.py
        def __init__(self, n, dtype, seed=0):
            g = torch.Generator().manual_seed(seed)
            self._scaling = (torch.randn(n, 3, generator=g) - 2).to(DEV).requires_grad_(True)
            self._rotation = torch.randn(n, 4, generator=g).to(DEV).requires_grad_(True)
            self.filter_3D = torch.exp(torch.randn(n, 1, generator=g, dtype=torch.float64) - 3).to(DEV)
            self._opacity = torch.nn.Parameter(raw_opacities(n, dtype, seed + 100).view(n, 1).to(DEV))

        @property
        def get_opacity(self):                       # :234
            return torch.sigmoid(self._opacity)

        @property
        def get_scaling_with_3D_filter(self):
            return prepass_reference(self._scaling, self._opacity, self._rotation, self.filter_3D)[0]

        @property
        def get_opacity_with_3D_filter(self):
            return prepass_reference(self._scaling, self._opacity, self._rotation, self.filter_3D)[1]

        @property
        def get_rotation(self):
            return prepass_reference(self._scaling, self._opacity, self._rotation, self.filter_3D)[2]
    return GaussianModel


def regulariser_statements(gaussians, lambda_opacity=10.0):
    """train.py:239-242 (and :837-843), unchanged"""
    loss = torch.zeros((), dtype=gaussians._opacity.dtype, device=DEV)
    opacity = gaussians.get_opacity.clamp(1.0e-3, 1.0 - 1.0e-3)
    opacity_loss = torch.nn.functional.binary_cross_entropy(opacity, opacity)
    loss += lambda_opacity * opacity_loss
    return loss, opacity_loss


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_install_runs_the_unchanged_statements_on_the_three_kernels(tag):
    from sfgs import opacity_reg
    cls = make_model_class()
    n = 100_003
    plain, gaussians = cls(n, DTYPES[tag]), cls(n, DTYPES[tag])
    loss_0, value_0 = regulariser_statements(plain)
    loss_0.backward()
    orig = cls.__dict__["get_opacity"]
    opacity_reg.install(cls)
    try:
        before = opacity_reg.materialisations
        (loss, value), fwd = launches(lambda: regulariser_statements(gaussians))
        _, bwd = launches(loss.backward)
        assert fwd == {"opacity_entropy_fwd": 1, "opacity_entropy_final": 1}
        assert bwd == {"opacity_entropy_bwd": 1}
        assert opacity_reg.materialisations == before                 # the handle never became a tensor
        # lambda_opacity = 10 arrives as the upstream gradient: compare the gradients of 10 * value
        x = gaussians._opacity.detach()
        v64, g64 = r64(x)
        g, g0 = gaussians._opacity.grad, plain._opacity.grad
        assert g.dtype == x.dtype and g.shape == x.shape
        ev, ev0 = abs(float(value.detach()) - v64), abs(float(value_0.detach()) - v64)
        eg = np.abs(g.cpu().double().numpy().reshape(-1) - 10.0 * g64).max()
        eg0 = np.abs(g0.cpu().double().numpy().reshape(-1) - 10.0 * g64).max()
        gmax = 10.0 * np.abs(g64).max()
        print(f"install {tag}: value err {ev:.3e} (unpatched {ev0:.3e});  grad err {eg:.3e} (unpatched {eg0:.3e}), max {gmax:.3e}")
        if tag == "f32":
            assert ev <= 2.0 * max(ev0, EPS32 * abs(v64)) and eg <= 2.0 * max(eg0, EPS32 * gmax)
        else:
            assert ev <= 1e-12 * abs(v64) and eg <= 1e-12 * gmax
    finally:
        opacity_reg.uninstall(cls)
    assert cls.__dict__["get_opacity"] is orig


OTHER_CONSUMERS = {
    "prune_mask": lambda o: (o < 0.005).squeeze(),                                           # gaussian_model.py:731
    "reset_opacity": lambda o: torch.min(o, torch.ones_like(o) * 0.01),                      # gaussian_model.py:485
    "other_target": lambda o: (lambda c: F.binary_cross_entropy(c, torch.full_like(c, 0.25)))(o.clamp(LO, HI)),
    "reduction_sum": lambda o: (lambda c: F.binary_cross_entropy(c, c, reduction="sum"))(o.clamp(LO, HI)),
}


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("use", sorted(OTHER_CONSUMERS))
def test_install_leaves_every_other_consumer_in_torch(use, tag):
    from sfgs import opacity_reg
    cls = make_model_class()
    fn = OTHER_CONSUMERS[use]
    plain, gaussians = cls(4099, DTYPES[tag]), cls(4099, DTYPES[tag])
    want = fn(plain.get_opacity)
    opacity_reg.install(cls)
    try:
        before = opacity_reg.materialisations
        got, counts = launches(lambda: fn(gaussians.get_opacity))
        assert not any(k in counts for k in KERNELS), counts
        assert opacity_reg.materialisations > before
        assert type(got) is torch.Tensor and got.dtype == want.dtype and torch.equal(got, want)
        if want.requires_grad:
            _, counts = launches(got.sum().backward)
            assert not any(k in counts for k in KERNELS), counts
            want.sum().backward()
            assert torch.equal(gaussians._opacity.grad, plain._opacity.grad)
    finally:
        opacity_reg.uninstall(cls)


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_install_together_with_the_prepass_hook(tag):
    """Both hooks on one class: `_opacity` receives the gradient of get_opacity_with_3D_filter.sum() (the fused pre-pass)
    plus the regulariser's. The bound on the sum is the sum of the two parts' bounds: the pre-pass's committed one
    (tests/test_prepass.py: 3e-6 of its largest gradient element) and the regulariser's bar of 2 against the unpatched
    class's own error -- both measured against the float64 formulas on the CPU."""
    from sfgs import opacity_reg, prepass
    cls = make_model_class()
    n = 4099
    plain, gaussians = cls(n, DTYPES[tag]), cls(n, DTYPES[tag])

    def objective(m):
        return m.get_opacity_with_3D_filter.sum() + regulariser_statements(m)[0]
    objective(plain).backward()
    prepass.install(cls)
    opacity_reg.install(cls)
    try:
        total, counts = launches(lambda: objective(gaussians))
        _, counts_bwd = launches(total.backward)
        assert counts.get("opacity_entropy_fwd") == 1 and counts.get("opacity_entropy_final") == 1
        assert counts_bwd.get("opacity_entropy_bwd") == 1 and counts_bwd.get("prepass_bwd") == 1
    finally:
        opacity_reg.uninstall(cls)
        prepass.uninstall(cls)
    x = gaussians._opacity.detach()
    _, g_reg = r64(x)
    s2 = torch.exp(gaussians._scaling.detach().cpu().double()) ** 2
    coef = torch.sqrt(s2.prod(dim=1) / (s2 + gaussians.filter_3D.cpu().double() ** 2).prod(dim=1))
    o = torch.sigmoid(x.cpu().double().reshape(-1))
    g_pre = (coef * o * (1.0 - o)).numpy()
    g64 = g_pre + 10.0 * g_reg
    got = gaussians._opacity.grad.cpu().double().numpy().reshape(-1)
    unpatched = plain._opacity.grad.cpu().double().numpy().reshape(-1)
    err, err0 = np.abs(got - g64).max(), np.abs(unpatched - g64).max()
    floor = EPS32 if tag == "f32" else 2.0 ** -52
    bound = 3e-6 * np.abs(g_pre).max() + 2.0 * max(err0, floor * np.abs(g64).max())
    print(f"with prepass {tag}: err {err:.3e} (unpatched {err0:.3e}), bound {bound:.3e}; regulariser's share of the "
          f"gradient up to {10.0 * np.abs(g_reg).max():.3e}")
    assert gaussians._opacity.grad.dtype == x.dtype
    assert err <= bound
    assert 10.0 * np.abs(g_reg).max() > 100.0 * bound                 # the bound would notice a missing regulariser
