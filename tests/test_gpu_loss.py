"""GPU tests of sfgs.loss (csrc/loss.hip): the fused training loss -- masked L1 + D-SSIM + Pearson depth term -- against
the golden vectors from the reference's own utils/loss_utils (tests/golden/make_golden_loss.py), the SSIM oracle, a float64
torch restatement of the Pearson term, fused_ssim (bit for bit) and its own composition from halves; launch counts and the
absence of host synchronisation; the l1_loss / pearson_corrcoef drop-ins and install()."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from sfgs import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_loss.npz")


# ---- references ------------------------------------------------------------------------------------------------------------
def pearson64(gt_depth, depth, mask, invalid):
    """train.py:207-211, 227-232 (invalid="zero") / :786-791 ("drop") and torchmetrics' _pearson_corrcoef_compute in
    float64 on the CPU. -> (1 - r, d(1 - r)/d depth, the scrubbed pairs) -- which pairs are scrubbed is decided on the
    float32 products with the mask, like the reference does; everything else is float64."""
    gt_depth, depth = gt_depth.detach().cpu(), depth.detach().cpu()
    m = torch.ones(1, 1, 1) if mask is None else mask.detach().cpu()
    bad = ~(torch.isfinite(m * gt_depth) & torch.isfinite(m * depth)).reshape(-1)
    d64 = depth.double().requires_grad_(True)
    a = (m * gt_depth).double().reshape(-1)
    b = (m.double() * d64).reshape(-1)
    if invalid == "zero":
        a = torch.where(bad, torch.zeros_like(a), a)
        b = torch.where(bad, torch.zeros_like(b), b)
    else:
        a, b = a[~bad], b[~bad]
    ac, bc = a - a.mean(), b - b.mean()
    r = ((ac * bc).sum() / ((ac * ac).sum() * (bc * bc).sum()).sqrt()).clamp(-1.0, 1.0)
    val = 1.0 - r
    if torch.isfinite(val):
        val.backward()
    grad = d64.grad if d64.grad is not None else torch.zeros_like(d64)
    return float(val.detach()), grad.numpy(), bad.reshape(depth.shape).numpy()


def depth_pair(h, w, seed, mean=400.0, spread=20.0, nan_frac=0.03, infs=5):
    """gt = mean + spread * randn; depth = 0.9 gt + noise + offset (400 +- 20: 6 randn + 7); NaN planted in `nan_frac` of
    depth and a few +-Inf in gt."""
    g = torch.Generator().manual_seed(seed)
    gt = mean + spread * torch.randn(1, h, w, generator=g)
    depth = 0.9 * gt + 0.3 * spread * torch.randn(1, h, w, generator=g) + 7.0 * spread / 20.0
    depth.view(-1)[torch.rand(h * w, generator=g) < nan_frac] = float("nan")
    idx = torch.randint(0, h * w, (infs,), generator=g)
    gt.view(-1)[idx] = torch.tensor([float("inf"), float("-inf")]).repeat(infs)[:infs]
    return gt, depth


def make_mask(kind, h, w, seed):
    g = torch.Generator().manual_seed(seed + 77)
    if kind == "none":
        return None
    if kind == "ones1":
        return torch.ones(1, 1, 1)
    if kind == "binary":
        return (torch.rand(1, h, w, generator=g) < 0.7).float()
    return torch.rand(1, h, w, generator=g)   # fractional


def image_pair(c, h, w, seed, noise=0.1):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(c, h, w, generator=g)
    b = (a + noise * torch.randn(c, h, w, generator=g)).clamp(0, 1)
    return a, b


def to_dev(t):
    return None if t is None else t.to(DEV)


# ---- 1. the reference's own functions (golden) --------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_training_loss_matches_reference_golden(tag):
    from sfgs.loss import training_loss
    G = np.load(GOLDEN)
    lam, lamd = float(G[f"{tag}_lambda_dssim"]), float(G[f"{tag}_lambda_depth"])
    image = torch.tensor(G[f"{tag}_image"], device=DEV, requires_grad=True)
    depth = torch.tensor(G[f"{tag}_depth"], device=DEV, requires_grad=True)
    gt_image, gt_depth, mask = (torch.tensor(G[f"{tag}_{k}"], device=DEV) for k in ("gt_image", "gt_depth", "mask"))
    loss, Ll1, ssim, depth_loss = training_loss(image, depth, gt_image, gt_depth, mask, lam, lamd)
    print(f"golden {tag}: ssim {ssim.item() - float(G[f'{tag}_ssim']):+.3e}  Ll1 rel "
          f"{Ll1.item() / float(G[f'{tag}_Ll1']) - 1:+.3e}  depth_loss {depth_loss.item() - float(G[f'{tag}_depth_loss']):+.3e}")
    assert abs(ssim.item() - float(G[f"{tag}_ssim"])) < 2e-6
    assert abs(Ll1.item() - float(G[f"{tag}_Ll1"])) <= 1e-6 * abs(float(G[f"{tag}_Ll1"]))
    # the depth term as in the Pearson test below: the float64 restatement is the reference, and the golden (the same
    # formula in float32, as train.py runs it) has to agree with it within the same bars
    d64, g64, bad = pearson64(gt_depth, depth, mask, "zero")
    assert abs(float(G[f"{tag}_depth_loss"]) - d64) <= 2.4e-7
    assert abs(depth_loss.item() - d64) <= 2.4e-7
    # image gradient: of the photometric part alone (autograd's through l1_loss and ssim), then of the whole loss
    ((1.0 - lam) * Ll1 + lam * (1.0 - ssim)).backward(retain_graph=True)
    ref = G[f"{tag}_image_grad"]
    got = image.grad.cpu().numpy()
    print(f"golden {tag}: image grad err / max {np.abs(got - ref).max() / np.abs(ref).max():.3e}")
    assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-10
    assert depth.grad is None or (depth.grad == 0).all()
    image.grad = depth.grad = None
    loss.backward()
    got = image.grad.cpu().numpy()
    assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-10
    gd, gd_ref = depth.grad.cpu().numpy(), lamd * g64
    print(f"golden {tag}: depth grad err / max {np.abs(gd - gd_ref).max() / np.abs(gd_ref).max():.3e}  (golden's own: "
          f"{np.abs(G[f'{tag}_depth_grad'] - gd_ref).max() / np.abs(gd_ref).max():.3e})")
    assert np.abs(gd - gd_ref).max() <= 1e-5 * np.abs(gd_ref).max()
    assert np.abs(G[f"{tag}_depth_grad"] - gd_ref).max() <= 1e-5 * np.abs(gd_ref).max()
    assert (gd[bad] == 0).all() and bad.any()
    assert abs(loss.item() - float(G[f"{tag}_loss"])) <= 2e-6


# ---- 2. photometric term against the SSIM oracle + numpy ------------------------------------------------------------------------
# the C, H, W of tests/test_gpu_ops.py's tile-boundary list
SHAPES = [(1, 1, 1), (1, 1, 7), (2, 5, 3), (1, 4, 43), (1, 21, 31), (3, 22, 32), (1, 23, 33), (2, 44, 64), (3, 45, 65),
          (1, 100, 37), (1, 67, 130), (1, 11, 200)]


@pytest.mark.parametrize("mask_kind", ["none", "ones1", "binary", "fractional"])
@pytest.mark.parametrize("shape", SHAPES)
def test_photometric_against_oracle_at_tile_boundaries(shape, mask_kind):
    from sfgs.loss import photometric
    c, h, w = shape
    a, b = image_pair(c, h, w, h * 1000 + w)
    mask = make_mask(mask_kind, h, w, h * 1000 + w)
    m = np.ones((1, 1, 1), np.float32) if mask is None else mask.numpy()
    xm, ym = (m * a.numpy()).astype(np.float32), (m * b.numpy()).astype(np.float32)
    val, _, grad = orc.ssim(xm[None], ym[None], want_grad=True)
    grad = m * grad[0]
    l1 = np.abs(xm.astype(np.float64) - ym.astype(np.float64)).mean()
    l1_grad = m * np.sign(xm - ym) / xm.size
    x = a.to(DEV).requires_grad_(True)
    Ll1, ssim = photometric(x, b.to(DEV), to_dev(mask))
    assert Ll1.shape == () and ssim.shape == ()
    print(f"{shape} {mask_kind}: ssim {ssim.item() - val:+.3e}  Ll1 {Ll1.item() - l1:+.3e} of {l1:.3e}")
    assert abs(ssim.item() - val) < 2e-6
    assert abs(Ll1.item() - l1) <= 1e-6 * l1
    ssim.backward(retain_graph=True)
    got = x.grad.cpu().numpy()
    assert np.abs(got - grad).max() <= 5e-5 * np.abs(grad).max() + 1e-9      # every pixel
    x.grad = None
    Ll1.backward()
    got = x.grad.cpu().numpy()
    assert np.abs(got - l1_grad).max() <= 1e-6 * np.abs(l1_grad).max()
    # without autograd: the derivative maps are not written, the values are the same bits
    with torch.no_grad():
        Ll1_n, ssim_n = photometric(a.to(DEV), b.to(DEV), to_dev(mask))
    assert torch.equal(Ll1_n, Ll1.detach()) and torch.equal(ssim_n, ssim.detach())


# ---- 3. Pearson term against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invalid", ["zero", "drop"])
@pytest.mark.parametrize("family", ["400pm20", "30pm8"])
@pytest.mark.parametrize("size", [(67, 130), (270, 480), (1080, 1920)])
def test_depth_pearson_against_float64(size, family, invalid):
    from sfgs.loss import depth_pearson
    h, w = size
    if family == "400pm20":   # NaN in 1 ... 5 % of depth, by size
        gt, depth = depth_pair(h, w, h + w, 400.0, 20.0, nan_frac={67: 0.01, 270: 0.03, 1080: 0.05}[h])
    else:
        gt, depth = depth_pair(h, w, h + w + 1, 30.0, 8.0, nan_frac=0.30)
    ref, gref, bad = pearson64(gt, depth, None, invalid)
    d = depth.to(DEV).requires_grad_(True)
    val = depth_pearson(d, gt.to(DEV), None, invalid)
    val.backward()
    got = d.grad.cpu().numpy()
    print(f"{size} {family} {invalid}: bad {bad.mean():.3f}  |r - r64| {abs(val.item() - ref):.3e}  "
          f"grad err / max {np.abs(got - gref).max() / np.abs(gref).max():.3e}")
    assert val.shape == () and abs(val.item() - ref) <= 2.4e-7
    assert np.abs(got - gref).max() <= 1e-5 * np.abs(gref).max()
    assert bad.any() and (got[bad] == 0).all()            # scrubbed / dropped pixels: exactly 0
    assert np.isfinite(got).all()


@pytest.mark.parametrize("invalid", ["zero", "drop"])
@pytest.mark.parametrize("mask_kind", ["ones1", "binary"])
def test_depth_pearson_with_a_mask_against_float64(mask_kind, invalid):
    from sfgs.loss import depth_pearson
    h, w = 135, 241                                         # H * W is odd: the 16-byte route's tail elements
    gt, depth = depth_pair(h, w, 11)
    mask = make_mask(mask_kind, h, w, 11)
    ref, gref, bad = pearson64(gt, depth, mask, invalid)
    d = depth.to(DEV).requires_grad_(True)
    val = depth_pearson(d, gt.to(DEV), to_dev(mask), invalid)
    val.backward()
    got = d.grad.cpu().numpy()
    assert abs(val.item() - ref) <= 2.4e-7
    assert np.abs(got - gref).max() <= 1e-5 * np.abs(gref).max()
    assert (got[bad] == 0).all()
    if mask_kind == "binary":
        assert (got[mask.numpy() == 0] == 0).all()


def test_depth_pearson_degenerate_inputs_do_not_fault():
    from sfgs.loss import depth_pearson
    h, w = 67, 130
    gt, _ = depth_pair(h, w, 3)
    # every pair bad: "drop" leaves n = 0 -> 0 / 0 = NaN as in torch (train.py:792 tests for it); gradient exactly 0
    d = torch.full((1, h, w), float("nan"), device=DEV, requires_grad=True)
    val = depth_pearson(d, gt.to(DEV), None, "drop")
    val.backward()
    assert torch.isnan(val) and (d.grad == 0).all()
    # "zero": every pair (0, 0): a constant -> NaN as well
    assert torch.isnan(depth_pearson(d.detach(), gt.to(DEV), None, "zero"))
    # a constant depth: must not fault; the value depends on rounding (in torch as well) and is not checked
    c = torch.full((1, h, w), 412.5, device=DEV, requires_grad=True)
    val = depth_pearson(c, torch.nan_to_num(gt, posinf=0.0, neginf=0.0).to(DEV), None, "zero")
    val.backward()
    torch.cuda.synchronize()
    assert c.grad.shape == c.shape


# ---- 4. bit checks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 270, 480), (3, 45, 65), (1, 23, 33)])
def test_ssim_half_is_bit_identical_to_fused_ssim(shape):
    from fused_ssim import fused_ssim
    from sfgs.loss import photometric
    a, b = image_pair(*shape, 5, noise=0.05)
    y = b.to(DEV)
    x0 = a.to(DEV).requires_grad_(True)
    v0 = fused_ssim(x0[None], y[None])
    (1.0 - v0).backward()
    for mask in (None, torch.ones(1, 1, 1, device=DEV), torch.ones(1, *shape[1:], device=DEV)):
        x = a.to(DEV).requires_grad_(True)
        _, v = photometric(x, y, mask)
        assert torch.equal(v, v0.detach())
        (1.0 - v).backward()                                # only the ssim output is differentiated
        assert torch.equal(x.grad, x0.grad)


def test_training_loss_is_bit_reproducible():
    from sfgs.loss import training_loss
    h, w = 270, 480
    a, b = image_pair(3, h, w, 9)
    gt, depth = depth_pair(h, w, 9)
    mask = make_mask("binary", h, w, 9)
    runs = []
    for _ in range(2):
        x, d = a.to(DEV).requires_grad_(True), depth.to(DEV).requires_grad_(True)
        out = training_loss(x, d, b.to(DEV), gt.to(DEV), to_dev(mask), 0.2, 0.5, invalid="drop")
        out[0].backward()
        runs.append([t.detach() for t in out] + [x.grad, d.grad])
    for p, q in zip(*runs):
        assert torch.equal(p, q)


# ---- 5. the whole loss at 1080p: composition, launches, no host synchronisation --------------------------------------------------
def _inputs_1080p():
    h, w = 1080, 1920
    a, b = image_pair(3, h, w, 21, noise=0.05)
    gt, depth = depth_pair(h, w, 21, nan_frac=0.01)
    return a.to(DEV), b.to(DEV), gt.to(DEV), depth.to(DEV), make_mask("binary", h, w, 21).to(DEV)


@pytest.mark.parametrize("invalid", ["zero", "drop"])
def test_training_loss_1080p_equals_its_composition(invalid):
    from sfgs.loss import depth_pearson, photometric, training_loss
    a, b, gt, depth, mask = _inputs_1080p()
    lam, lamd = 0.2, 0.5
    x0, d0 = a.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    Ll1_0, ssim_0 = photometric(x0, b, mask)
    dl_0 = depth_pearson(d0, gt, mask, invalid)
    loss_0 = (1.0 - lam) * Ll1_0 + lam * (1.0 - ssim_0) + lamd * dl_0
    loss_0.backward()
    x, d = a.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    L.profile_enable(True)
    try:
        L.profile_collect()
        loss, Ll1, ssim, dl = training_loss(x, d, b, gt, mask, lam, lamd, invalid=invalid)
        fwd = {k: v[1] for k, v in L.profile_collect().items()}
        loss.backward()
        bwd = {k: v[1] for k, v in L.profile_collect().items()}
    finally:
        L.profile_enable(False)
    assert fwd == {"loss_photo_fwd": 1, "loss_depth_fwd": 1, "loss_final": 1}     # exactly three library launches
    assert bwd == {"loss_photo_bwd": 1, "loss_depth_bwd": 1}                      # exactly two
    for name, got, want in (("loss", loss, loss_0), ("Ll1", Ll1, Ll1_0), ("ssim", ssim, ssim_0), ("depth_loss", dl, dl_0)):
        print(f"{invalid} {name}: rel {abs(float(got) - float(want)) / abs(float(want)):.3e}")
        assert abs(float(got) - float(want)) <= 5e-7 * abs(float(want)), name
    for name, got, want in (("image", x.grad, x0.grad), ("depth", d.grad, d0.grad)):
        err = float((got - want).abs().max() / want.abs().max())
        print(f"{invalid} grad {name}: err / max {err:.3e}")
        assert err <= 1e-6, name


def test_training_loss_does_not_synchronise_the_host():
    from sfgs.loss import training_loss
    a, b, gt, depth, mask = _inputs_1080p()
    one = torch.ones((1, 1, 1), device=DEV)
    big = torch.randn(8192, 8192, device=DEV)
    x, d = a.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    training_loss(x, d, b, gt, mask, 0.2, 0.5)[0].backward()       # warm-up: library load, allocator
    big @ big
    x.grad = d.grad = None
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    honoured = False
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(40):                                           # a long queue in front of the loss
            big @ big
        for m, inv in ((mask, "zero"), (one, "drop")):
            loss = training_loss(x, d, b, gt, m, 0.2, 0.5, invalid=inv)[0]
            loss.backward()
        done.record()
        returned_early = not done.query()       # the calls came back while the queue in front of them was still running
        try:
            loss.item()
        except RuntimeError:
            honoured = True                     # this build raises on a synchronising call: the block above made none
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    print(f"sync debug mode honoured by this torch build: {honoured}; returned before the queue drained: {returned_early}")
    assert returned_early
    assert torch.isfinite(loss) and torch.isfinite(x.grad).all()


# ---- 6. drop-ins and install() -------------------------------------------------------------------------------------------------------
def test_l1_loss_drop_in_against_torch():
    from sfgs.loss import l1_loss
    for shape, seed in (((3, 67, 131), 1), ((1, 1080, 1920), 2), ((7,), 3), ((2, 3, 5, 9), 4)):
        g = torch.Generator().manual_seed(seed)
        a = torch.rand(*shape, generator=g).to(DEV).requires_grad_(True)
        b = torch.rand(*shape, generator=g).to(DEV).requires_grad_(True)
        v = l1_loss(a, b)
        (3.0 * v).backward()
        ref = (a.detach().double() - b.detach().double()).abs().mean()
        assert v.shape == () and abs(v.item() - float(ref)) <= 1e-6 * float(ref)
        gref = 3.0 * torch.sign(a.detach() - b.detach()) / a.numel()
        assert a.grad.shape == a.shape and torch.allclose(a.grad, gref, rtol=1e-6, atol=0)
        assert torch.allclose(b.grad, -gref, rtol=1e-6, atol=0)
    # an unaligned view (storage offset of one float): the scalar route
    base = torch.rand(3 * 50 * 70 + 1, device=DEV)
    a, b = base[1:].view(3, 50, 70), torch.rand(3, 50, 70, device=DEV)
    assert abs(float(l1_loss(a, b)) - float((a.double() - b.double()).abs().mean())) <= 1e-6


def _pearson_torch64(p, t):
    p, t = (v.detach().double().cpu().reshape(-1).requires_grad_(True) for v in (p, t))
    pc, tc = p - p.mean(), t - t.mean()
    r = ((pc * tc).sum() / ((pc * pc).sum() * (tc * tc).sum()).sqrt()).clamp(-1.0, 1.0)
    r.backward()
    return r.item(), p.grad.numpy(), t.grad.numpy()


@pytest.mark.parametrize("shape", [(8710,), (129600, 1), (3,)])
def test_pearson_corrcoef_drop_in_against_torch(shape):
    from sfgs.loss import pearson_corrcoef
    g = torch.Generator().manual_seed(shape[0])
    p = (400.0 + 20.0 * torch.randn(*shape, generator=g))
    t = 0.9 * p + 6.0 * torch.randn(*shape, generator=g) + 7.0
    ref, gp, gt_ = _pearson_torch64(p, t)
    pd, td = p.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    r = pearson_corrcoef(pd, td)
    r.backward()
    assert r.shape == () and abs(r.item() - ref) <= 2.4e-7
    assert pd.grad.shape == pd.shape and td.grad.shape == td.shape
    assert np.abs(pd.grad.cpu().numpy().reshape(-1) - gp).max() <= 1e-5 * np.abs(gp).max()
    assert np.abs(td.grad.cpu().numpy().reshape(-1) - gt_).max() <= 1e-5 * np.abs(gt_).max()
    # no scrub on this path: a NaN in the inputs is a NaN out, as with torchmetrics
    bad = p.clone()
    bad.view(-1)[0] = float("nan")
    assert torch.isnan(pearson_corrcoef(bad.to(DEV), t.to(DEV)))


def test_install_routes_the_training_modules_loss_calls_to_the_hip_kernels():
    from sfgs import loss
    train = types.ModuleType("train")

    def torch_l1(network_output, gt):                       # utils.loss_utils.l1_loss
        return torch.abs(network_output - gt).mean()

    def torch_pearson(preds, target):                       # torchmetrics' formula
        pc, tc = preds - preds.mean(), target - target.mean()
        return ((pc * tc).sum() / ((pc * pc).sum() * (tc * tc).sum()).sqrt()).clamp(-1.0, 1.0)
    train.l1_loss, train.pearson_corrcoef = torch_l1, torch_pearson
    exec("def depth_loss_func(gt_depth, depth):\n    return (1 - pearson_corrcoef(gt_depth, depth)).mean()\n", train.__dict__)   # train.py:970-973

    def step():                                             # train.py:217, 227-232
        a, b = image_pair(3, 67, 130, 4)
        gt, depth = depth_pair(67, 130, 4)
        x, d = a.to(DEV).requires_grad_(True), depth.to(DEV).requires_grad_(True)
        Ll1 = train.l1_loss(x, b.to(DEV))
        gt_depth, dd = gt.to(DEV).reshape(-1, 1), (1.0 * d).reshape(-1, 1)
        nan_inf_mask = torch.isnan(dd) | torch.isinf(dd) | torch.isnan(gt_depth) | torch.isinf(gt_depth)
        dd[nan_inf_mask] = 0.0
        gt_depth[nan_inf_mask] = 0.0
        depth_loss = train.depth_loss_func(gt_depth, dd)
        (0.8 * Ll1 + 0.5 * depth_loss).backward()
        return Ll1.item(), depth_loss.item(), x.grad, d.grad

    def counted(fn):
        L.profile_enable(True)
        try:
            L.profile_collect()
            res = fn()
            return res, {k: v[1] for k, v in L.profile_collect().items()}
        finally:
            L.profile_enable(False)
    ref, launches = counted(step)
    assert not any(k.startswith("loss_") for k in launches)
    loss.install(train)
    try:
        got, launches = counted(step)
    finally:
        loss.uninstall(train)
    # l1_loss: streaming pass + finalisation, one streaming backward; pearson_corrcoef: the same (gradient w.r.t. `target`)
    assert launches == {"loss_depth_fwd": 2, "loss_final": 2, "loss_depth_bwd": 2}
    assert abs(got[0] - ref[0]) <= 1e-6 * ref[0] and abs(got[1] - ref[1]) <= 1e-6
    assert torch.allclose(got[2], ref[2], rtol=1e-5, atol=1e-12)
    assert float((got[3] - ref[3]).abs().max()) <= 1e-5 * float(ref[3].abs().max())
    assert train.l1_loss is torch_l1 and train.pearson_corrcoef is torch_pearson
    _, launches = counted(step)
    assert not any(k.startswith("loss_") for k in launches)
