"""sfgs.metrics on the GPU: the evaluation pass of training_report (clamp, L1, PSNR) and SSIM in two launches per view.

The accuracy bar, in the house form: with e_kernel = |kernel - oracle64| and e_ref = |reference - oracle64| on the same input
(oracle64: tests/metrics_np.py; the reference: the golden value for golden cases, otherwise the reference's spelling run on
the device in the test),
    l1, mse:        e_kernel <= 2 e_ref + 16 * 2^-24 * |value|
    psnr, psnr_c:   e_kernel <= 2 e_ref + (20 / ln 10) * 1/2 * 16 * 2^-24 dB
-- the kernel's float32 chain per tile is one subtraction, one product, three adds per thread and an eight-level tree,
everything after it is float64; 16 roundings bound that chain for non-negative terms, and -10 log10 carries a relative error
e of the mse to (10 / ln 10) e dB. ssim: within 2e-6 of the golden value (what tests/test_gpu_ops.py applies to fused_ssim),
and its float32 rounding is bit-identical to fused_ssim on the clamped pair (same tiles, chains and reduction order).
Every case prints e_kernel, e_ref and the bar.

The kernels have no profiler id (the library's id list is pinned by older tests), so launches are counted with torch.profiler."""
import functools
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import metrics_np as mnp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_metrics.npz")
SLACK_REL = 16 * 2.0 ** -24
SLACK_DB = (20.0 / math.log(10.0)) * 0.5 * SLACK_REL
SSIM_ABS = 2e-6
GOLDEN_CASES = ("clamp", "tile", "gray", "same", "nan", "view0", "view1", "view2")
TILE_SHAPES = [(3, 45, 65), (3, 22, 32), (1, 23, 33), (2, 5, 3), (1, 1, 1), (4, 21, 31), (3, 418, 608)]


# ---- inputs, the reference's spelling on the device, the bar --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair(shape, wide=True):
    """A seeded (image, gt_image) pair on the CPU; wide: values in about [-0.3, 1.3] on both operands (the clamp matters)."""
    g = torch.Generator().manual_seed(1000 * shape[0] + 37 * shape[1] + shape[2])
    gt = torch.rand(*shape, generator=g)
    image = gt + 0.1 * torch.randn(*shape, generator=g)
    return (1.6 * image - 0.3, 1.6 * gt - 0.3) if wide else (image, gt)


@functools.lru_cache(maxsize=None)
def oracle_row(shape, clamp, wide=True):
    a, b = pair(shape, wide)
    return mnp.view_metrics(a.numpy(), b.numpy(), clamp=clamp, ssim=True)


@torch.no_grad()
def reference_spelling(image, gt_image, clamp):
    """train.py:1064,1075,1090-1091 around utils.loss_utils.l1_loss and utils.image_utils.psnr / mse, on the device."""
    if clamp:
        image, gt_image = torch.clamp(image, 0.0, 1.0), torch.clamp(gt_image, 0.0, 1.0)
    l1 = torch.abs((image - gt_image)).mean().mean().double()
    mse_c = (((image - gt_image)) ** 2).view(image.shape[0], -1).mean(1, keepdim=True)
    psnr_c = 20 * torch.log10(1.0 / torch.sqrt(mse_c))
    return {"l1": l1.item(), "psnr": psnr_c.mean().double().item(), "psnr_c": psnr_c.double().cpu().numpy().reshape(-1),
            "mse_c": mse_c.double().cpu().numpy().reshape(-1), "mse": ((image - gt_image) ** 2).mean().double().item()}


def hold(name, field, got, want, ref, slack_rel=None):
    """One figure against the bar (slack_rel None: the dB bar). Non-finite expectations must match exactly."""
    got, want, ref = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (got, want, ref))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (name, field, got, want)
    if not fin.any():
        print(f"{name} {field}: {got} as expected")
        return
    e_kernel, e_ref = np.abs(got[fin] - want[fin]), np.abs(ref[fin] - want[fin])
    bar = 2 * e_ref + (SLACK_DB if slack_rel is None else slack_rel * np.abs(want[fin]))
    print(f"{name} {field}: e_kernel {e_kernel.max():.3e}  e_ref {e_ref.max():.3e}  bar {bar.min():.3e}")
    assert np.isfinite(got[fin]).all() and (e_kernel <= bar).all(), (name, field, got, want, ref)


def hold_row(name, row, want, ref, P, ssim):
    """A kernel row [8] against oracle64's row `want` and the reference's figures `ref`."""
    hold(name, "l1", row[0], want[0], ref["l1"], SLACK_REL)
    hold(name, "mse", row[3], want[3], ref["mse"], SLACK_REL)
    hold(name, "psnr", row[1], want[1], ref["psnr"])
    hold(name, "psnr_c", row[4:4 + P], want[4:4 + P], ref["psnr_c"])
    assert np.isnan(row[4 + P:]).all(), (name, row)                     # channels that do not exist
    if not ssim:
        assert np.isnan(row[2]), (name, row)


def fused_ssim_value(x, y, clamp):
    from fused_ssim import fused_ssim
    if clamp:
        x, y = torch.clamp(x, 0.0, 1.0), torch.clamp(y, 0.0, 1.0)
    return fused_ssim(x[None], y[None], train=False)


def same_f32_bits(ssim64, f32_tensor):
    a = np.float32(ssim64)
    b = f32_tensor.cpu().numpy().astype(np.float32).reshape(())
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def device_activities(fn):
    """fn() under torch.profiler: {name: count} of everything with device time (kernels, copies, memsets), and fn's result."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    return {e.key: e.count for e in prof.key_averages() if e.device_time_total > 0}, res


def stream_vector_width(acts):
    """The V of the one metrics_stream_kernel<V, CLAMP> launch among the activities (demangled or mangled name)."""
    keys = [k for k in acts if "metrics_stream_kernel" in k]
    assert len(keys) == 1 and acts[keys[0]] == 1, acts
    m = re.search(r"metrics_stream_kernel(?:<\s*(?:\(int\)\s*)?(\d)|ILi(\d))", keys[0])
    assert m, keys[0]
    return int(m.group(1) or m.group(2))


# ---- 1. the reference's own output (golden) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", GOLDEN_CASES)
def test_metrics_match_reference_golden(tag):
    from sfgs.metrics import view_metrics
    G = np.load(GOLDEN)
    a, b = G[f"{tag}_image"], G[f"{tag}_gt_image"]
    P = a.shape[0]
    x, y = torch.tensor(a, device=DEV), torch.tensor(b, device=DEV)
    want = mnp.view_metrics(a, b)
    ref = {"l1": G[f"{tag}_l1"], "psnr": G[f"{tag}_psnr"], "psnr_c": G[f"{tag}_psnr_c"],
           "mse": np.mean(G[f"{tag}_mse_c"].astype(np.float64))}
    out = view_metrics(x, y)
    assert out.shape == (8,) and out.dtype == torch.float64 and out.device == x.device
    row = out.cpu().numpy()
    print(tag, dict(zip(mnp.ROW, row)))
    for k, name in ((0, "l1"), (1, "psnr")):                            # +inf and NaN: the golden entries, exactly
        if not np.isfinite(ref[name]):
            assert np.array_equal(row[k], ref[name], equal_nan=True), (name, row)
    bad = ~np.isfinite(G[f"{tag}_psnr_c"])
    assert np.array_equal(row[4:4 + P][bad], G[f"{tag}_psnr_c"][bad].astype(np.float64), equal_nan=True)
    hold_row(f"golden {tag}", row, want, ref, P, ssim=True)
    gs = float(G[f"{tag}_ssim"])
    if np.isfinite(gs):
        print(f"golden {tag} ssim: |kernel - golden| {abs(row[2] - gs):.3e}  |kernel - oracle64| {abs(row[2] - want[2]):.3e}")
        assert abs(row[2] - gs) <= SSIM_ABS
    else:
        assert np.isnan(row[2])
    assert same_f32_bits(row[2], fused_ssim_value(x, y, True))
    # the stream route on the same input: the same figures, no SSIM
    hold_row(f"golden {tag} stream", view_metrics(x, y, ssim=False).cpu().numpy(), want, ref, P, ssim=False)


def test_golden_three_view_set_gives_the_two_printed_means():
    from sfgs.metrics import Evaluator
    G = np.load(GOLDEN)
    ev = Evaluator(3)
    for v in ("view0", "view1", "view2"):
        ev.add(torch.tensor(G[f"{v}_image"], device=DEV), torch.tensor(G[f"{v}_gt_image"], device=DEV))
    r = ev.result()
    want = mnp.summarise(np.stack([mnp.view_metrics(G[f"{v}_image"], G[f"{v}_gt_image"]) for v in ("view0", "view1", "view2")]))
    hold("views", "l1_test", r["l1"], want["l1"], G["views_l1_test"], SLACK_REL)
    hold("views", "psnr_test", r["psnr"], want["psnr"], G["views_psnr_test"])


# ---- 2. the tile route against the reference's spelling on the device --------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("shape", TILE_SHAPES)
def test_tile_route(shape, clamp):
    from sfgs.metrics import view_metrics
    a, b = pair(shape)
    x, y = a.to(DEV), b.to(DEV)
    want = oracle_row(shape, clamp)
    ref = reference_spelling(x, y, clamp)
    row = view_metrics(x, y, clamp=clamp).cpu().numpy()
    name = f"tile {shape} clamp={clamp}"
    hold_row(name, row, want, ref, shape[0], ssim=True)
    print(f"{name} ssim: {row[2]:.9f}  |kernel - oracle64| {abs(row[2] - want[2]):.3e}")
    assert same_f32_bits(row[2], fused_ssim_value(x, y, clamp))
    if clamp:                                   # operands in [0, 1]: the range fused_ssim's 2e-6 was established on
        assert abs(row[2] - want[2]) <= SSIM_ABS
    # both routes give the same l1, mse and psnr_c on the same input, within the bar
    srow = view_metrics(x, y, clamp=clamp, ssim=False).cpu().numpy()
    hold_row(name + " stream", srow, want, ref, shape[0], ssim=False)
    P = shape[0]
    assert abs(srow[0] - row[0]) <= 2 * SLACK_REL * abs(want[0]) and abs(srow[3] - row[3]) <= 2 * SLACK_REL * abs(want[3])
    fin = np.isfinite(want[4:4 + P])            # (1,1,1) clamps both pixels to the same value: +inf on both routes
    assert np.array_equal(srow[4:4 + P][~fin], row[4:4 + P][~fin], equal_nan=True)
    assert np.abs(srow[4:4 + P][fin] - row[4:4 + P][fin]).max(initial=0.0) <= 2 * SLACK_DB


def test_out_row_is_written_in_place_and_runs_are_bit_identical():
    from sfgs.metrics import view_metrics
    a, b = pair((3, 45, 65))
    x, y = a.to(DEV), b.to(DEV)
    table = torch.zeros(3, 8, dtype=torch.float64, device=DEV)
    got = view_metrics(x, y, out=table[1])
    assert got.data_ptr() == table[1].data_ptr()
    again = view_metrics(x, y)
    t = table.cpu().numpy()
    assert np.array_equal(t[1].view(np.uint64), again.cpu().numpy().view(np.uint64))
    assert (t[0] == 0).all() and (t[2] == 0).all()                      # nothing next to the row is touched


# ---- 3. the stream route ---------------------------------------------------------------------------------------------------------------
def stream_inputs(kind):
    """-> (x, y) on the device, the contiguous CPU pair they equal, the vector width the route must take (None: not checked)."""
    if kind == "aligned":
        a, b = pair((3, 64, 64))
        return a.to(DEV), b.to(DEV), a, b, 4
    if kind == "odd":                            # H * W is not a multiple of 4
        a, b = pair((3, 7, 5))
        return a.to(DEV), b.to(DEV), a, b, 1
    if kind == "offset":                         # storage starts one float past a 16-byte boundary
        a, b = pair((3, 64, 64))
        bx, by = torch.zeros(a.numel() + 1, device=DEV), torch.zeros(a.numel() + 1, device=DEV)
        x, y = bx[1:].view(3, 64, 64), by[1:].view(3, 64, 64)
        x.copy_(a)
        y.copy_(b)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        return x, y, a, b, 1
    if kind == "pixels":
        a, b = pair((4, 1, 1))
        return a.to(DEV), b.to(DEV), a, b, 1
    if kind == "ragged":                         # several blocks per plane, a ragged last block
        a, b = pair((1, 300, 301))
        return a.to(DEV), b.to(DEV), a, b, 4
    assert kind == "permuted"                    # [H,W,C] storage seen as [C,H,W]
    a, b = pair((3, 33, 47))
    x, y = a.permute(1, 2, 0).contiguous().to(DEV).permute(2, 0, 1), b.permute(1, 2, 0).contiguous().to(DEV).permute(2, 0, 1)
    assert not x.is_contiguous()
    return x, y, a, b, None


@pytest.mark.parametrize("kind", ["aligned", "odd", "offset", "pixels", "ragged", "permuted"])
def test_stream_route(kind):
    from sfgs import metrics
    x, y, a, b, vec = stream_inputs(kind)
    P = a.shape[0]
    for clamp in (True, False):
        want = mnp.view_metrics(a.numpy(), b.numpy(), clamp=clamp, ssim=False)
        ref = reference_spelling(x, y, clamp)
        acts, out = device_activities(lambda: metrics.view_metrics(x, y, clamp=clamp, ssim=False))
        if vec is not None:
            assert stream_vector_width(acts) == vec, acts
        hold_row(f"stream {kind} clamp={clamp}", out.cpu().numpy(), want, ref, P, ssim=False)
    # the drop-ins: no clamp, float32 [P,1]
    want = mnp.view_metrics(a.numpy(), b.numpy(), clamp=False, ssim=False)
    ref = reference_spelling(x, y, False)
    p, m = metrics.psnr(x, y), metrics.mse(x, y)
    assert p.shape == m.shape == (P, 1) and p.dtype == m.dtype == torch.float32 and p.device == x.device
    hold(f"psnr() {kind}", "psnr_c", p.cpu().numpy().reshape(-1), want[4:4 + P], ref["psnr_c"])
    hold(f"mse() {kind}", "mse_c", m.cpu().numpy().reshape(-1), mnp.plane_mse(a.numpy(), b.numpy()), ref["mse_c"], SLACK_REL)


def test_dropins_take_the_batched_form_and_special_values():
    from sfgs import metrics
    a, b = pair((3, 64, 64), wide=False)
    x, y = a.to(DEV), b.to(DEV)
    p = metrics.psnr(x[None], y[None])                                   # planes = shape[0] = 1, as the reference views it
    assert p.shape == (1, 1)
    hold("psnr() batched", "psnr", p.item(), mnp.psnr_of_mse(mnp.plane_mse(a.numpy()[None], b.numpy()[None]))[0],
         reference_spelling(x[None], y[None], False)["psnr_c"][0])
    assert torch.isposinf(metrics.psnr(x, x)).all() and (metrics.mse(x, x) == 0).all()
    z = x.clone()
    z[1, 5, 7] = float("nan")
    p, m = metrics.psnr(z, y), metrics.mse(z, y)
    assert torch.isnan(p[1]) and torch.isnan(m[1]) and torch.isfinite(p[[0, 2]]).all() and torch.isfinite(m[[0, 2]]).all()
    row = metrics.view_metrics(z, y, ssim=False).cpu().numpy()
    assert np.isnan(row[[0, 1, 2, 3, 5, 7]]).all() and np.isfinite(row[[4, 6]]).all()
    # the clamp keeps NaN, as torch.clamp does (fminf / fmaxf would turn it into 0 or 1)
    for ssim in (True, False):
        row = metrics.view_metrics(z, y, clamp=True, ssim=ssim).cpu().numpy()
        assert np.isnan(row[[0, 1, 3, 5]]).all() and np.isfinite(row[[4, 6]]).all(), row


# ---- 4. the Evaluator --------------------------------------------------------------------------------------------------------------------
VIEW_SHAPES = ((3, 45, 65), (3, 33, 70), (1, 58, 36))


def run_evaluator():
    from sfgs.metrics import Evaluator
    ev = Evaluator(3, device=DEV)
    for s in VIEW_SHAPES:
        a, b = pair(s)
        ev.add(a.to(DEV), b.to(DEV))
    return ev


def test_evaluator_accumulates_views_of_different_sizes():
    ev = run_evaluator()
    r = ev.result()
    assert r["n"] == 3 and r["per_view"].shape == (3, 8) and r["per_view"].dtype == np.float64
    for i, s in enumerate(VIEW_SHAPES):
        a, b = pair(s)
        hold_row(f"evaluator view {i}", r["per_view"][i], oracle_row(s, True), reference_spelling(a.to(DEV), b.to(DEV), True),
                 s[0], ssim=True)
        assert abs(r["per_view"][i, 2] - oracle_row(s, True)[2]) <= SSIM_ABS
    want = mnp.summarise(r["per_view"])                                  # means and POPULATION stds of the rows
    for k in ("l1", "psnr", "ssim", "l1_std", "psnr_std", "ssim_std"):
        assert r[k] == pytest.approx(want[k], rel=1e-14, abs=0), k
    assert r["psnr_std"] == pytest.approx(np.std(r["per_view"][:, 1]), rel=1e-14) and r["psnr_std"] > 0
    a, b = pair(VIEW_SHAPES[0])
    with pytest.raises(ValueError, match="full"):                        # a fourth add on capacity 3
        ev.add(a.to(DEV), b.to(DEV))
    assert ev.n == 3
    again = run_evaluator().result()                                     # two runs are bit-identical
    assert np.array_equal(again["per_view"].view(np.uint64), r["per_view"].view(np.uint64))
    ev.reset()
    assert ev.n == 0 and ev.result()["n"] == 0 and ev.result()["per_view"].shape == (0, 8)
    ev.add(a.to(DEV), b.to(DEV), ssim=False)                             # ... and the table is usable again
    r1 = ev.result()
    assert r1["n"] == 1 and np.isnan(r1["ssim"]) and r1["l1"] == pytest.approx(r["per_view"][0, 0], rel=2 * SLACK_REL)


def test_add_is_two_launches_without_host_synchronisation_and_result_is_one_copy():
    from sfgs.metrics import Evaluator
    a, b = pair((3, 270, 480))
    x, y = a.to(DEV), b.to(DEV)
    ev = Evaluator(8)
    ev.add(x, y)                                                         # warm-up: library load, allocator, the table
    ev.add(x, y, ssim=False)
    acts, _ = device_activities(lambda: ev.add(x, y))
    print("device activities of one add:", acts)
    assert sum(acts.values()) == 2 and len(acts) == 2
    assert any("metrics_tile_kernel" in k for k in acts) and any("metrics_final_kernel" in k for k in acts)
    acts, _ = device_activities(lambda: ev.add(x, y, ssim=False))
    print("device activities of one add without SSIM:", acts)
    assert sum(acts.values()) == 2 and len(acts) == 2
    assert any("metrics_stream_kernel" in k for k in acts) and any("metrics_final_kernel" in k for k in acts)
    acts, r = device_activities(ev.result)
    print("device activities of result():", acts)
    assert sum(acts.values()) == 1 and ("memcpy" in next(iter(acts)).lower() or "copy" in next(iter(acts)).lower())
    assert r["n"] == 4 and np.array_equal(r["per_view"][0].view(np.uint64), r["per_view"][2].view(np.uint64))
    # no host synchronisation: the calls return while a long queue in front of them is still running
    big = torch.randn(4096, 4096, device=DEV)
    big @ big
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    honoured = False
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(60):
            big @ big
        ev.add(x, y)
        ev.add(x, y, ssim=False)
        done.record()
        returned_early = not done.query()
        try:
            ev._table[0, 0].item()
        except RuntimeError:
            honoured = True                     # this build raises on a synchronising call: the block above made none
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    print(f"sync debug mode honoured by this torch build: {honoured}; returned before the queue drained: {returned_early}")
    assert returned_early


# ---- 5. the hook ---------------------------------------------------------------------------------------------------------------------------
def test_install_routes_psnr_to_the_kernel():
    from sfgs import metrics

    def psnr(img1, img2):                                                # utils/image_utils.py:17-19
        mse = (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
        return 20 * torch.log10(1.0 / torch.sqrt(mse))
    train = types.ModuleType("train")
    train.psnr = psnr
    a, b = pair((3, 45, 65), wide=False)
    x, y = torch.clamp(a.to(DEV), 0.0, 1.0), torch.clamp(b.to(DEV), 0.0, 1.0)
    ref = train.psnr(x, y)
    metrics.install(train)
    try:
        assert train.psnr is metrics.psnr
        acts, got = device_activities(lambda: train.psnr(x, y))
        assert any("metrics_stream_kernel" in k for k in acts), acts
    finally:
        metrics.uninstall(train)
    assert train.psnr is psnr
    assert got.shape == (3, 1) and got.dtype == torch.float32
    want = mnp.psnr_of_mse(mnp.plane_mse(a.numpy(), b.numpy(), clamp=True))
    hold("installed psnr", "psnr_c", got.cpu().numpy().reshape(-1), want, ref.double().cpu().numpy().reshape(-1))
    # what training_report does with it (train.py:1091)
    hold("installed psnr", ".mean().double()", got.mean().double().item(), want.mean(), ref.mean().double().item())
