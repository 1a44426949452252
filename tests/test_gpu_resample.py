"""GPU tests of sfgs.resample (csrc/resample.hip) and of the loss's subpixel_offset keyword.

The accuracy bar, everywhere:   e_kernel = max |kernel - oracle64|  <=  2 * e_ref + 8 * 2^-24,   e_ref = max |reference - oracle64|
on the same input, oracle64 = tests/resample_np.py. The reference is the golden output (tests/golden/make_golden_resample.py:
the reference's statements around torch's CPU grid_sample) for the golden cases and the reference's spelling (train.py:64-77)
run on the device inside the test otherwise. At float32 the error is the rounding of x + ox at magnitude W; the reference
(normalise, un-normalise) and the kernel (x + ox directly) round at different points, so neither is "the" answer -- the bar
allows the kernel twice the reference's own error plus the rounding of four products and their sum for values in [0, 1].
Every case prints e_kernel, e_ref and the largest difference to torch's device result.

The kernel has no profiler id (the library's id list is pinned by older tests), so launches are counted with
torch.profiler -- every device activity of the call -- next to the library's own counters for the loss kernels."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from resample_np import resample64
from sfgs import _lib as L
from test_gpu_loss import depth_pair, image_pair, pearson64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_resample.npz")
SLACK = 8 * 2.0 ** -24


# ---- the reference's spelling, on the device --------------------------------------------------------------------------------------
@torch.no_grad()
def reference_spelling(image, offset):
    """train.py:64-77 (`.cuda()` -> the test's device); image is the already masked ground truth (train.py:207)."""
    height, width = image.shape[1:]
    meshgrid = np.meshgrid(range(width), range(height), indexing='xy')
    id_coords = np.stack(meshgrid, axis=0).astype(np.float32)
    id_coords = torch.from_numpy(id_coords).to(image.device)
    id_coords = id_coords.permute(1, 2, 0) + offset
    id_coords[..., 0] /= (width - 1)
    id_coords[..., 1] /= (height - 1)
    id_coords = id_coords * 2 - 1
    return torch.nn.functional.grid_sample(image[None], id_coords[None], align_corners=True, padding_mode="border")[0]


def inputs(c, h, w, seed, half=0.5, mask_kind=None):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(c, h, w, generator=g)
    offset = (torch.rand(h, w, 2, generator=g) - 0.5) * (2.0 * half)
    mask = {None: None, "ones1": torch.ones(1, 1, 1), "scalar": torch.full((1, 1, 1), 0.75),
            "fractional": torch.rand(1, h, w, generator=g), "binary": (torch.rand(1, h, w, generator=g) < 0.7).float()}[mask_kind]
    return image, offset, mask


def to_dev(t):
    return None if t is None else t.to(DEV)


def check(name, image, offset, mask, golden_out=None):
    """Run the kernel and the device reference on (image, offset, mask) (CPU tensors), print the three figures, assert the
    bar on every pixel. -> (kernel result, torch's device result), numpy."""
    from sfgs.resample import resample_gt
    x, o, m = to_dev(image), to_dev(offset), to_dev(mask)
    got_t = resample_gt(x, o, m)
    assert got_t.shape == image.shape and got_t.dtype == torch.float32 and not got_t.requires_grad
    got = got_t.cpu().numpy()
    dev_ref = reference_spelling(x if m is None else m * x, o).cpu().numpy()
    want = resample64(image.numpy(), offset.numpy(), None if mask is None else mask.numpy())
    ref = dev_ref if golden_out is None else golden_out
    e_kernel = np.abs(got - want).max()
    e_ref = np.abs(ref - want).max()
    d_torch = np.abs(got - dev_ref).max()
    print(f"{name} {tuple(image.shape)}: e_kernel {e_kernel:.3e}  e_ref {e_ref:.3e}  bar {2 * e_ref + SLACK:.3e}  "
          f"max |kernel - torch device| {d_torch:.3e}")
    assert np.isfinite(got).all()
    assert e_kernel <= 2 * e_ref + SLACK
    return got, dev_ref


# ---- 1. the reference's own output (golden) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_resample_matches_reference_golden(tag):
    G = np.load(GOLDEN)
    mask = torch.tensor(G[f"{tag}_mask"]) if f"{tag}_mask" in G.files else None
    check(f"golden {tag}", torch.tensor(G[f"{tag}_image"]), torch.tensor(G[f"{tag}_offset"]), mask, golden_out=G[f"{tag}_out"])


# ---- 2. against the reference's spelling on the device --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(45, 65), (64, 64)])
@pytest.mark.parametrize("mask_kind", [None, "scalar", "fractional"])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_resample_channels_and_mask_forms(c, mask_kind, shape):
    h, w = shape
    image, offset, mask = inputs(c, h, w, 100 * c + h, mask_kind=mask_kind)
    check(f"C {c} mask {mask_kind}", image, offset, mask)


def test_resample_width_that_is_no_multiple_of_the_wave():
    image, offset, mask = inputs(3, 33, 130, 7, half=3.0, mask_kind="binary")     # every border clamps, too
    check("W 130", image, offset, mask)
    image, offset, mask = inputs(2, 3, 257, 8, mask_kind="ones1")                  # one pixel past a workgroup, C = 2
    check("W 257", image, offset, mask)


@pytest.mark.parametrize("shift", [(0, 0), (1, 1), (-2, -2), (1, -2)])
def test_resample_integer_offsets_shift_exactly(shift):
    c, h, w = 3, 45, 65
    image, offset, mask = inputs(c, h, w, 9, mask_kind="fractional")
    offset[..., 0], offset[..., 1] = float(shift[0]), float(shift[1])
    got, _ = check(f"integer {shift}", image, offset, mask)
    s = (mask * image).numpy()
    xs = np.clip(np.arange(w) + shift[0], 0, w - 1)
    ys = np.clip(np.arange(h) + shift[1], 0, h - 1)
    np.testing.assert_array_equal(got, s[:, ys][:, :, xs])             # weights 1, 0, 0, 0: the tap itself


def test_resample_offsets_that_land_exactly_on_the_last_column_and_row():
    c, h, w = 3, 45, 65
    image, offset, mask = inputs(c, h, w, 10)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    offset[..., 0] = torch.where(xx % 2 == 0, (w - 1) - xx, offset[..., 0])     # u = W - 1 exactly on every other column
    offset[..., 1] = torch.where(yy % 3 == 0, (h - 1) - yy, offset[..., 1])     # v = H - 1 exactly on every third row
    got, _ = check("on W-1 / H-1", image, offset, mask)
    both = ((xx % 2 == 0) & (yy % 3 == 0)).numpy()
    np.testing.assert_array_equal(got[:, both], np.broadcast_to(image.numpy()[:, -1, -1][:, None], (c, int(both.sum()))))


def test_resample_offsets_far_outside_the_frame():
    c, h, w = 3, 45, 65
    image, offset, mask = inputs(c, h, w, 11, mask_kind="binary")
    g = torch.Generator().manual_seed(12)
    far = torch.where(torch.rand(h, w, 2, generator=g) < 0.5, -1.0e4, 1.0e4)
    pick = torch.rand(h, w, 2, generator=g) < 0.5
    offset = torch.where(pick, far, offset)
    got, _ = check("+-1e4", image, offset, mask)
    corner = (pick[..., 0] & pick[..., 1]).numpy()                                  # both coordinates pushed out: a frame corner
    s = (mask * image).numpy()
    xi = np.where(far[..., 0].numpy() > 0, w - 1, 0)
    yi = np.where(far[..., 1].numpy() > 0, h - 1, 0)
    np.testing.assert_array_equal(got[:, corner], s[:, yi[corner], xi[corner]])


def test_resample_full_size_frame():
    """1080 x 1920: the only size at which the coordinate's rounding reaches 1e-4. A single run."""
    image, offset, mask = inputs(3, 1080, 1920, 13, mask_kind="binary")
    check("1080p", image, offset, mask)


def test_resample_non_finite_offsets_follow_torch():
    """NaN / +-inf offsets. Where BOTH coordinates are decided by the clip alone -- non-finite, or +-1e4 -- the sample is a
    frame corner with weights 1, 0, 0, 0 and the result must equal torch's device result exactly (expected: NaN and -inf -> 0,
    +inf -> W - 1 / H - 1). Where the other coordinate is an ordinary offset its float32 rounding differs between the
    reference's sequence and x + ox, so those pixels meet the bar like every other pixel (the oracle clips as above)."""
    c, h, w = 3, 45, 65
    image, offset, mask = inputs(c, h, w, 14, mask_kind="fractional")
    nan, inf = float("nan"), float("inf")
    specials = [nan, inf, -inf]
    exact = [(a, b) for a in specials for b in specials]
    exact += [(nan, 1.0e4), (-1.0e4, inf), (inf, -1.0e4), (1.0e4, -inf), (-inf, 1.0e4), (-1.0e4, nan)]
    mixed = [(nan, 0.3), (0.2, inf), (-inf, -0.4), (0.45, nan), (inf, 0.0), (-0.25, -inf)]
    where = {}
    for k, (ox, oy) in enumerate(exact + mixed):
        y, x = 2 + (5 * k) % (h - 4), 3 + (11 * k) % (w - 6)
        assert (y, x) not in where
        where[(y, x)] = (ox, oy)
        offset[y, x, 0], offset[y, x, 1] = ox, oy
    got, dev_ref = check("non-finite", image, offset, mask)
    s = (mask * image).numpy()
    pos = lambda t, last: last if t > 0 else 0              # NaN > 0 is False
    for (y, x), (ox, oy) in list(where.items())[:len(exact)]:
        np.testing.assert_array_equal(got[:, y, x], dev_ref[:, y, x], err_msg=f"offset ({ox}, {oy}) at ({y}, {x})")
        np.testing.assert_array_equal(got[:, y, x], s[:, pos(oy, h - 1), pos(ox, w - 1)], err_msg=f"offset ({ox}, {oy})")


def test_resample_never_reads_past_the_planes():
    """The input sits at the end of an allocation whose tail (2 W floats: longer than a row) the test fills with 1e30 (and, in
    a second pass, +inf, which a weight of 0 would turn into NaN); the mask plane likewise. All offsets push to the bottom-right corner: the right and
    bottom neighbours of that tap have index W / H. The output must equal the corner values. Values only."""
    from sfgs.resample import resample_gt
    c, h, w = 3, 45, 65
    tail = 2 * w            # the right neighbour would be index P, the bottom ones P + W - 1 and P + W: all inside the tail
    image, _, mask = inputs(c, h, w, 15, mask_kind="fractional")
    for fill in (1.0e30, float("inf")):
        buf = torch.full((c * h * w + tail,), fill, device=DEV)
        mbuf = torch.full((h * w + tail,), fill, device=DEV)
        buf[:c * h * w] = image.reshape(-1).to(DEV)
        mbuf[:h * w] = mask.reshape(-1).to(DEV)
        x, m = buf[:c * h * w].view(c, h, w), mbuf[:h * w].view(1, h, w)
        assert x.is_contiguous() and x.data_ptr() == buf.data_ptr() and m.data_ptr() == mbuf.data_ptr()
        corner = (m[:, -1, -1] * x[:, -1, -1]).cpu()
        for ox, oy in ((float(w), float(h)), (float(w - 1), float(h - 1)), (0.5 + w, 0.25 + h), (float("inf"), float("inf"))):
            offset = torch.empty(h, w, 2, device=DEV)
            offset[..., 0], offset[..., 1] = ox, oy
            offset[0, 0, 0], offset[0, 0, 1] = float(w - 1), float(h - 1)            # lands on the corner exactly
            out = resample_gt(x, offset, m).cpu()
            assert torch.equal(out, corner[:, None, None].expand(c, h, w)), (fill, ox, oy)


# ---- 3. determinism, streams, views, launches -------------------------------------------------------------------------------------------
def test_resample_is_deterministic_and_runs_on_any_stream_and_view():
    from sfgs.resample import resample_gt
    c, h, w = 3, 45, 65
    image, offset, mask = inputs(c, h, w, 16, mask_kind="fractional")
    x, o, m = to_dev(image), to_dev(offset), to_dev(mask)
    first = resample_gt(x, o, m)
    assert torch.equal(first, resample_gt(x, o, m))                                   # two runs: identical bytes
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = resample_gt(x, o, m)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(first, on_side)
    # non-contiguous views of all three give the contiguous result
    xv = torch.empty(c, h, 2 * w, device=DEV)[:, :, ::2]
    xv.copy_(x)
    ov = torch.empty(2, h, w, device=DEV).permute(1, 2, 0)
    ov.copy_(o)
    mv = torch.empty(1, w, h, device=DEV).transpose(1, 2)
    mv.copy_(m)
    assert not (xv.is_contiguous() or ov.is_contiguous() or mv.is_contiguous())
    assert torch.equal(first, resample_gt(xv, ov, mv))
    # an offset tensor that starts at an odd float (4-byte aligned only)
    base = torch.empty(h * w * 2 + 1, device=DEV)
    o_odd = base[1:].view(h, w, 2)
    o_odd.copy_(o)
    assert o_odd.data_ptr() % 8 == 4 and torch.equal(first, resample_gt(x, o_odd, m))
    # never requires grad, whatever the inputs do
    assert not resample_gt(x.clone().requires_grad_(True), o, m).requires_grad


def device_activities(fn):
    """fn() under torch.profiler: {name: count} of everything with device time (kernels, copies, memsets), and fn's result."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    return {e.key: e.count for e in prof.key_averages() if e.device_time_total > 0}, res


def ours(acts):
    return {k: n for k, n in acts.items() if "resample_gt_kernel" in k or "loss_" in k}


def test_resample_is_one_launch_without_host_synchronisation():
    from sfgs.resample import resample_gt
    image, offset, mask = inputs(3, 270, 480, 17, mask_kind="binary")
    x, o, m = to_dev(image), to_dev(offset), to_dev(mask)
    want = resample_gt(x, o, m)                                                       # warm-up: library load, allocator
    acts, got = device_activities(lambda: resample_gt(x, o, m))
    print("device activities of one resample_gt call:", acts)
    assert len(acts) == 1 and sum(acts.values()) == 1 and "resample_gt_kernel" in next(iter(acts))
    assert torch.equal(got, want)
    # no host synchronisation: the call returns while a long queue in front of it is still running
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
        out = resample_gt(x, o, m)
        out = resample_gt(x, o, None)
        done.record()
        returned_early = not done.query()
        try:
            out[0, 0, 0].item()
        except RuntimeError:
            honoured = True                     # this build raises on a synchronising call: the block above made none
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    print(f"sync debug mode honoured by this torch build: {honoured}; returned before the queue drained: {returned_early}")
    assert returned_early


def test_install_routes_create_offset_gt_to_the_kernel():
    from sfgs import resample
    train = types.ModuleType("train")
    train.create_offset_gt = reference_spelling
    exec("def step(mask, original_image, subpixel_offset):\n"
         "    gt_image = mask * original_image\n"                                    # train.py:207
         "    return create_offset_gt(gt_image, subpixel_offset)\n", train.__dict__)     # train.py:215
    image, offset, mask = inputs(3, 45, 65, 18, mask_kind="binary")
    x, o, m = to_dev(image), to_dev(offset), to_dev(mask)
    before = train.step(m, x, o)
    resample.install(train)
    try:
        hooked = train.step(m, x, o)
    finally:
        resample.uninstall(train)
    assert train.create_offset_gt is reference_spelling
    assert torch.equal(hooked, resample.resample_gt(m * x, o))                        # the direct call, bit for bit
    assert torch.equal(hooked, resample.resample_gt(x, o, m))                         # ... and the mask folded into the taps
    assert not torch.equal(hooked, before) and float((hooked - before).abs().max()) < 1e-5


# ---- 4. the loss with subpixel_offset --------------------------------------------------------------------------------------------------
def test_loss_without_mask_equals_the_loss_of_the_resampled_target_bit_for_bit():
    from sfgs.loss import photometric, training_loss
    from sfgs.resample import resample_gt
    a, b = image_pair(3, 45, 65, 19)
    _, offset, _ = inputs(3, 45, 65, 19)
    o, y = to_dev(offset), to_dev(b)
    x0 = a.to(DEV).requires_grad_(True)
    out0 = training_loss(x0, None, resample_gt(y, o), None, None, 0.2, 0)
    out0[0].backward()
    x1 = a.to(DEV).requires_grad_(True)
    out1 = training_loss(x1, None, y, None, None, 0.2, 0, subpixel_offset=o)
    out1[0].backward()
    for p, q in zip(out0, out1):
        assert torch.equal(p, q)
    assert torch.equal(x0.grad, x1.grad)
    Ll1, ssim = photometric(x1.detach(), y, None, o)
    assert torch.equal(Ll1, out1[1]) and torch.equal(ssim, out1[2])
    assert not torch.equal(out1[1], training_loss(x1.detach(), None, y, None, None, 0.2, 0)[1])   # the offset did something


@pytest.mark.parametrize("shape", [(3, 45, 65), (3, 22, 32)])
def test_loss_with_mask_uses_the_resampled_target_as_given(shape):
    """mask * image against resample_gt(gt_image, offset, mask), which is NOT masked a second time: Ll1 = mean |m x - y|, the
    SSIM oracle on (m x, y), autograd for the L1 gradient, y = the device's resample_gt output. Tolerances: the ones
    tests/test_gpu_loss.py applies to these quantities against the same oracle (ssim 2e-6, Ll1 1e-6 relative, ssim gradient
    5e-5 of its maximum + 1e-9, L1 gradient 1e-6 of its maximum, loss 2e-6); the gradient of the loss is their combination."""
    from sfgs.loss import training_loss
    from sfgs.resample import resample_gt
    c, h, w = shape
    lam = 0.2
    a, b = image_pair(c, h, w, 20 + h)
    _, offset, mask = inputs(c, h, w, 21 + h, mask_kind="binary")
    o, m = to_dev(offset), to_dev(mask)
    y = resample_gt(b.to(DEV), o, m).cpu().numpy()
    mn = mask.numpy()
    assert (np.abs(y)[:, mn[0] == 0] > 0).any()            # masked-out pixels next to kept ones are not zero in the target
    xm = (mn * a.numpy()).astype(np.float32)
    val, _, g_ssim = orc.ssim(xm[None], y[None], want_grad=True)
    g_ssim = mn * g_ssim[0]
    x64 = a.double().requires_grad_(True)
    l1_64 = (mask.double() * x64 - torch.from_numpy(y).double()).abs().mean()
    l1_64.backward()
    l1, g_l1 = float(l1_64), x64.grad.numpy()
    loss_ref = (1.0 - lam) * l1 + lam * (1.0 - val)
    x = a.to(DEV).requires_grad_(True)
    loss, Ll1, ssim, depth_loss = training_loss(x, None, b.to(DEV), None, m, lam, 0, subpixel_offset=o)
    print(f"{shape}: ssim {ssim.item() - val:+.3e}  Ll1 rel {Ll1.item() / l1 - 1:+.3e}  loss {loss.item() - loss_ref:+.3e}")
    assert abs(ssim.item() - val) < 2e-6
    assert abs(Ll1.item() - l1) <= 1e-6 * l1
    assert abs(loss.item() - loss_ref) <= 2e-6 and depth_loss.item() == 0.0
    ssim.backward(retain_graph=True)
    assert np.abs(x.grad.cpu().numpy() - g_ssim).max() <= 5e-5 * np.abs(g_ssim).max() + 1e-9
    x.grad = None
    Ll1.backward(retain_graph=True)
    assert np.abs(x.grad.cpu().numpy() - g_l1).max() <= 1e-6 * np.abs(g_l1).max()
    x.grad = None
    loss.backward()
    g_loss = (1.0 - lam) * g_l1 - lam * g_ssim
    bar = (1.0 - lam) * 1e-6 * np.abs(g_l1).max() + lam * (5e-5 * np.abs(g_ssim).max() + 1e-9)
    got = x.grad.cpu().numpy()
    print(f"{shape}: loss grad err {np.abs(got - g_loss).max():.3e}  bar {bar:.3e}")
    assert np.abs(got - g_loss).max() <= bar
    assert (got[:, mn[0] == 0] == 0).all()                 # the image keeps its mask
    # masking the target again -- what the kernels do without the new bit -- is a different loss
    again = training_loss(a.to(DEV), None, resample_gt(b.to(DEV), o, m), None, m, lam, 0)
    assert abs(again[1].item() - Ll1.item()) > 1e-4 * l1


def test_loss_depth_pair_keeps_its_mask_and_launch_counts():
    from sfgs.loss import depth_pearson, training_loss
    c, h, w = 3, 45, 65
    lam, lamd = 0.2, 0.5
    a, b = image_pair(c, h, w, 30)
    gt, depth = depth_pair(h, w, 30)
    _, offset, mask = inputs(c, h, w, 31, mask_kind="binary")
    x, y, o, m, gtd = a.to(DEV), b.to(DEV), to_dev(offset), to_dev(mask), gt.to(DEV)
    ref, gref, bad = pearson64(gt, depth, mask, "drop")

    def leaves():
        return x.clone().requires_grad_(True), depth.to(DEV).requires_grad_(True)

    def forward(xi, di):
        return training_loss(xi, di, y, gtd, m, lam, lamd, invalid="drop", subpixel_offset=o)
    forward(*leaves())[0].backward()                                                  # warm-up
    xi, di = leaves()
    out = forward(xi, di)
    loss, Ll1, ssim, dl = out
    loss.backward()
    d0 = depth.to(DEV).requires_grad_(True)
    dl0 = depth_pearson(d0, gtd, m, "drop")
    (lamd * dl0).backward()
    assert torch.equal(dl, dl0.detach()) and abs(dl.item() - ref) <= 2.4e-7            # the depth pair took the mask
    assert torch.equal(di.grad, d0.grad)
    got = di.grad.cpu().numpy()
    assert np.abs(got - lamd * gref).max() <= 1e-5 * np.abs(lamd * gref).max()
    assert (got[bad] == 0).all() and (got[mask.numpy() == 0] == 0).all()
    Ll1_p, ssim_p = training_loss(x, None, y, None, m, lam, 0, subpixel_offset=o)[1:3]
    assert torch.equal(Ll1, Ll1_p) and torch.equal(ssim, ssim_p)
    assert abs(loss.item() - ((1 - lam) * Ll1.item() + lam * (1 - ssim.item()) + lamd * dl.item())) <= 5e-7
    # launches, the library's own counters: the three loss kernels forward, two backward, as without the keyword
    L.profile_enable(True)
    try:
        L.profile_collect()
        out = forward(*leaves())
        fwd = {k: v[1] for k, v in L.profile_collect().items()}
        out[0].backward()
        bwd = {k: v[1] for k, v in L.profile_collect().items()}
    finally:
        L.profile_enable(False)
    assert fwd == {"loss_photo_fwd": 1, "loss_depth_fwd": 1, "loss_final": 1}
    assert bwd == {"loss_photo_bwd": 1, "loss_depth_bwd": 1}
    # ... and every device kernel of the library, the one without a profiler id included: 3 + 1 forward, 2 backward
    xi, di = leaves()
    torch.cuda.synchronize()
    acts, out = device_activities(lambda: forward(xi, di))
    fwd = ours(acts)
    print("forward:", acts)
    assert sum(fwd.values()) == 4 and sum(n for k, n in fwd.items() if "resample_gt_kernel" in k) == 1
    assert not any("memcpy" in k.lower() or "memset" in k.lower() for k in acts)       # no intermediate copy, no host read
    acts, _ = device_activities(lambda: out[0].backward())
    bwd = ours(acts)
    print("backward:", bwd)
    assert sum(bwd.values()) == 2 and not any("resample_gt_kernel" in k for k in bwd)


def test_loss_with_subpixel_offset_does_not_synchronise_the_host():
    from sfgs.loss import training_loss
    c, h, w = 3, 270, 480
    a, b = image_pair(c, h, w, 40)
    gt, depth = depth_pair(h, w, 40)
    _, offset, mask = inputs(c, h, w, 41, mask_kind="binary")
    y, o, m, gtd = b.to(DEV), to_dev(offset), to_dev(mask), gt.to(DEV)
    x, d = a.to(DEV).requires_grad_(True), depth.to(DEV).requires_grad_(True)
    big = torch.randn(4096, 4096, device=DEV)
    training_loss(x, d, y, gtd, m, 0.2, 0.5, subpixel_offset=o)[0].backward()         # warm-up
    big @ big
    x.grad = d.grad = None
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(60):
            big @ big
        loss = training_loss(x, d, y, gtd, m, 0.2, 0.5, invalid="drop", subpixel_offset=o)[0]
        loss.backward()
        done.record()
        returned_early = not done.query()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    assert returned_early
    assert torch.isfinite(loss) and torch.isfinite(x.grad).all()
