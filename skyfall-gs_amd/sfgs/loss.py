"""sfgs.loss -- the training loss between render() and loss.backward() (reference train.py:205-234, and :760-799 in the
IDU episode) on HIP kernels: masked L1 + D-SSIM + Pearson depth term in THREE launches forward and TWO backward
(csrc/loss.hip through libsfgs.so), with no host read of a device value.

    loss, Ll1, ssim, depth_loss = training_loss(image, depth, gt_image, gt_depth, mask, lambda_dssim, lambda_depth)

replaces (for people who edit their copy of train.py) the four `mask *` products, l1_loss, fused_ssim, the NaN / Inf scrub
of the depth pair and pearson_corrcoef; all four scalars are differentiable, so a caller can still add terms of its own.
photometric() and depth_pearson() are the two halves. l1_loss() and pearson_corrcoef() are drop-ins for
utils.loss_utils.l1_loss and torchmetrics.functional.regression.pearson_corrcoef built on the same kernels;
install(train_module) rebinds exactly those two names in the module that holds the training loop (and nothing else: no lazy
tensors, no tensor subclass, no patching of torch or of a class), uninstall(train_module) restores them.

    loss = loss + lambda_opacity * opacity_entropy(gaussians._opacity)

is the opacity regulariser of train.py:236-242 / :834-843 (`get_opacity.clamp(1e-3, 1 - 1e-3)` and
`binary_cross_entropy(opacity, opacity)`) on the raw opacity: two launches forward, one backward (csrc/opacity_reg.hip). The
route for an UNCHANGED train.py is sfgs.opacity_reg.install(GaussianModel).

training_loss(..., subpixel_offset=offset) and photometric(..., subpixel_offset=offset) are the jittered mode
(`--ray_jitter --resample_gt_image`, train.py:214-215 / :770-771): the target becomes
sfgs.resample.resample_gt(gt_image, offset, mask) -- one more launch forward -- and the photometric kernels take it as
given instead of multiplying the mask in a second time (a masked-out pixel next to kept ones is not zero after resampling).

There is no torch fallback: without the HIP library every operator raises."""
import torch

from . import _call
from . import _lib as L
from . import resample as _resample

__all__ = ["training_loss", "photometric", "depth_pearson", "l1_loss", "pearson_corrcoef", "opacity_entropy", "install",
           "uninstall"]

_INVALID = {"zero": L.LOSS_INVALID_ZERO, "drop": L.LOSS_INVALID_DROP}
OUT_LOSS, OUT_L1, OUT_SSIM, OUT_DEPTH, OUT_R = range(5)


def _check_mask(mask, H, W):
    if mask is None:
        return
    _call.check_tensor("mask", mask, f"None, (1,1,1) or [1,{H},{W}]",
                       lambda t: tuple(t.shape) in ((1, 1, 1), (1, H, W)))


def _check_invalid(invalid):
    if invalid not in _INVALID:
        raise ValueError(f"invalid must be 'zero' or 'drop', got {invalid!r}")
    return _INVALID[invalid]


def _check_images(image, gt_image):
    _call.check_tensor("image", image, "[C,H,W]", lambda t: t.dim() == 3 and t.numel() > 0)
    _call.check_tensor("gt_image", gt_image, f"{tuple(image.shape)} like image", lambda t: t.shape == image.shape)
    return tuple(int(v) for v in image.shape)


def _check_depths(depth, gt_depth, H=None, W=None):
    want = "[1,H,W]" if H is None else f"[1,{H},{W}]"
    _call.check_tensor("depth", depth, want, lambda t: t.dim() == 3 and t.shape[0] == 1 and t.numel() > 0 and
                       (H is None or tuple(t.shape[1:]) == (H, W)))
    _call.check_tensor("gt_depth", gt_depth, f"{tuple(depth.shape)} like depth", lambda t: t.shape == depth.shape)
    return int(depth.shape[1]), int(depth.shape[2])


class _Loss(torch.autograd.Function):
    """out5 = (loss, Ll1, ssim, depth_loss, r) from one library call; the backward is one library call too. `first` /
    `second` are the streaming pair in the reference's argument order (gt_depth, depth)."""

    @staticmethod
    def forward(ctx, image, gt_image, first, second, mask, shape, lambda_dssim, lambda_depth, invalid, terms):
        lib = L.load()
        Cc, H, W = shape
        ref = image if image is not None else second
        dev = ref.device
        with_grad = bool(image is not None and ctx.needs_input_grad[0])
        args = L.SfgsLossArgs(L.C.sizeof(L.SfgsLossArgs), Cc, H, W,
                              None if image is None else image.data_ptr(), None if gt_image is None else gt_image.data_ptr(),
                              None if second is None else second.data_ptr(), None if first is None else first.data_ptr(),
                              None if mask is None else mask.data_ptr(), 0 if mask is None else mask.numel(),
                              float(lambda_dssim), float(lambda_depth), int(invalid), int(terms), int(with_grad), 0)
        with torch.cuda.device(dev):
            scratch = _call.scratch(lib.sfgs_loss_scratch_bytes(L.C.byref(args)), dev, refused_if_zero=True)
            out = torch.empty(5, dtype=torch.float32, device=dev)
            L.check(lib.sfgs_loss_forward(L.C.byref(args), L.ptr(out), L.ptr(scratch), scratch.numel(),
                                          _call.stream(dev)))
        ctx.args = args
        ctx.save_for_backward(scratch, image, gt_image, first, second, mask)   # the pointers in `args` stay valid
        ctx.want = (with_grad, bool(second is not None and ctx.needs_input_grad[3]),
                    bool(first is not None and ctx.needs_input_grad[2]))
        return out

    @staticmethod
    def backward(ctx, g_out):
        lib = L.load()
        scratch, image, _, first, second, _ = ctx.saved_tensors
        want_image, want_second, want_first = ctx.want
        dev = scratch.device
        with torch.cuda.device(dev):
            g = g_out.contiguous()
            g_image = torch.empty_like(image) if want_image else None
            g_second = torch.empty_like(second) if want_second else None
            g_first = torch.empty_like(first) if want_first else None
            L.check(lib.sfgs_loss_backward(L.C.byref(ctx.args), L.ptr(scratch), L.ptr(g), L.ptr(g_image), L.ptr(g_second),
                                           L.ptr(g_first), _call.stream(dev)))
        return g_image, None, g_first, g_second, None, None, None, None, None, None


def _mask_arg(mask):
    return None if mask is None else mask.contiguous().detach()


def _jittered_target(gt_image, subpixel_offset, mask, shape):
    """The checked, contiguous target resampled at the jittered rays (mask applied to the taps): one launch."""
    return _resample.run(gt_image, subpixel_offset.detach().contiguous(), mask, shape)


def training_loss(image, depth, gt_image, gt_depth, mask, lambda_dssim, lambda_depth, invalid="zero", subpixel_offset=None):
    """-> (loss, Ll1, ssim, depth_loss), four differentiable device scalars (train.py:205-234 with invalid="zero",
    :760-799 with invalid="drop"). image, gt_image: [C,H,W]; depth, gt_depth: [1,H,W] or None (then lambda_depth must be
    0 and depth_loss is 0); mask: None, (1,1,1) or [1,H,W]. Gradients reach image and depth.
    subpixel_offset: None, or the [H,W,2] offsets render() was given (resample_gt_image): mask * image is then compared with
    resample_gt(gt_image, subpixel_offset, mask); the depth pair keeps its mask."""
    mode = _check_invalid(invalid)
    Cc, H, W = _check_images(image, gt_image)
    _check_mask(mask, H, W)
    if subpixel_offset is not None:
        _resample.check_shapes(gt_image, subpixel_offset, None, name="gt_image")
    terms = L.LOSS_PHOTOMETRIC
    if depth is None or gt_depth is None:
        if depth is not None or gt_depth is not None:
            raise ValueError("depth and gt_depth must both be given or both be None")
        if lambda_depth != 0:
            raise ValueError("lambda_depth must be 0 without depth and gt_depth")
    else:
        _check_depths(depth, gt_depth, H, W)
        terms |= L.LOSS_DEPTH
    _call.check_gpu(image=image, gt_image=gt_image, depth=depth, gt_depth=gt_depth, mask=mask)
    if subpixel_offset is not None:
        _resample.check_devices(gt_image, subpixel_offset, mask, name="gt_image")
    if depth is not None:
        depth, gt_depth = depth.contiguous(), gt_depth.contiguous().detach()
    gt_image, mask = gt_image.contiguous().detach(), _mask_arg(mask)
    if subpixel_offset is not None:
        gt_image = _jittered_target(gt_image, subpixel_offset, mask, (Cc, H, W))
        terms |= L.LOSS_GT_PREMASKED
    out = _Loss.apply(image.contiguous(), gt_image, gt_depth, depth, mask, (Cc, H, W), lambda_dssim, lambda_depth, mode, terms)
    o = out.unbind(0)
    return o[OUT_LOSS], o[OUT_L1], o[OUT_SSIM], o[OUT_DEPTH]


def photometric(image, gt_image, mask=None, subpixel_offset=None):
    """-> (Ll1, ssim) of mask * image against mask * gt_image: l1_loss and fused_ssim in one launch (plus the
    finalisation). Without a mask, or with one of ones, ssim is bit-identical to fused_ssim(image[None], gt_image[None]).
    subpixel_offset: None or [H,W,2] -- the second operand is then resample_gt(gt_image, subpixel_offset, mask), as given."""
    Cc, H, W = _check_images(image, gt_image)
    _check_mask(mask, H, W)
    if subpixel_offset is not None:
        _resample.check_shapes(gt_image, subpixel_offset, None, name="gt_image")
    _call.check_gpu(image=image, gt_image=gt_image, mask=mask)
    if subpixel_offset is not None:
        _resample.check_devices(gt_image, subpixel_offset, mask, name="gt_image")
    terms = L.LOSS_PHOTOMETRIC
    gt_image, mask = gt_image.contiguous().detach(), _mask_arg(mask)
    if subpixel_offset is not None:
        gt_image = _jittered_target(gt_image, subpixel_offset, mask, (Cc, H, W))
        terms |= L.LOSS_GT_PREMASKED
    out = _Loss.apply(image.contiguous(), gt_image, None, None, mask, (Cc, H, W), 0.0, 0.0, L.LOSS_INVALID_ZERO, terms)
    o = out.unbind(0)
    return o[OUT_L1], o[OUT_SSIM]


def depth_pearson(depth, gt_depth, mask=None, invalid="zero"):
    """-> 1 - pearson_corrcoef(mask * gt_depth, mask * depth) with the NaN / Inf scrub of train.py:229-231 ("zero": a pair
    with a non-finite member becomes (0, 0)) or :788-790 ("drop": it is left out; n = 0 gives NaN)."""
    mode = _check_invalid(invalid)
    H, W = _check_depths(depth, gt_depth)
    _check_mask(mask, H, W)
    _call.check_gpu(depth=depth, gt_depth=gt_depth, mask=mask)
    out = _Loss.apply(None, None, gt_depth.contiguous().detach(), depth.contiguous(), _mask_arg(mask), (1, H, W), 0.0, 0.0,
                      mode, L.LOSS_DEPTH)
    return out[OUT_DEPTH]


def l1_loss(network_output, gt):
    """utils.loss_utils.l1_loss: mean |network_output - gt| (one streaming launch plus the finalisation)."""
    _call.check_tensor("network_output", network_output, "a non-empty tensor", lambda t: t.numel() > 0)
    _call.check_tensor("gt", gt, f"{tuple(network_output.shape)} like network_output",
                       lambda t: t.shape == network_output.shape)
    _call.check_gpu(network_output=network_output, gt=gt)
    n = network_output.numel()
    out = _Loss.apply(None, None, network_output.contiguous().view(-1), gt.contiguous().view(-1), None, (1, 1, n), 0.0, 0.0,
                      L.LOSS_INVALID_KEEP, L.LOSS_L1_STREAM)
    return out[OUT_L1]


def pearson_corrcoef(preds, target):
    """torchmetrics.functional.regression.pearson_corrcoef for float32 [P] or [P,1] inputs: r clamped to [-1, 1], no
    scrub (a NaN in the inputs gives NaN). Differentiable w.r.t. both arguments."""
    ok = lambda t: t.numel() > 0 and (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1))
    _call.check_tensor("preds", preds, "[P] or [P,1]", ok)
    _call.check_tensor("target", target, f"{tuple(preds.shape)} like preds", lambda t: t.shape == preds.shape)
    _call.check_gpu(preds=preds, target=target)
    n = preds.shape[0]
    out = _Loss.apply(None, None, preds.contiguous().view(-1), target.contiguous().view(-1), None, (1, 1, n), 0.0, 0.0,
                      L.LOSS_INVALID_KEEP, L.LOSS_DEPTH)
    return out[OUT_R]


class _OpacityEntropy(torch.autograd.Function):
    """mean h(clamp(sigmoid(x), lo, hi)) of the raw opacity x, one library call each way; nothing N-sized is saved but x."""

    @staticmethod
    def forward(ctx, x, lo, hi):
        lib = L.load()
        dev = x.device
        with_grad = bool(ctx.needs_input_grad[0])
        args = L.SfgsOpacityEntropyArgs(L.C.sizeof(L.SfgsOpacityEntropyArgs), x.numel(), x.data_ptr(),
                                        int(x.dtype == torch.float64), float(lo), float(hi), int(with_grad))
        with torch.cuda.device(dev):
            scratch = _call.scratch(lib.sfgs_opacity_entropy_scratch_bytes(L.C.byref(args)), dev, refused_if_zero=True)
            out = torch.empty((), dtype=x.dtype, device=dev)
            L.check(lib.sfgs_opacity_entropy_forward(L.C.byref(args), L.ptr(out), L.ptr(scratch), scratch.numel(),
                                                     _call.stream(dev)))
        ctx.args = args
        ctx.save_for_backward(x)   # the pointer in `args` stays valid
        return out

    @staticmethod
    def backward(ctx, g_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        lib = L.load()
        x, = ctx.saved_tensors
        dev = x.device
        with torch.cuda.device(dev):
            g = g_out.contiguous()
            grad = torch.empty_like(x)
            L.check(lib.sfgs_opacity_entropy_backward(L.C.byref(ctx.args), L.ptr(g), L.ptr(grad), _call.stream(dev)))
        return grad, None, None


def _check_bounds(lo, hi, dtype):
    """0 < lo < hi < 1 must hold for the bounds as torch's clamp takes them: rounded to the tensor's dtype."""
    numbers = all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in (lo, hi))
    if not numbers or not 0.0 < torch.tensor(lo, dtype=dtype).item() < torch.tensor(hi, dtype=dtype).item() < 1.0:
        raise ValueError(f"lo and hi must be numbers with 0 < lo < hi < 1 in {dtype}, got {lo!r}, {hi!r}")


def opacity_entropy(opacity_raw, lo=1e-3, hi=1 - 1e-3):
    """-> mean over the N Gaussians of binary_cross_entropy(o, o), o = sigmoid(opacity_raw).clamp(lo, hi): the
    lambda_opacity term of train.py:236-242 / :834-843, a differentiable device scalar of the input's dtype.
    opacity_raw: [N] or [N,1], float32 or float64 (`_opacity` after the first reset_opacity), on the GPU."""
    _call.check_tensor("opacity_raw", opacity_raw, "a non-empty [N] or [N,1]",
                       lambda t: (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1)) and t.numel() > 0,
                       dtypes=(torch.float32, torch.float64))
    _check_bounds(lo, hi, opacity_raw.dtype)
    _call.check_gpu(opacity_raw=opacity_raw)
    return _OpacityEntropy.apply(opacity_raw.contiguous().view(-1), lo, hi)


_hook = _call.NameHook(l1_loss=l1_loss, pearson_corrcoef=pearson_corrcoef)


def install(train_module):
    """Rebind `l1_loss` and `pearson_corrcoef` in the namespace of the module that holds the training loop (train.py
    looks both up in its globals when called; depth_loss_func reaches pearson_corrcoef the same way). A second install
    is a no-op."""
    _hook.install(train_module)


def uninstall(train_module):
    """Restore what install() replaced. Without an install: a no-op."""
    _hook.uninstall(train_module)
