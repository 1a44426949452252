"""sfgs.resample -- the jittered ground truth of `--ray_jitter --resample_gt_image` on a HIP kernel (csrc/resample.hip through
libsfgs.so): `create_offset_gt` of the reference (train.py:64-77) applied to `mask * original_image` (train.py:207, 214-215;
:770-771 in the IDU episode), so that the target is sampled where the jittered rays of render(subpixel_offset=...) went.

    gt_image = resample_gt(viewpoint_cam.original_image, subpixel_offset, mask)      # float32 [C,H,W], never requires grad

The reference rebuilds the pixel grid on the host every iteration (np.meshgrid of Python ranges, stack, cast, a pageable
upload), normalises it in six elementwise launches and calls grid_sample(bilinear, padding_mode="border",
align_corners=True). Here the pixel's coordinate comes from the thread index: one launch, no intermediate tensor, no host
read. The mask is applied to the four taps, as the reference's order of statements does.

create_offset_gt(image, offset) has the reference's signature; install(train_module) rebinds exactly that name in the
module that holds the training loop (train.py looks it up in its globals at both call sites), uninstall(train_module)
restores it. sfgs.loss.training_loss(..., subpixel_offset=...) covers the whole block between render() and backward() for
this mode.

There is no torch fallback: without the HIP library every operator raises."""
import torch

from . import _lib as L

__all__ = ["resample_gt", "create_offset_gt", "install", "uninstall"]


def check_tensor(name, t, shape_text, ok_shape):
    """float32 tensor of an accepted shape, or ValueError naming the argument (sfgs.loss uses the same check)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if not ok_shape(t):
        raise ValueError(f"{name} must be {shape_text}, got {tuple(t.shape)}")


def check_shapes(image, subpixel_offset, mask, name="image"):
    """The dtype / shape checks (they need no device). -> (C, H, W)"""
    check_tensor(name, image, "[C,H,W] with 1 <= C <= 4, H >= 2 and W >= 2",
                  lambda t: t.dim() == 3 and 1 <= t.shape[0] <= 4 and t.shape[1] >= 2 and t.shape[2] >= 2)
    Cc, H, W = (int(v) for v in image.shape)
    if Cc * H * W >= 1 << 31:
        raise ValueError(f"{name} must hold fewer than 2^31 elements, got {tuple(image.shape)}")
    check_tensor("subpixel_offset", subpixel_offset, f"[{H},{W},2]", lambda t: tuple(t.shape) == (H, W, 2))
    if mask is not None:
        check_tensor("mask", mask, f"None, (1,1,1) or [1,{H},{W}]", lambda t: tuple(t.shape) in ((1, 1, 1), (1, H, W)))
    return Cc, H, W


def check_devices(image, subpixel_offset, mask, name="image"):
    """After every dtype / shape check, and still before the library is loaded: GPU tensors on one device."""
    for n, t in ((name, image), ("subpixel_offset", subpixel_offset), ("mask", mask)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"{n} must be a GPU tensor")
    for n, t in (("subpixel_offset", subpixel_offset), ("mask", mask)):
        if t is not None and t.device != image.device:
            raise ValueError(f"{n} must be on {name}'s device {image.device}, got {t.device}")


def _run(image, subpixel_offset, mask, shape):
    """The checked arguments, contiguous -> the resampled [C,H,W] on the current stream of image's device."""
    lib = L.load()
    Cc, H, W = shape
    dev = image.device
    args = L.SfgsResampleArgs(L.C.sizeof(L.SfgsResampleArgs), Cc, H, W, image.data_ptr(),
                              None if mask is None else mask.data_ptr(), 0 if mask is None else mask.numel(),
                              subpixel_offset.data_ptr())
    with torch.cuda.device(dev):
        stream = L.C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        out = torch.empty((Cc, H, W), dtype=torch.float32, device=dev)
        L.check(lib.sfgs_resample_gt(L.C.byref(args), L.ptr(out), stream))
    return out


def resample_gt(image, subpixel_offset, mask=None):
    """-> float32 [C,H,W]: bilinear samples of mask * image at (x + ox, y + oy), clamped to the frame (grid_sample with
    padding_mode="border", align_corners=True). image: [C,H,W] float32 on the GPU, C <= 4; subpixel_offset: [H,W,2], channel 0
    = x, channel 1 = y -- what render() was given; mask: None, (1,1,1) or [1,H,W]. Non-finite offsets: NaN and -inf sample
    column / row 0, +inf the last one. The result never requires grad (the reference's function is @torch.no_grad())."""
    shape = check_shapes(image, subpixel_offset, mask)
    check_devices(image, subpixel_offset, mask)
    return _run(image.detach().contiguous(), subpixel_offset.detach().contiguous(),
                None if mask is None else mask.detach().contiguous(), shape)


def create_offset_gt(image, offset):
    """The reference's signature (train.py:64-77): image is the already masked [C,H,W] ground truth."""
    return resample_gt(image, offset)


_NAME = "create_offset_gt"
_saved = {}   # module -> its own create_offset_gt


def install(train_module):
    """Rebind `create_offset_gt` in the namespace of the module that holds the training loop (train.py looks the name up in
    its globals at :215 and :771). A second install is a no-op; nothing else is patched."""
    if train_module in _saved:
        return
    _saved[train_module] = getattr(train_module, _NAME)
    setattr(train_module, _NAME, create_offset_gt)


def uninstall(train_module):
    """Restore what install() replaced. Without an install: a no-op."""
    if train_module in _saved:
        setattr(train_module, _NAME, _saved.pop(train_module))
