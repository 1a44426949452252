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

from . import _call
from . import _lib as L

__all__ = ["resample_gt", "create_offset_gt", "install", "uninstall"]

check_tensor = _call.check_tensor    # importable from here as before


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
    # spelled out, not _call.check_gpu + _call.same_device: at 1024 x 1024 without a mask the call is bound by the host, and
    # the two keyword-argument calls cost it 0.5 us of 12 (profiles/r13_wrapper_plumbing_ab.txt)
    for n, t in ((name, image), ("subpixel_offset", subpixel_offset), ("mask", mask)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"{n} must be a GPU tensor")
    for n, t in (("subpixel_offset", subpixel_offset), ("mask", mask)):
        if t is not None and t.device != image.device:
            raise ValueError(f"{n} must be on {name}'s device {image.device}, got {t.device}")


def run(image, subpixel_offset, mask, shape):
    """The checked arguments, contiguous -> the resampled [C,H,W] on the current stream of image's device."""
    lib = L.load()
    Cc, H, W = shape
    dev = image.device
    args = L.SfgsResampleArgs(L.C.sizeof(L.SfgsResampleArgs), Cc, H, W, image.data_ptr(),
                              None if mask is None else mask.data_ptr(), 0 if mask is None else mask.numel(),
                              subpixel_offset.data_ptr())
    with torch.cuda.device(dev):
        out = torch.empty((Cc, H, W), dtype=torch.float32, device=dev)
        L.check(lib.sfgs_resample_gt(L.C.byref(args), L.ptr(out), _call.stream(dev)))
    return out


def resample_gt(image, subpixel_offset, mask=None):
    """-> float32 [C,H,W]: bilinear samples of mask * image at (x + ox, y + oy), clamped to the frame (grid_sample with
    padding_mode="border", align_corners=True). image: [C,H,W] float32 on the GPU, C <= 4; subpixel_offset: [H,W,2], channel 0
    = x, channel 1 = y -- what render() was given; mask: None, (1,1,1) or [1,H,W]. Non-finite offsets: NaN and -inf sample
    column / row 0, +inf the last one. The result never requires grad (the reference's function is @torch.no_grad())."""
    shape = check_shapes(image, subpixel_offset, mask)
    check_devices(image, subpixel_offset, mask)
    return run(image.detach().contiguous(), subpixel_offset.detach().contiguous(),
               None if mask is None else mask.detach().contiguous(), shape)


def create_offset_gt(image, offset):
    """The reference's signature (train.py:64-77): image is the already masked [C,H,W] ground truth."""
    return resample_gt(image, offset)


_hook = _call.NameHook(create_offset_gt=create_offset_gt)


def install(train_module):
    """Rebind `create_offset_gt` in the namespace of the module that holds the training loop (train.py looks the name up in
    its globals at :215 and :771). A second install is a no-op; nothing else is patched."""
    _hook.install(train_module)


def uninstall(train_module):
    """Restore what install() replaced. Without an install: a no-op."""
    _hook.uninstall(train_module)
