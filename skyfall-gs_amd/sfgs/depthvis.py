"""sfgs.depthvis -- depth colorisation for depth videos and evaluation reports on HIP kernels (csrc/depthvis.hip through
libsfgs.so): `colorize_depth_torch` of the reference (render_video.py:129-170, the same function in
render_video_from_ply.py:126-167 and train.py:1001-1041) without its per-frame trip to the host.

    rgb = colorize_depth(depth)                          # float32 [3,H,W], the reference's return value, bit for bit
    rgb8 = colorize_depth(depth, out="uint8_hwc")        # uint8 [H,W,3]: what a video writer takes
    frame8 = quantize_frame(image)                       # float32 [3,H,W] -> uint8 [H,W,3] (render_video.py:264)

The reference downloads the depth map, takes `1 / depth` where `depth > 0` (and the mask), normalises with
`np.nanquantile(disp, 0.01)` and `np.nanquantile(disp, 0.99)`, looks `1 - disp` up in matplotlib's colormap, converts to
uint8 and uploads `uint8 / 255`. Here the two quantiles are exact order statistics from a radix select on the device
(three histogram passes with integer atomics), interpolated in float32 the way numpy does it, and a last pass looks up a
256-entry uint8 table: eight launches, no host read of a device value, the same bytes as the reference.

install(module) rebinds exactly `module.colorize_depth_torch` (train, render_video, render_video_from_ply) to a function
with the reference's signature; uninstall(module) restores it.

There is no torch fallback: without the HIP library every operator raises."""
import numpy as np
import torch

from . import _call
from . import _lib as L

__all__ = ["colorize_depth", "quantize_frame", "spectral_lut", "spectral_table", "install", "uninstall"]

_OUT = {"float_chw": L.DEPTHVIS_FLOAT_CHW, "uint8_hwc": L.DEPTHVIS_UINT8_HWC}

# ColorBrewer's 11-class "Spectral" (the anchors of matplotlib's colormap of that name), as 8-bit RGB
_SPECTRAL_ANCHORS = ((158, 1, 66), (213, 62, 79), (244, 109, 67), (253, 174, 97), (254, 224, 139), (255, 255, 191),
                     (230, 245, 152), (171, 221, 164), (102, 194, 165), (50, 136, 189), (94, 79, 162))


def _to_uint8_table(rgb):
    """The reference's conversion of colormap output: (clip(c, 0, 1) * 255).astype(uint8), in float64."""
    return (np.clip(np.asarray(rgb, dtype=np.float64), 0.0, 1.0) * 255).astype(np.uint8)


def spectral_table():
    """-> float64 [256,3]: the "Spectral" colormap's 256 entries before the conversion to bytes. Piecewise linear between the
    11 anchors, placed evenly on [0, 1], sampled at linspace(0, 1, 256)."""
    anchors = np.asarray(_SPECTRAL_ANCHORS, dtype=np.float64) / 255.0
    pos = np.linspace(0.0, 1.0, len(anchors))
    at = np.linspace(0.0, 1.0, 256)
    seg = np.searchsorted(pos, at)[1:-1]                      # the anchor at or right of every inner sample
    w = (at[1:-1] - pos[seg - 1]) / (pos[seg] - pos[seg - 1])
    inner = w[:, None] * (anchors[seg] - anchors[seg - 1]) + anchors[seg - 1]
    return np.concatenate([anchors[:1], inner, anchors[-1:]])


def spectral_lut():
    """-> uint8 [256,3]: spectral_table() as the reference turns colormap output into bytes."""
    return _to_uint8_table(spectral_table())


def _named_lut(cmap):
    if cmap == "Spectral":
        return spectral_lut()
    try:
        import matplotlib
    except ImportError:
        raise ValueError(f"cmap {cmap!r}: only 'Spectral' is built in, and matplotlib is not importable") from None
    try:
        cm = matplotlib.colormaps[cmap]
    except KeyError:
        raise ValueError(f"cmap {cmap!r} is not a matplotlib colormap") from None
    if cm.N != 256:
        raise ValueError(f"cmap {cmap!r} has {cm.N} entries; the kernel's table has 256")
    return _to_uint8_table(cm(np.arange(256))[:, :3])


_lut_cache = {}   # (cmap name, device) -> uint8 [256,3] on that device


def _device_lut(cmap, device):
    key = (cmap, str(device))
    if key not in _lut_cache:
        _lut_cache[key] = torch.from_numpy(_named_lut(cmap)).to(device)
    return _lut_cache[key]


def colorize_depth(depth, mask=None, normalize=True, cmap="Spectral", out="float_chw", lut=None):
    """The reference's colorize_depth_torch(depth, mask, normalize, cmap) on the device.
    depth: float32 [1,H,W] or [H,W] on the GPU; mask: None, or bool / uint8 of the same H x W (non-zero = use the pixel).
    out="float_chw" -> float32 [3,H,W] with values k / 255 (what the reference returns); out="uint8_hwc" -> uint8 [H,W,3].
    lut: a uint8 [256,3] tensor on depth's device to use instead of the named colormap. cmap other than "Spectral" is
    resolved through matplotlib when it is importable."""
    H, W = _call.check_depth_map(depth)
    _call.check_pixel_mask(mask, H, W)
    if out not in _OUT:
        raise ValueError(f"out must be 'float_chw' or 'uint8_hwc', got {out!r}")
    if lut is not None:
        if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
            raise ValueError("lut must be a uint8 tensor of shape [256,3]")
    elif not isinstance(cmap, str):
        raise ValueError(f"cmap must be a colormap name, got {cmap!r}")
    _call.check_gpu(depth=depth)
    dev = depth.device
    _call.same_device(dev, "depth's device", mask=mask, lut=lut)
    if lut is None:
        lut = _device_lut(cmap, dev)                      # ValueError for an unknown name
    lib = L.load()
    depth = depth.detach().contiguous()
    lut = lut.contiguous()
    if mask is not None:
        mask = mask.detach().contiguous()
    args = L.SfgsDepthVisArgs(L.C.sizeof(L.SfgsDepthVisArgs), H, W, depth.data_ptr(),
                              None if mask is None else mask.data_ptr(), lut.data_ptr(), int(bool(normalize)), _OUT[out])
    with torch.cuda.device(dev):
        scratch = _call.scratch(lib.sfgs_depthvis_scratch_bytes(L.C.byref(args)), dev, refused_if_zero=True)
        if out == "float_chw":
            result = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        else:
            result = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        L.check(lib.sfgs_depthvis_forward(L.C.byref(args), L.ptr(result), L.ptr(scratch), scratch.numel(),
                                          _call.stream(dev)))
    return result


def quantize_frame(image):
    """float32 [3,H,W] on the GPU -> uint8 [H,W,3]: `(img * 255 + 0.5).clip(0, 255).astype(np.uint8)` of
    render_video.py:264 on the transposed frame, in float32. NaN gives 0 (numpy leaves the conversion of NaN to an integer
    undefined); -inf gives 0 and +inf 255, as the clip does."""
    _call.check_tensor("image", image, "a non-empty [3,H,W]", lambda t: t.dim() == 3 and t.shape[0] == 3 and t.numel() > 0)
    _call.check_gpu(image=image)
    lib = L.load()
    dev = image.device
    image = image.detach().contiguous()
    H, W = int(image.shape[1]), int(image.shape[2])
    with torch.cuda.device(dev):
        result = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        L.check(lib.sfgs_frame_quantize(L.ptr(image), H, W, L.ptr(result), _call.stream(dev)))
    return result


def colorize_depth_torch(depth_tensor, mask=None, normalize=True, cmap='Spectral'):
    """The reference's signature. depth_tensor: float32 [1,H,W] on the GPU (the reference uses only [0] of the leading
    dimension); mask: None or [1,H,W] -> float32 [3,H,W] on depth_tensor.device."""
    return colorize_depth(depth_tensor[0], None if mask is None else mask[0], normalize=normalize, cmap=cmap)


_hook = _call.NameHook(colorize_depth_torch=colorize_depth_torch)


def install(module):
    """Rebind `colorize_depth_torch` in the namespace of a module that defines it (train, render_video,
    render_video_from_ply: their loops look the name up in the module's globals when they call it). A second install is a
    no-op; nothing else is patched."""
    _hook.install(module)


def uninstall(module):
    """Restore what install() replaced. Without an install: a no-op."""
    _hook.uninstall(module)
