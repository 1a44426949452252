"""sfgs._call -- what the Python wrappers of libsfgs.so do around a library call, written once: the raw stream handle, the
scratch buffer, the argument checks and their messages, and the rebinding of names in a caller's module. Plain functions
that a wrapper calls in the order it needs: dtype / shape checks first (they need no device), device checks after them,
L.load() last -- so a wrong argument is reported on a machine with no GPU and no library. (_lib.py stays ctypes-only and
imports without torch; this module is where torch comes in.)"""
import torch

from . import _lib as L


def stream(dev):
    """The current stream of `dev` as the `void* stream` argument of a library call."""
    return L.C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def scratch(nbytes, dev, refused_if_zero=False):
    """uint8 [max(nbytes, 1)] on `dev` for a `*_scratch_bytes` answer. refused_if_zero: this entry point answers 0 when it
    refuses its arguments, and the library's message becomes a RuntimeError."""
    if refused_if_zero and nbytes == 0:
        raise RuntimeError(f"libsfgs: {L.load().sfgs_last_error().decode(errors='replace')}")
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)


def check_tensor(name, t, shape_text, ok_shape, dtypes=(torch.float32,), none_ok=False):
    """A tensor of one of `dtypes` for which ok_shape(t) holds, or ValueError naming the argument."""
    if t is None and none_ok:
        return
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor{' or None' if none_ok else ''}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d).removeprefix('torch.') for d in dtypes)}, got {t.dtype}")
    if not ok_shape(t):
        raise ValueError(f"{name} must be {shape_text}, got {tuple(t.shape)}")


def check_gpu(**tensors):
    """After every dtype / shape check, and still before the library is loaded. None is skipped."""
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise ValueError(f"{name} must be a GPU tensor")


def same_device(dev, what, **tensors):
    """Every tensor (None is skipped) is on `dev`; `what` names that device in the message: "device", "image's device"."""
    for name, t in tensors.items():
        if t is not None and t.device != dev:
            raise ValueError(f"{name} must be on {what} {dev}, got {t.device}")


def check_depth_map(depth, name="depth"):
    """float32 [1,H,W] or [H,W] -> (H, W)"""
    check_tensor(name, depth, "a non-empty [1,H,W] or [H,W]",
                 lambda t: (t.dim() == 2 or (t.dim() == 3 and t.shape[0] == 1)) and t.numel() > 0)
    return int(depth.shape[-2]), int(depth.shape[-1])


def check_pixel_mask(mask, H, W, name="mask"):
    """None, or bool / uint8 [H,W] or [1,H,W] (non-zero = use the pixel)."""
    check_tensor(name, mask, f"[{H},{W}] or [1,{H},{W}]", lambda t: tuple(t.shape) in ((H, W), (1, H, W)),
                 dtypes=(torch.bool, torch.uint8), none_ok=True)


class NameHook:
    """Rebinds names in the globals of a caller's module (the reference looks its helpers up there when it calls them) and
    puts the module's own objects back. Nothing else is patched."""

    def __init__(self, **replacements):
        self.replacements = replacements
        self._saved = {}   # module -> {name: the module's own object}

    def install(self, module):
        """A second install is a no-op."""
        if module in self._saved:
            return
        self._saved[module] = {name: getattr(module, name) for name in self.replacements}
        for name, new in self.replacements.items():
            setattr(module, name, new)

    def uninstall(self, module):
        """Without an install: a no-op."""
        for name, own in self._saved.pop(module, {}).items():
            setattr(module, name, own)
