"""The opacity regulariser of an UNCHANGED train.py (:236-242, and :834-843 in the IDU episode) on the HIP kernels of
sfgs.loss.opacity_entropy:

    opacity = gaussians.get_opacity.clamp(1.0e-3, 1.0 - 1.0e-3)
    opacity_loss = torch.nn.functional.binary_cross_entropy(opacity, opacity)
    loss += opt.lambda_opacity * opacity_loss

The statements live in a function body and spell the cross entropy through the module global `torch`, so there is no name to
rebind (what sfgs.loss.install does for l1_loss). Instead `install(GaussianModel)` patches the `get_opacity` property: for
a GPU `_opacity` of float32 / float64 it returns an `OpacityHandle`, a storage-less tensor (sfgs/_handles.py) that stands for
`sigmoid(_opacity)`. The handle records exactly ONE operation, `clamp` with two Python numbers, which yields a second handle;
`binary_cross_entropy(h, h)` of that SAME clamped handle with no weight and reduction 'mean' runs the fused operator on the
raw parameter (two launches forward, one backward, nothing N-sized in between). Every other use of either handle --
`get_opacity < min_opacity`, add_histogram, arithmetic, indexing, another target, another reduction -- first becomes the
reference's own value (the original getter on the live parameter, with its autograd graph; then `.clamp(lo, hi)`) and
proceeds in torch, so no other caller of the getter sees a difference.

A handle remembers `_opacity._version`. Used after the parameter was modified in place (or replaced on the model) it raises
a RuntimeError instead of silently showing new values (ADVICE on sfgs.max_radii); the getter hands out a fresh handle on
every read, so the training loop never meets this. `materialisations` counts the handles that had to become real tensors."""
import torch
import torch.nn.functional as F

from . import _handles
from . import loss as _loss

__all__ = ["install", "uninstall", "OpacityHandle", "materialisations"]

materialisations = 0          # handles (plain or clamped) that were turned into the tensor they stand for
_HANDLE_DEVICES = {"cuda"}    # device types the getter answers with a handle; everything else gets the original getter

_METADATA = frozenset(("dim", "ndimension", "numel", "nelement", "size", "__len__", "is_contiguous", "element_size",
                       "is_floating_point", "is_complex", "stride", "storage_offset"))


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _clamp_bounds(input, min=None, max=None, *, out=None):
    """(lo, hi) when the call is clamp(handle, number, number); None otherwise."""
    return (min, max) if out is None and _is_number(min) and _is_number(max) else None


def _bce_pair(input, target, weight=None, size_average=None, reduce=None, reduction="mean"):
    """The handle when the call is binary_cross_entropy(h, h) in its default form; None otherwise."""
    plain = weight is None and size_average is None and reduce is None and reduction == "mean"
    return input if plain and input is target and isinstance(input, OpacityHandle) else None


class OpacityHandle(torch.Tensor):
    """`sigmoid(_opacity)` (bounds None) or `sigmoid(_opacity).clamp(lo, hi)` not yet computed."""

    @staticmethod
    def __new__(cls, param, owner, getter, version, bounds=None, parent=None):
        t = torch.Tensor._make_wrapper_subclass(cls, param.shape, dtype=param.dtype, device=param.device,
                                                requires_grad=torch.is_grad_enabled() and param.requires_grad)
        t._sfgs_param, t._sfgs_owner, t._sfgs_getter, t._sfgs_version = param, owner, getter, version
        t._sfgs_bounds, t._sfgs_parent, t._sfgs_real = bounds, parent, None
        return t

    def _check_fresh(self):
        if self._sfgs_param._version != self._sfgs_version or getattr(self._sfgs_owner, "_opacity", None) is not self._sfgs_param:
            raise RuntimeError("sfgs.opacity_reg: `_opacity` was modified in place (or replaced) after this get_opacity "
                               "result was taken; read get_opacity again instead of keeping its result across the update")

    def materialise(self):
        """The tensor this handle stands for, computed once by the reference's own getter (and torch's clamp)."""
        global materialisations
        if self._sfgs_real is None:
            if self._sfgs_parent is not None:
                self._sfgs_real = self._sfgs_parent.materialise().clamp(*self._sfgs_bounds)
            else:
                self._check_fresh()
                self._sfgs_real = self._sfgs_getter(self._sfgs_owner)
            materialisations += 1
        return self._sfgs_real

    def _fused_bounds(self):
        """(lo, hi) when the fused operator can stand for this clamped handle; None otherwise."""
        if self._sfgs_bounds is None or self._sfgs_real is not None:
            return None
        lo, hi = (torch.tensor(v, dtype=self.dtype).item() for v in self._sfgs_bounds)   # as clamp rounds them
        return (self._sfgs_bounds if 0.0 < lo < hi < 1.0 else None)

    @classmethod
    def _unwrap(cls, x):
        if isinstance(x, OpacityHandle):
            return x.materialise()
        if isinstance(x, (list, tuple)):
            return type(x)(cls._unwrap(y) for y in x)
        if isinstance(x, dict):
            return {k: cls._unwrap(v) for k, v in x.items()}
        return x

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        if name == "__get__":
            if not _handles.answered_by_wrapper(func):
                # .grad, .grad_fn, ._version, .data ...: properties of the tensor the handle stands for, read from it
                return getattr(args[0].materialise(), _handles.property_name(func))
            if _handles.property_name(func) == "is_leaf":
                return not args[0].requires_grad          # the result of sigmoid is a leaf only when it needs no gradient
        if name == "__get__" or name in _METADATA:        # shape, dtype, device, ...: answered by the wrapper's metadata
            with torch._C.DisableTorchFunctionSubclass():
                return func(*args, **kwargs)
        if func in (torch.Tensor.clamp, torch.clamp) and args and isinstance(args[0], OpacityHandle) \
                and args[0]._sfgs_bounds is None and args[0]._sfgs_real is None:
            try:
                bounds = _clamp_bounds(*args, **kwargs)
            except TypeError:
                bounds = None
            if bounds is not None:
                h = args[0]
                return OpacityHandle(h._sfgs_param, h._sfgs_owner, h._sfgs_getter, h._sfgs_version, bounds, h)
        if func is F.binary_cross_entropy:
            try:
                h = _bce_pair(*args, **kwargs)
            except TypeError:
                h = None
            bounds = h._fused_bounds() if h is not None else None
            if bounds is not None:
                h._check_fresh()
                return _loss.opacity_entropy(h._sfgs_param, *bounds)
        return func(*cls._unwrap(args), **cls._unwrap(kwargs))

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):   # backstop: nothing should get here unmaterialised
        return func(*cls._unwrap(args), **cls._unwrap(kwargs or {}))


def _wants_handle(p):
    return (isinstance(p, torch.Tensor) and p.device.type in _HANDLE_DEVICES and p.dtype in (torch.float32, torch.float64)
            and p.numel() > 0 and (p.dim() == 1 or (p.dim() == 2 and p.shape[1] == 1)))


_ORIG = {}   # class -> its own get_opacity property object


def install(gaussian_model_cls):
    """Patch `get_opacity` of the reference's GaussianModel (see the module text). A second install is a no-op, and so is
    an install on a class that defines no `get_opacity` property of its own."""
    orig = gaussian_model_cls.__dict__.get("get_opacity")
    if gaussian_model_cls in _ORIG or not isinstance(orig, property):
        return
    _ORIG[gaussian_model_cls] = orig

    def get_opacity(self):
        p = getattr(self, "_opacity", None)
        if not _wants_handle(p):
            return orig.fget(self)
        return OpacityHandle(p, self, orig.fget, p._version)

    gaussian_model_cls.get_opacity = property(get_opacity)


def uninstall(gaussian_model_cls):
    """Put the original property object back. Without an install: a no-op."""
    orig = _ORIG.pop(gaussian_model_cls, None)
    if orig is not None:
        gaussian_model_cls.get_opacity = orig
