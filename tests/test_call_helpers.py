"""sfgs._call on the host: every message of the shared argument checks against the literal text the operator modules raised
before they shared them (sfgs.resample.check_tensor, sfgs.loss._check_gpu, sfgs.depthvis / sfgs.geometry _check_depth and
_check_mask, sfgs.metrics._check_row, the three spellings of "same device"), and the name hook on throwaway modules. No
library, no GPU: CPU tensors and the `meta` device stand in for devices."""
import types

import pytest
import torch

from sfgs import _call


def _raises(text, fn, *args, **kwargs):
    with pytest.raises(ValueError) as e:
        fn(*args, **kwargs)
    assert str(e.value) == text


def test_check_tensor_messages_float32():
    ok = lambda t: t.dim() == 3
    _call.check_tensor("image", torch.zeros(1, 2, 3), "[C,H,W]", ok)
    _raises("image must be a tensor", _call.check_tensor, "image", [1.0], "[C,H,W]", ok)
    _raises("image must be a tensor", _call.check_tensor, "image", None, "[C,H,W]", ok)
    _raises("image must be float32, got torch.float64", _call.check_tensor, "image", torch.zeros(1, 2, 3).double(), "[C,H,W]", ok)
    _raises("image must be [C,H,W], got (2, 3)", _call.check_tensor, "image", torch.zeros(2, 3), "[C,H,W]", ok)
    _raises("gt_image must be (3, 4, 5) like image, got (3, 4, 6)", _call.check_tensor, "gt_image", torch.zeros(3, 4, 6),
            "(3, 4, 5) like image", lambda t: tuple(t.shape) == (3, 4, 5))


def test_check_tensor_messages_other_dtypes():
    ok = lambda t: t.numel() > 0
    f64 = dict(dtypes=(torch.float32, torch.float64))
    _call.check_tensor("opacity_raw", torch.zeros(4).double(), "a non-empty [N] or [N,1]", ok, **f64)
    _raises("opacity_raw must be a tensor", _call.check_tensor, "opacity_raw", 0.5, "a non-empty [N] or [N,1]", ok, **f64)
    _raises("opacity_raw must be float32 or float64, got torch.float16", _call.check_tensor, "opacity_raw",
            torch.zeros(4).half(), "a non-empty [N] or [N,1]", ok, **f64)
    _raises("opacity_raw must be a non-empty [N] or [N,1], got (0,)", _call.check_tensor, "opacity_raw", torch.zeros(0),
            "a non-empty [N] or [N,1]", ok, **f64)
    _raises("ref must be float32 or float64, got torch.int32", _call.check_tensor, "ref", torch.zeros(2, 2, dtype=torch.int32),
            "a non-empty [H,W]", ok, **f64)
    # sfgs.metrics' `out` row: float64 only, None allowed
    row = dict(dtypes=(torch.float64,), none_ok=True)
    is_row = lambda t: tuple(t.shape) == (8,) and t.is_contiguous()
    assert _call.check_tensor("out", None, "a contiguous [8]", is_row, **row) is None
    _call.check_tensor("out", torch.zeros(8).double(), "a contiguous [8]", is_row, **row)
    _raises("out must be a tensor or None", _call.check_tensor, "out", 3, "a contiguous [8]", is_row, **row)
    _raises("out must be float64, got torch.float32", _call.check_tensor, "out", torch.zeros(8), "a contiguous [8]", is_row, **row)
    _raises("out must be a contiguous [8], got (8,)", _call.check_tensor, "out", torch.zeros(16).double()[::2],
            "a contiguous [8]", is_row, **row)


def test_check_gpu_message_and_none():
    _call.check_gpu()
    _call.check_gpu(mask=None)
    _raises("depth must be a GPU tensor", _call.check_gpu, depth=torch.zeros(2, 2))
    _raises("gt_image must be a GPU tensor", _call.check_gpu, mask=None, gt_image=torch.zeros(1), image=torch.zeros(1))


def test_same_device_messages():
    cpu, other = torch.device("cpu"), torch.device("meta")
    here, there = torch.zeros(2), torch.zeros(2, device=other)
    _call.same_device(cpu, "device", depth=here, mask=None)
    _raises("mask must be on device cpu, got meta", _call.same_device, cpu, "device", depth=here, mask=there)
    _raises("out must be on image's device cpu, got meta", _call.same_device, cpu, "image's device", out=there)
    _raises("subpixel_offset must be on gt_image's device cpu, got meta", _call.same_device, cpu, "gt_image's device",
            subpixel_offset=there, mask=there)
    _raises("lut must be on depth's device meta, got cpu", _call.same_device, other, "depth's device", mask=None, lut=here)
    _raises("image must be on the Evaluator's device meta, got cpu", _call.same_device, other, "the Evaluator's device",
            image=here)
    # as a GPU is printed
    _raises("sec must be on device cuda:0, got cpu", _call.same_device, torch.device("cuda:0"), "device", sec=here)


def test_check_depth_map():
    assert _call.check_depth_map(torch.zeros(1, 4, 5)) == (4, 5)
    assert _call.check_depth_map(torch.zeros(4, 5)) == (4, 5)
    _raises("depth must be a tensor", _call.check_depth_map, [[1.0]])
    _raises("depth must be float32, got torch.float64", _call.check_depth_map, torch.zeros(4, 5).double())
    for shape in ((2, 4, 5), (5,), (1, 1, 4, 5), (1, 0, 5), (0, 5)):
        _raises(f"depth must be a non-empty [1,H,W] or [H,W], got {shape}", _call.check_depth_map, torch.zeros(shape))
    _raises("gt_depth must be float32, got torch.int64", _call.check_depth_map, torch.zeros(4, 5, dtype=torch.int64),
            name="gt_depth")


def test_check_pixel_mask():
    assert _call.check_pixel_mask(None, 4, 5) is None
    for m in (torch.zeros(4, 5, dtype=torch.bool), torch.zeros(1, 4, 5, dtype=torch.uint8)):
        _call.check_pixel_mask(m, 4, 5)
    _raises("mask must be a tensor or None", _call.check_pixel_mask, [[True]], 4, 5)
    _raises("mask must be bool or uint8, got torch.float32", _call.check_pixel_mask, torch.zeros(4, 5), 4, 5)
    _raises("mask must be [4,5] or [1,4,5], got (5, 4)", _call.check_pixel_mask, torch.zeros(5, 4, dtype=torch.bool), 4, 5)
    _raises("mask must be [4,5] or [1,4,5], got (2, 4, 5)", _call.check_pixel_mask, torch.zeros(2, 4, 5, dtype=torch.uint8), 4, 5)
    _raises("keep_mask must be a tensor or None", _call.check_pixel_mask, 1, 4, 5, "keep_mask")
    _raises("keep_mask must be bool or uint8, got torch.int32", _call.check_pixel_mask,
            torch.zeros(4, 5, dtype=torch.int32), 4, 5, name="keep_mask")
    _raises("keep_mask must be [4,5] or [1,4,5], got (4,)", _call.check_pixel_mask, torch.zeros(4, dtype=torch.bool), 4, 5,
            "keep_mask")


def _module(name, **names):
    m = types.ModuleType(name)
    vars(m).update(names)
    return m


def test_name_hook_install_and_uninstall():
    def own_f(): pass
    def own_g(): pass
    def new_f(): pass
    def new_g(): pass
    untouched = object()
    hook = _call.NameHook(f=new_f, g=new_g)
    m = _module("train_a", f=own_f, g=own_g, h=untouched)
    hook.install(m)
    assert m.f is new_f and m.g is new_g and m.h is untouched
    hook.install(m)                                   # a no-op: the replacement is not saved as the module's own
    assert m.f is new_f and m.g is new_g
    hook.uninstall(m)
    assert m.f is own_f and m.g is own_g and m.h is untouched
    hook.uninstall(m)                                 # a second uninstall is one without an install
    assert m.f is own_f and m.g is own_g


def test_name_hook_uninstall_without_install_is_a_no_op():
    def own(): pass
    hook = _call.NameHook(f=lambda: None)
    m = _module("train_b", f=own)
    before = dict(vars(m))
    hook.uninstall(m)
    assert m.f is own and dict(vars(m)) == before


def test_name_hook_tracks_modules_independently():
    def own_a(): pass
    def own_b(): pass
    def new(): pass
    hook = _call.NameHook(f=new)
    a, b = _module("train_a", f=own_a), _module("train_b", f=own_b)
    hook.install(a)
    assert a.f is new and b.f is own_b
    hook.install(b)
    hook.uninstall(a)
    assert a.f is own_a and b.f is new
    hook.install(a)                                   # after an uninstall, install works again
    assert a.f is new
    hook.uninstall(b)
    hook.uninstall(a)
    assert a.f is own_a and b.f is own_b


def test_name_hook_needs_every_name_before_it_touches_one():
    def own(): pass
    hook = _call.NameHook(f=lambda: None, missing=lambda: None)
    m = _module("train_c", f=own)
    with pytest.raises(AttributeError):
        hook.install(m)
    assert m.f is own and not hasattr(m, "missing")
    hook.uninstall(m)
    assert m.f is own
