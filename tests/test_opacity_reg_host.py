"""sfgs.loss.opacity_entropy and sfgs.opacity_reg without a GPU: the argument checks run before the library is loaded, the
C header, the library and the ctypes binding agree on the three entry points, the entry points validate their arguments
before any HIP call, and the get_opacity handle of sfgs.opacity_reg -- on CPU tensors, with the fused entry replaced by a
torch restatement -- recognises exactly the regulariser's statements and is the reference's own tensor for everything
else. The kernels themselves: tests/test_gpu_opacity_reg.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from sfgs import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
ENTRY_POINTS = ("sfgs_opacity_entropy_scratch_bytes", "sfgs_opacity_entropy_forward", "sfgs_opacity_entropy_backward")


# ---- sfgs.loss.opacity_entropy: validation -------------------------------------------------------------------------------------
def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    from sfgs import loss
    assert "opacity_entropy" in loss.__all__

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load", no_library)
    x = torch.zeros(8, 1)
    with pytest.raises(ValueError, match="opacity_raw must be a tensor"):
        loss.opacity_entropy([0.0, 1.0])
    for bad in (x.half(), x.long(), x.bfloat16()):
        with pytest.raises(ValueError, match="opacity_raw must be float32 or float64"):
            loss.opacity_entropy(bad)
    for bad in (torch.zeros(8, 2), torch.zeros(2, 4, 1), torch.zeros(()), torch.zeros(1, 8)):
        with pytest.raises(ValueError, match=r"\[N\] or \[N,1\]"):
            loss.opacity_entropy(bad)
    for empty in (torch.zeros(0), torch.zeros(0, 1)):
        with pytest.raises(ValueError, match="non-empty"):
            loss.opacity_entropy(empty)
    for lo, hi in ((0.0, 0.5), (0.5, 1.0), (0.6, 0.4), (0.5, 0.5), (-0.1, 0.9), (0.1, 1.5), ("a", 0.5), (None, 0.5),
                   (torch.tensor(0.1), 0.9), (float("nan"), 0.9)):
        with pytest.raises(ValueError, match="lo and hi"):
            loss.opacity_entropy(x, lo, hi)
    with pytest.raises(ValueError, match="lo and hi"):           # 1 - 1e-9 is 1.0 in float32: the clamp's upper bound
        loss.opacity_entropy(x, 1e-3, 1 - 1e-9)
    with pytest.raises(ValueError, match="opacity_raw must be a GPU tensor"):   # ... but a bound of the float64 clamp
        loss.opacity_entropy(x.double(), 1e-3, 1 - 1e-9)
    # device: everything else is right, the tensor is on the CPU -- no fallback, by design
    for ok in (x, x.double(), x.view(-1)):
        with pytest.raises(ValueError, match="opacity_raw must be a GPU tensor"):
            loss.opacity_entropy(ok)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_entry_points(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfgs.h"
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    assert L.ABI_VERSION >= 20 and lib.sfgs_abi_version() == L.ABI_VERSION
    assert "train.py:236-242" in hdr and "834-843" in hdr
    # the argument struct: the header's field order, size and offsets
    fields = [f for f, _ in L.SfgsOpacityEntropyArgs._fields_]
    assert fields == ["struct_size", "n", "opacity_raw", "is_f64", "lo", "hi", "with_grad"]
    body = re.search(r"typedef struct SfgsOpacityEntropyArgs \{(.*?)\} SfgsOpacityEntropyArgs;", hdr, re.S).group(1)
    declared = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert declared == fields
    src = tmp_path / "layout.c"
    prints = "\n".join(f'  printf("{f} %zu\\n", offsetof(SfgsOpacityEntropyArgs, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                   f'  printf("sizeof %zu\\n", sizeof(SfgsOpacityEntropyArgs));\n{prints}\n  return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SfgsOpacityEntropyArgs)
    for f in fields:
        assert int(out[f]) == getattr(L.SfgsOpacityEntropyArgs, f).offset, f


def test_kernel_ids_keep_every_older_position_up_to_the_loss_kernels():
    """Ids 0..26 are the parent's. The three new ids follow them, in front of the five loss kernels, which stay the last
    names of the list (tests/test_loss_host.py); ids are resolved by name (L.profile_select, L.profile_collect)."""
    lib = L.load()
    names = [lib.sfgs_profile_kernel_name(i).decode() for i in range(lib.sfgs_profile_kernel_count())]
    assert names[27:30] == ["opacity_entropy_fwd", "opacity_entropy_final", "opacity_entropy_bwd"]
    assert names[1] == "preprocess" and names.index("ssim_fwd") == 13 and names.index("densify") == 26
    assert names[-5:] == ["loss_photo_fwd", "loss_depth_fwd", "loss_final", "loss_photo_bwd", "loss_depth_bwd"]
    assert len(names) == 35 and len(set(names)) == 35            # sfgs_profile_select takes a 64-bit mask


def test_gpu_free_entry_points_validate_their_arguments():
    lib = L.load()
    dummy = C.c_double(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value

    def args(**kw):
        a = L.SfgsOpacityEntropyArgs(C.sizeof(L.SfgsOpacityEntropyArgs), 2_000_000, fp, 0, 1e-3, 1 - 1e-3, 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    full = lib.sfgs_opacity_entropy_scratch_bytes(C.byref(args()))
    assert 0 < full <= 64 * 1024                                  # per-block partial sums only: nothing N-sized
    # the partial count is a function of n (and the dtype) alone, and capped
    assert lib.sfgs_opacity_entropy_scratch_bytes(C.byref(args(n=64_000_000))) == \
        lib.sfgs_opacity_entropy_scratch_bytes(C.byref(args(n=8_000_000)))
    assert lib.sfgs_opacity_entropy_scratch_bytes(C.byref(args(n=1))) == 256
    assert lib.sfgs_opacity_entropy_scratch_bytes(None) == 0
    assert lib.sfgs_opacity_entropy_scratch_bytes(C.byref(args(struct_size=8))) == 0
    assert b"struct_size" in lib.sfgs_last_error()
    for bad in (dict(n=0), dict(n=-5), dict(opacity_raw=None), dict(lo=0.0), dict(hi=1.0), dict(lo=0.6, hi=0.4),
                dict(lo=0.5, hi=0.5), dict(lo=float("nan")), dict(hi=1 - 1e-9)):    # the last: 1.0 once rounded to float32
        assert lib.sfgs_opacity_entropy_scratch_bytes(C.byref(args(**bad))) == 0, bad
        # status codes before any HIP call: the pointers are never dereferenced
        assert lib.sfgs_opacity_entropy_forward(C.byref(args(**bad)), fp, fp, full, None) == -1, bad
        assert lib.sfgs_opacity_entropy_backward(C.byref(args(**bad)), fp, fp, None) == -1, bad
    assert b"lo < hi" in lib.sfgs_last_error()
    assert lib.sfgs_opacity_entropy_scratch_bytes(C.byref(args(hi=1 - 1e-9, is_f64=1))) > 0   # a bound in float64
    assert lib.sfgs_opacity_entropy_forward(C.byref(args()), None, fp, full, None) == -1
    assert lib.sfgs_opacity_entropy_forward(C.byref(args()), fp, None, full, None) == -1
    assert lib.sfgs_opacity_entropy_forward(C.byref(args()), fp, fp, full - 1, None) == -3     # SFGS_E_CAPACITY
    assert lib.sfgs_opacity_entropy_backward(C.byref(args()), None, fp, None) == -1
    assert lib.sfgs_opacity_entropy_backward(C.byref(args()), fp, None, None) == -1
    assert lib.sfgs_opacity_entropy_backward(C.byref(args(with_grad=0)), fp, fp, None) == -1
    assert b"with_grad" in lib.sfgs_last_error()


# ---- sfgs.opacity_reg: the handle, on CPU tensors -------------------------------------------------------------------------------
def make_model_class():
    class GaussianModel:                                          # scene/gaussian_model.py:234 and the members it needs
        def __init__(self, raw):
            self._opacity = torch.nn.Parameter(raw.clone())

        @property
        def get_opacity(self):
            return torch.sigmoid(self._opacity)
    return GaussianModel


def raw_values(n=257, dtype=torch.float32, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 1, generator=g, dtype=dtype) * 24.0 - 12.0)


@pytest.fixture
def patched(monkeypatch):
    """(GaussianModel with the hook installed and handles enabled for CPU tensors, the list of fused-entry calls)"""
    from sfgs import loss, opacity_reg
    calls = []

    def restatement(opacity_raw, lo=1e-3, hi=1 - 1e-3):
        calls.append((opacity_raw, lo, hi))
        o = torch.sigmoid(opacity_raw).clamp(lo, hi)
        return F.binary_cross_entropy(o, o)
    monkeypatch.setattr(loss, "opacity_entropy", restatement)
    monkeypatch.setattr(opacity_reg, "_HANDLE_DEVICES", {"cpu", "cuda"})
    cls = make_model_class()
    opacity_reg.install(cls)
    yield cls, calls
    opacity_reg.uninstall(cls)


def test_cpu_parameters_get_the_original_getter():
    from sfgs import opacity_reg
    cls = make_model_class()
    orig = cls.__dict__["get_opacity"]
    opacity_reg.install(cls)
    try:
        assert cls.__dict__["get_opacity"] is not orig
        m = cls(raw_values())
        before = opacity_reg.materialisations
        o = m.get_opacity
        assert type(o) is torch.Tensor and o.grad_fn is not None
        assert torch.equal(o, torch.sigmoid(m._opacity))
        assert opacity_reg.materialisations == before
        m._opacity = torch.nn.Parameter(torch.zeros(4, 1, dtype=torch.float16))     # and any other dtype / shape
        assert type(m.get_opacity) is torch.Tensor
    finally:
        opacity_reg.uninstall(cls)


def test_install_twice_is_a_noop_and_uninstall_restores_the_property_object():
    from sfgs import opacity_reg
    cls = make_model_class()
    orig = cls.__dict__["get_opacity"]
    opacity_reg.uninstall(cls)                                    # without an install: a no-op
    assert cls.__dict__["get_opacity"] is orig
    opacity_reg.install(cls)
    first = cls.__dict__["get_opacity"]
    opacity_reg.install(cls)
    assert cls.__dict__["get_opacity"] is first and first is not orig
    opacity_reg.uninstall(cls)
    assert cls.__dict__["get_opacity"] is orig
    opacity_reg.uninstall(cls)
    assert cls.__dict__["get_opacity"] is orig

    class NoGetter:                                               # the launcher tests' stand-in models have no get_opacity
        pass

    class Inherits(cls):                                          # ... and a property of a base class is not this class's own
        pass
    for other in (NoGetter, Inherits):
        before = dict(other.__dict__)
        opacity_reg.install(other)
        assert dict(other.__dict__) == before
        opacity_reg.uninstall(other)
        assert dict(other.__dict__) == before


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("spelling", ["method", "function", "keywords"])
def test_the_regularisers_statements_call_the_fused_entry_exactly_once(patched, dtype, spelling):
    from sfgs import opacity_reg
    cls, calls = patched
    gaussians, plain = cls(raw_values(dtype=dtype)), make_model_class()(raw_values(dtype=dtype))
    before = opacity_reg.materialisations
    h = gaussians.get_opacity
    assert type(h) is opacity_reg.OpacityHandle
    # metadata is answered without computing anything
    assert h.shape == (257, 1) and h.dtype == dtype and h.device.type == "cpu" and h.requires_grad and not h.is_leaf
    assert len(h) == 257 and h.dim() == 2 and h.numel() == 257 and h.size(0) == 257
    if spelling == "method":
        opacity = gaussians.get_opacity.clamp(1.0e-3, 1.0 - 1.0e-3)                     # train.py:239
    elif spelling == "function":
        opacity = torch.clamp(gaussians.get_opacity, 1.0e-3, 1.0 - 1.0e-3)
    else:
        opacity = gaussians.get_opacity.clamp(min=1.0e-3, max=1.0 - 1.0e-3)
    assert type(opacity) is opacity_reg.OpacityHandle and opacity.shape == (257, 1) and opacity.dtype == dtype
    opacity_loss = torch.nn.functional.binary_cross_entropy(opacity, opacity)              # train.py:240
    loss = torch.zeros((), dtype=dtype)
    loss += 10.0 * opacity_loss                                                            # train.py:242
    loss.backward()
    assert len(calls) == 1 and calls[0][0] is gaussians._opacity
    assert calls[0][1:] == (1.0e-3, 1.0 - 1.0e-3)
    assert opacity_reg.materialisations == before
    o = plain.get_opacity.clamp(1.0e-3, 1.0 - 1.0e-3)
    want = 10.0 * F.binary_cross_entropy(o, o)
    want.backward()
    assert torch.equal(loss.detach(), want.detach()) and torch.equal(gaussians._opacity.grad, plain._opacity.grad)
    with torch.no_grad():                                         # evaluation: no graph, still the fused entry
        opacity = gaussians.get_opacity.clamp(1.0e-3, 1.0 - 1.0e-3)
        assert not opacity.requires_grad and opacity.is_leaf
        value = F.binary_cross_entropy(opacity, opacity)
    assert len(calls) == 2 and not value.requires_grad and opacity_reg.materialisations == before


OTHER_USES = {
    "prune_mask": lambda o: (o < 0.005).squeeze(),                                           # gaussian_model.py:731
    "reset_opacity": lambda o: torch.min(o, torch.ones_like(o) * 0.01),                      # gaussian_model.py:485
    "histogram": lambda o: torch.histc(o.detach(), bins=16),                                 # train.py:1100
    "arithmetic": lambda o: (o * 2.0 + 1.0).sum(),
    "indexing": lambda o: o[3:40:2].sum(),
    "sum": lambda o: o.sum(),
    "numpy": lambda o: torch.from_numpy(o.detach().cpu().numpy().copy()),
    "clamp_one_bound": lambda o: F.binary_cross_entropy(o.clamp(min=1e-3), o.clamp(min=1e-3)),
    "clamp_tensor_bounds": lambda o: o.clamp(torch.tensor(1e-3), torch.tensor(0.999)).sum(),
    "clamp_bounds_outside_0_1": lambda o: F.binary_cross_entropy(o.clamp(0.0, 1.0), o.clamp(0.0, 1.0).detach()),
    "two_clamps": lambda o: F.binary_cross_entropy(o.clamp(1e-3, 0.999), o.clamp(1e-3, 0.999)),
    "clamp_of_a_clamp": lambda o: (lambda c: F.binary_cross_entropy(c, c))(o.clamp(1e-3, 0.999).clamp(0.01, 0.99)),
    "unclamped_bce": lambda o: F.binary_cross_entropy(o, o),
    "other_target": lambda o: (lambda c: F.binary_cross_entropy(c, torch.full_like(c, 0.5)))(o.clamp(1e-3, 0.999)),
    "detached_target": lambda o: (lambda c: F.binary_cross_entropy(c, c.detach()))(o.clamp(1e-3, 0.999)),
    "reduction_sum": lambda o: (lambda c: F.binary_cross_entropy(c, c, reduction="sum"))(o.clamp(1e-3, 0.999)),
    "reduction_none": lambda o: (lambda c: F.binary_cross_entropy(c, c, reduction="none").sum())(o.clamp(1e-3, 0.999)),
    "weight": lambda o: (lambda c: F.binary_cross_entropy(c, c, weight=torch.full_like(c, 2.0)))(o.clamp(1e-3, 0.999)),
    "clamped_then_arithmetic": lambda o: (o.clamp(1e-3, 0.999) ** 2).mean(),
    "bce_then_more": lambda o: (lambda c: F.binary_cross_entropy(c, c, reduction="sum") + c.sum())(o.clamp(1e-3, 0.999)),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("use", sorted(OTHER_USES))
def test_every_other_use_is_bit_identical_to_the_unpatched_getter(patched, use, dtype):
    from sfgs import opacity_reg
    cls, calls = patched
    fn = OTHER_USES[use]
    gaussians, plain = cls(raw_values(dtype=dtype)), make_model_class()(raw_values(dtype=dtype))
    before = opacity_reg.materialisations
    got, want = fn(gaussians.get_opacity), fn(plain.get_opacity)
    assert not calls, "the fused entry ran for a use that is not the regulariser's"
    assert opacity_reg.materialisations > before
    assert type(got) is torch.Tensor and got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got, want)
    assert got.requires_grad == want.requires_grad
    if want.requires_grad:
        got.sum().backward()
        want.sum().backward()
        assert torch.equal(gaussians._opacity.grad, plain._opacity.grad)


def test_other_attributes_are_read_from_the_tensor_the_handle_stands_for(patched):
    cls, _ = patched
    gaussians = cls(raw_values())
    h = gaussians.get_opacity
    assert h._version == 0 and type(h.grad_fn).__name__ == "SigmoidBackward0"
    assert torch.equal(h.data, torch.sigmoid(gaussians._opacity).data)
    assert torch.equal(h.T, torch.sigmoid(gaussians._opacity).T)


def test_a_handle_kept_across_an_in_place_update_raises(patched):
    cls, calls = patched
    gaussians = cls(raw_values())
    kept, kept_clamped = gaussians.get_opacity, gaussians.get_opacity.clamp(1e-3, 0.999)
    used_before = gaussians.get_opacity
    value_before = used_before.sum().item()                       # looked at before the update: keeps its values, like a tensor
    with torch.no_grad():
        gaussians._opacity.add_(1.0)                              # what optimizer.step() does
    with pytest.raises(RuntimeError, match="modified in place"):
        kept.sum()
    with pytest.raises(RuntimeError, match="modified in place"):
        F.binary_cross_entropy(kept_clamped, kept_clamped)
    with pytest.raises(RuntimeError, match="modified in place"):
        kept_clamped.sum()
    assert not calls
    assert used_before.sum().item() == value_before
    fresh = gaussians.get_opacity                                 # a new read stands for the new values
    assert torch.equal(fresh.sum(), torch.sigmoid(gaussians._opacity).sum())
    # the parameter object replaced on the model (densification, reset_opacity): stale as well
    kept = gaussians.get_opacity
    gaussians._opacity = torch.nn.Parameter(gaussians._opacity.detach().clone())
    with pytest.raises(RuntimeError, match="replaced"):
        kept.sum()


def test_the_launcher_installs_the_hook():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import launch_scenes
    from sfgs import opacity_reg
    src = open(launch_scenes.__file__).read()
    assert "opacity_reg" in src
    assert hasattr(opacity_reg, "install") and hasattr(opacity_reg, "uninstall")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "scene")), reason="reference tree not present (GPU box)")
def test_the_committed_golden_file_is_reproduced_by_the_reference(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_opacity_reg.py"), "--check"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "reproduced exactly" in r.stdout
