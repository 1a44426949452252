"""sfgs.resample without a GPU: the module imports, its argument checks (and those of the loss's subpixel_offset keyword)
run before the library is loaded, install() / uninstall() rebind exactly one name, the C header, the library and the ctypes
binding agree on ABI 23 and on SfgsResampleArgs, the entry point validates its arguments before any HIP call, and the float64
oracle (tests/resample_np.py) agrees with the reference's own output (tests/golden/make_golden_resample.py). The kernel
itself: tests/test_gpu_resample.py."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from resample_np import resample64
from sfgs import _lib as L
from sfgs import resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_resample.npz")


def test_module_imports_without_a_gpu():
    for name in ("resample_gt", "create_offset_gt", "install", "uninstall"):
        assert callable(getattr(resample, name)), name
    assert sorted(resample.__all__) == ["create_offset_gt", "install", "resample_gt", "uninstall"]


def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load", no_load)
    img, off = torch.zeros(3, 8, 9), torch.zeros(8, 9, 2)
    # not tensors, dtype
    with pytest.raises(ValueError, match="image must be a tensor"):
        resample.resample_gt(np.zeros((3, 8, 9), np.float32), off)
    with pytest.raises(ValueError, match="image must be float32"):
        resample.resample_gt(img.double(), off)
    with pytest.raises(ValueError, match="subpixel_offset must be float32"):
        resample.resample_gt(img, off.half())
    with pytest.raises(ValueError, match="mask must be float32"):
        resample.resample_gt(img, off, torch.ones(1, 8, 9, dtype=torch.bool))
    # shape
    with pytest.raises(ValueError, match="image must be"):
        resample.resample_gt(img[None], off)
    with pytest.raises(ValueError, match="image must be"):
        resample.resample_gt(torch.zeros(5, 8, 9), off)                       # C > 4
    with pytest.raises(ValueError, match="image must be"):
        resample.resample_gt(torch.zeros(3, 1, 9), torch.zeros(1, 9, 2))      # H < 2
    with pytest.raises(ValueError, match="image must be"):
        resample.resample_gt(torch.zeros(3, 8, 1), torch.zeros(8, 1, 2))      # W < 2
    with pytest.raises(ValueError, match="subpixel_offset must be"):
        resample.resample_gt(img, torch.zeros(9, 8, 2))
    with pytest.raises(ValueError, match="subpixel_offset must be"):
        resample.resample_gt(img, torch.zeros(2, 8, 9))
    with pytest.raises(ValueError, match="mask must be"):
        resample.resample_gt(img, off, torch.ones(3, 8, 9))
    with pytest.raises(ValueError, match="mask must be"):
        resample.resample_gt(img, off, torch.ones(8, 9))
    # device: everything else is right, the tensors are on the CPU -- no fallback, by design
    with pytest.raises(ValueError, match="image must be a GPU tensor"):
        resample.resample_gt(img, off, torch.ones(1, 1, 1))
    with pytest.raises(ValueError, match="image must be a GPU tensor"):
        resample.create_offset_gt(img, off)
    # the loss's keyword: the same checks, the same place
    from sfgs import loss
    dep = torch.zeros(1, 8, 9)
    with pytest.raises(ValueError, match="subpixel_offset must be"):
        loss.training_loss(img, dep, img, dep, None, 0.2, 0.5, subpixel_offset=torch.zeros(8, 9))
    with pytest.raises(ValueError, match="subpixel_offset must be float32"):
        loss.photometric(img, img, subpixel_offset=off.double())
    with pytest.raises(ValueError, match="gt_image must be"):
        loss.photometric(torch.zeros(5, 8, 9), torch.zeros(5, 8, 9), subpixel_offset=off)   # C > 4 only with the keyword
    with pytest.raises(ValueError, match="image must be a GPU tensor"):
        loss.training_loss(img, dep, img, dep, None, 0.2, 0.5, subpixel_offset=off)
    with pytest.raises(ValueError, match="image must be a GPU tensor"):
        loss.photometric(img, img, None, off)


def test_install_rebinds_exactly_one_name_and_uninstall_restores_it():
    train = types.ModuleType("train")
    orig, other = (lambda image, offset: "reference"), (lambda a, b: "l1")
    train.create_offset_gt, train.l1_loss = orig, other
    exec("def step(gt_image, subpixel_offset):\n    return create_offset_gt(gt_image, subpixel_offset)\n", train.__dict__)   # train.py:215
    before = dict(train.__dict__)
    resample.uninstall(train)                     # without an install: a no-op
    assert dict(train.__dict__) == before
    resample.install(train)
    changed = {k for k in before if train.__dict__[k] is not before[k]}
    assert changed == {"create_offset_gt"} and set(train.__dict__) == set(before)
    assert train.create_offset_gt is resample.create_offset_gt
    with pytest.raises(ValueError, match="image must be a GPU tensor"):   # the call site now reaches the HIP operator
        train.step(torch.zeros(3, 4, 5), torch.zeros(4, 5, 2))
    resample.install(train)                       # a second install: a no-op (the original is not overwritten)
    resample.uninstall(train)
    assert dict(train.__dict__) == before and train.step(None, None) == "reference"
    resample.uninstall(train)
    assert dict(train.__dict__) == before


def test_header_library_and_binding_agree_on_abi_23(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    m = re.search(r"\bsfgs_resample_gt\s*\(([^;]*)\)\s*;", hdr)
    assert m, "sfgs_resample_gt is not declared in include/sfgs.h"
    assert len(m.group(1).split(",")) == len(L.SYMBOLS["sfgs_resample_gt"][1])
    assert lib.sfgs_resample_gt is not None
    declared_version = int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1))
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() and L.ABI_VERSION >= 23
    assert int(re.search(r"#define\s+SFGS_LOSS_GT_PREMASKED\s+(\d+)", hdr).group(1)) == L.LOSS_GT_PREMASKED == 8
    # the argument struct: same size and field offsets as the C compiler's
    fields = [f for f, _ in L.SfgsResampleArgs._fields_]
    src = tmp_path / "layout.c"
    body = "\n".join(f'  printf("{f} %zu\\n", offsetof(SfgsResampleArgs, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                   f'  printf("sizeof %zu\\n", sizeof(SfgsResampleArgs));\n{body}\n  return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SfgsResampleArgs)
    for f in fields:
        assert int(out[f]) == getattr(L.SfgsResampleArgs, f).offset, f


def test_entry_point_validates_its_arguments_before_any_hip_call():
    lib = L.load()
    dummy = (C.c_float * 4)()
    fp = C.cast(dummy, C.c_void_p).value
    far = fp + (1 << 40)                          # never dereferenced: every call below fails its checks first

    def args(**kw):
        a = L.SfgsResampleArgs(C.sizeof(L.SfgsResampleArgs), 3, 1080, 1920, fp, None, 0, fp)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    call = lambda a, out=far: lib.sfgs_resample_gt(C.byref(a) if a is not None else None, out, None)
    assert call(None) == -1
    assert call(args(struct_size=8)) == -1 and b"struct_size" in lib.sfgs_last_error()
    assert call(args(C=0)) == -1 and call(args(C=5)) == -1 and b"1 ... 4" in lib.sfgs_last_error()
    assert call(args(H=1)) == -1 and b"at least 2" in lib.sfgs_last_error()
    assert call(args(W=1)) == -1
    assert call(args(C=4, H=32768, W=16384)) == -4 and b"2^31" in lib.sfgs_last_error()   # C * H * W = 2^31 exactly
    assert call(args(mask_elems=7, mask=fp)) == -1 and b"mask_elems" in lib.sfgs_last_error()
    assert call(args(mask_elems=1)) == -1                                                   # mask NULL, mask_elems 1
    assert call(args(mask=fp)) == -1                                                        # mask set, mask_elems 0
    assert call(args(src=None)) == -1 and call(args(offset=None)) == -1 and call(args(), None) == -1
    assert call(args(), fp + 4) == -1 and b"overlaps" in lib.sfgs_last_error()
    # the loss: the new bit needs the photometric term and is known to the plan
    la = L.SfgsLossArgs(C.sizeof(L.SfgsLossArgs), 3, 64, 64, fp, fp, fp, fp, None, 0, 0.2, 0.5, L.LOSS_INVALID_ZERO,
                        L.LOSS_PHOTOMETRIC | L.LOSS_GT_PREMASKED, 0, 0)
    assert lib.sfgs_loss_scratch_bytes(C.byref(la)) > 0
    la.terms = L.LOSS_DEPTH | L.LOSS_GT_PREMASKED
    assert lib.sfgs_loss_scratch_bytes(C.byref(la)) == 0 and b"GT_PREMASKED" in lib.sfgs_last_error()
    la.terms = L.LOSS_GT_PREMASKED
    assert lib.sfgs_loss_scratch_bytes(C.byref(la)) == 0


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_oracle_agrees_with_the_reference_golden(tag):
    G = np.load(GOLDEN)
    mask = G[f"{tag}_mask"] if f"{tag}_mask" in G.files else None
    want = G[f"{tag}_out"]
    got = resample64(G[f"{tag}_image"], G[f"{tag}_offset"], mask)
    err = np.abs(got - want).max()
    print(f"golden {tag} {want.shape}: max |reference - oracle64| {err:.3e}")
    assert got.shape == want.shape and got.dtype == np.float64
    assert err <= 1e-5
    if tag == "b":      # all four borders clamp
        off = G["b_offset"]
        H, W = off.shape[:2]
        xx, yy = np.meshgrid(np.arange(W), np.arange(H))
        u, v = xx + off[..., 0], yy + off[..., 1]
        assert (u < 0).any() and (u > W - 1).any() and (v < 0).any() and (v > H - 1).any()


def test_oracle_edge_semantics():
    """Integer offsets shift, offsets far outside clamp to the border, non-finite offsets: NaN, -inf -> 0, +inf -> last."""
    g = np.random.default_rng(5)
    src = g.random((2, 6, 7), dtype=np.float32)
    H, W = 6, 7
    off = np.zeros((H, W, 2), np.float32)
    np.testing.assert_array_equal(resample64(src, off), src.astype(np.float64))
    off[..., 0] = 1.0
    want = np.concatenate([src[:, :, 1:], src[:, :, -1:]], axis=2)
    np.testing.assert_array_equal(resample64(src, off), want.astype(np.float64))
    off[..., 0], off[..., 1] = -1e4, 1e4
    np.testing.assert_array_equal(resample64(src, off), np.broadcast_to(src[:, -1:, :1], src.shape).astype(np.float64))
    off[..., 0], off[..., 1] = np.nan, np.inf
    np.testing.assert_array_equal(resample64(src, off), np.broadcast_to(src[:, -1:, :1], src.shape).astype(np.float64))
    off[..., 0], off[..., 1] = np.inf, -np.inf
    np.testing.assert_array_equal(resample64(src, off), np.broadcast_to(src[:, :1, -1:], src.shape).astype(np.float64))
    m = np.zeros((1, H, W), np.float32)
    m[0, 2, 3] = 1.0
    off[...] = 0.5                                      # the mask is applied to the TAPS: the kept pixel bleeds into four
    out = resample64(src, off, m)
    assert np.count_nonzero(out[0]) == 4 and out[0, 1, 2] == 0.25 * float(src[0, 2, 3])
