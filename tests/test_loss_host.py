"""sfgs.loss without a GPU: the module imports, its argument checks run before the library is loaded, install() /
uninstall() rebind exactly two names, and the C header, the library and the ctypes binding agree on the three entry
points. The kernels themselves: tests/test_gpu_loss.py."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from sfgs import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_module_imports_without_a_gpu():
    from sfgs import loss
    for name in ("training_loss", "photometric", "depth_pearson", "l1_loss", "pearson_corrcoef", "install", "uninstall"):
        assert callable(getattr(loss, name)), name


def test_argument_checks_name_the_argument():
    from sfgs import loss
    img = torch.zeros(3, 8, 9)
    dep = torch.zeros(1, 8, 9)
    # dtype
    with pytest.raises(ValueError, match="image"):
        loss.training_loss(img.double(), dep, img, dep, None, 0.2, 0.5)
    with pytest.raises(ValueError, match="gt_image"):
        loss.photometric(img, img.half())
    with pytest.raises(ValueError, match="gt_depth"):
        loss.depth_pearson(dep, dep.double())
    with pytest.raises(ValueError, match="mask"):
        loss.photometric(img, img, mask=torch.ones(1, 8, 9, dtype=torch.bool))
    # shape
    with pytest.raises(ValueError, match="image"):
        loss.photometric(img[None], img[None])
    with pytest.raises(ValueError, match="gt_image"):
        loss.photometric(img, torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="depth"):
        loss.training_loss(img, torch.zeros(1, 9, 8), img, torch.zeros(1, 9, 8), None, 0.2, 0.5)
    with pytest.raises(ValueError, match="mask"):
        loss.training_loss(img, dep, img, dep, torch.ones(3, 8, 9), 0.2, 0.5)
    with pytest.raises(ValueError, match="mask"):
        loss.depth_pearson(dep, dep, mask=torch.ones(8, 9))
    with pytest.raises(ValueError, match="preds"):
        loss.pearson_corrcoef(torch.zeros(10, 2), torch.zeros(10, 2))
    with pytest.raises(ValueError, match="target"):
        loss.pearson_corrcoef(torch.zeros(10), torch.zeros(11))
    with pytest.raises(ValueError, match="gt"):
        loss.l1_loss(torch.zeros(4, 4), torch.zeros(4, 5))
    # mode / missing halves
    with pytest.raises(ValueError, match="invalid"):
        loss.training_loss(img, dep, img, dep, None, 0.2, 0.5, invalid="nan_to_num")
    with pytest.raises(ValueError, match="lambda_depth"):
        loss.training_loss(img, None, img, None, None, 0.2, 0.5)
    with pytest.raises(ValueError, match="both"):
        loss.training_loss(img, dep, img, None, None, 0.2, 0.0)
    # device: everything else is right, the tensors are on the CPU -- no fallback, by design
    with pytest.raises(ValueError, match="image must be a GPU tensor"):
        loss.training_loss(img, dep, img, dep, torch.ones(1, 1, 1), 0.2, 0.5)
    with pytest.raises(ValueError, match="depth must be a GPU tensor"):
        loss.depth_pearson(dep, dep)
    with pytest.raises(ValueError, match="network_output must be a GPU tensor"):
        loss.l1_loss(img, img)
    with pytest.raises(ValueError, match="preds must be a GPU tensor"):
        loss.pearson_corrcoef(torch.zeros(10, 1), torch.zeros(10, 1))


def test_install_rebinds_exactly_two_names_and_uninstall_restores_them():
    from sfgs import loss
    train = types.ModuleType("train")
    orig_l1, orig_pc, other = (lambda a, b: "l1"), (lambda a, b: "pearson"), (lambda a, b: "ssim")
    train.l1_loss, train.pearson_corrcoef, train.fused_ssim = orig_l1, orig_pc, other
    train.depth_loss_func = types.FunctionType(
        compile("def depth_loss_func(gt_depth, depth):\n    return pearson_corrcoef(gt_depth, depth)\n", "train.py", "exec").co_consts[0],
        train.__dict__)
    before = dict(train.__dict__)
    loss.uninstall(train)                         # without an install: a no-op
    assert dict(train.__dict__) == before
    loss.install(train)
    changed = {k for k in before if train.__dict__[k] is not before[k]}
    assert changed == {"l1_loss", "pearson_corrcoef"} and set(train.__dict__) == set(before)
    assert train.l1_loss is loss.l1_loss and train.pearson_corrcoef is loss.pearson_corrcoef
    with pytest.raises(ValueError, match="preds must be a GPU tensor"):   # depth_loss_func now reaches the HIP operator
        train.depth_loss_func(torch.zeros(4, 1), torch.zeros(4, 1))
    train.fused_ssim = other
    loss.install(train)                           # a second install: a no-op (the originals are not overwritten)
    loss.uninstall(train)
    assert dict(train.__dict__) == before
    assert train.depth_loss_func(None, None) == "pearson"
    loss.uninstall(train)
    assert dict(train.__dict__) == before


def test_header_library_and_binding_agree_on_the_loss_entry_points(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    for name in ("sfgs_loss_scratch_bytes", "sfgs_loss_forward", "sfgs_loss_backward"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfgs.h"
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    assert L.ABI_VERSION >= 19 and lib.sfgs_abi_version() == L.ABI_VERSION
    # the argument struct: same size and field offsets as the C compiler's
    fields = [f for f, _ in L.SfgsLossArgs._fields_]
    src = tmp_path / "layout.c"
    body = "\n".join(f'  printf("{f} %zu\\n", offsetof(SfgsLossArgs, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                   f'  printf("sizeof %zu\\n", sizeof(SfgsLossArgs));\n{body}\n  return 0;\n}}\n')
    import subprocess
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SfgsLossArgs)
    for f in fields:
        assert int(out[f]) == getattr(L.SfgsLossArgs, f).offset, f
    # the header's constants are the binding's
    for cname, val in (("PHOTOMETRIC", L.LOSS_PHOTOMETRIC), ("DEPTH", L.LOSS_DEPTH), ("L1_STREAM", L.LOSS_L1_STREAM),
                       ("INVALID_ZERO", L.LOSS_INVALID_ZERO), ("INVALID_DROP", L.LOSS_INVALID_DROP),
                       ("INVALID_KEEP", L.LOSS_INVALID_KEEP)):
        assert int(re.search(r"#define\s+SFGS_LOSS_" + cname + r"\s+(\d+)", hdr).group(1)) == val, cname


def test_gpu_free_entry_points_validate_their_arguments():
    lib = L.load()
    dummy = C.c_float(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value

    def args(**kw):
        a = L.SfgsLossArgs(C.sizeof(L.SfgsLossArgs), 3, 1080, 1920, fp, fp, fp, fp, None, 0, 0.2, 0.5, L.LOSS_INVALID_ZERO,
                           L.LOSS_PHOTOMETRIC | L.LOSS_DEPTH, 1, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    full = lib.sfgs_loss_scratch_bytes(C.byref(args()))
    assert full > 3 * 3 * 1080 * 1920 * 4                      # the three derivative maps
    assert lib.sfgs_loss_scratch_bytes(C.byref(args(with_grad=0))) < 1 << 20   # only partial sums without them
    assert lib.sfgs_loss_scratch_bytes(C.byref(args(struct_size=8))) == 0 and b"struct_size" in lib.sfgs_last_error()
    assert lib.sfgs_loss_scratch_bytes(None) == 0
    # status codes before any HIP call: the pointers are never dereferenced
    assert lib.sfgs_loss_forward(C.byref(args(terms=0)), fp, fp, full, None) == -1
    assert lib.sfgs_loss_forward(C.byref(args(mask_elems=7, mask=fp)), fp, fp, full, None) == -1
    assert b"mask_elems" in lib.sfgs_last_error()
    assert lib.sfgs_loss_forward(C.byref(args(mask_elems=1)), fp, fp, full, None) == -1       # mask NULL, mask_elems 1
    assert lib.sfgs_loss_forward(C.byref(args(depth=None)), fp, fp, full, None) == -1
    assert lib.sfgs_loss_forward(C.byref(args(invalid_mode=3)), fp, fp, full, None) == -1
    assert lib.sfgs_loss_forward(C.byref(args()), None, fp, full, None) == -1
    assert lib.sfgs_loss_forward(C.byref(args()), fp, fp, full - 1, None) == -3              # SFGS_E_CAPACITY
    assert lib.sfgs_loss_forward(C.byref(args(H=32768, W=32768)), fp, fp, C.c_size_t(1 << 62), None) == -4
    assert b"2^30" in lib.sfgs_last_error()
    assert lib.sfgs_loss_backward(C.byref(args(terms=L.LOSS_DEPTH)), fp, fp, fp, None, None, None) == -1   # g_image without the term
    names = [lib.sfgs_profile_kernel_name(i).decode() for i in range(lib.sfgs_profile_kernel_count())]
    assert names[-5:] == ["loss_photo_fwd", "loss_depth_fwd", "loss_final", "loss_photo_bwd", "loss_depth_bwd"]
    assert names[1] == "preprocess" and names.index("ssim_fwd") == 13                           # appended: the old ids stay
