"""sfgs.metrics without a GPU: the float64 restatement of the block (tests/metrics_np.py, what the kernels are held to) agrees
with every golden case -- the reference's own float32 functions driven by training_report's statements -- to the precision
float32 leaves; the argument checks run before the library is loaded; install / uninstall rebind one name; the C header, the
library and the ctypes binding agree; the scratch-size entry point rejects bad arguments. The kernels themselves:
tests/test_gpu_metrics.py."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import metrics_np as mnp
from sfgs import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_metrics.npz")
ENTRY_POINTS = ("sfgs_metrics_scratch_bytes", "sfgs_metrics_view")
CASES = ("clamp", "tile", "gray", "same", "nan")
VIEWS = ("view0", "view1", "view2")
# what the reference's float32 statements can differ from float64 by: a float32 mean carries the rounding of its sum and of
# the division plus the growth of a pairwise sum (4 roundings allowed); a PSNR near 20 dB is a float32 with a spacing of
# 1.9e-6 dB, its mean over three planes is rounded again and the mse under it carries the mean's relative error (0.9e-6 dB)
REL_MEAN = 4 * 2.0 ** -24
ABS_PSNR = 4e-6
ABS_SSIM = 2e-6        # tests/test_gpu_ops.py applies the same to fused_ssim


def test_golden_covers_the_cases_it_promises():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert g["clamp_image"].shape == (3, 45, 65) and g["tile_image"].shape == (3, 22, 32) and g["gray_image"].shape == (1, 23, 33)
    for name in ("clamp_image", "clamp_gt_image"):                       # the clamp matters on both operands
        assert g[name].min() < -0.1 and g[name].max() > 1.1
    assert np.array_equal(g["same_image"], g["same_gt_image"]) and np.isposinf(g["same_psnr"]) and g["same_l1"] == 0.0
    nan_at = np.argwhere(np.isnan(g["nan_image"]))
    assert len(nan_at) == 1 and nan_at[0][0] == 1 and not np.isnan(g["nan_gt_image"]).any()
    assert np.isnan(g["nan_l1"]) and np.isnan(g["nan_psnr"]) and np.isnan(g["nan_psnr_c"][1])
    assert np.isfinite(g["nan_psnr_c"][[0, 2]]).all()
    assert len({g[f"{v}_image"].shape for v in VIEWS}) == 3              # three views of different sizes
    assert np.isfinite(g["views_l1_test"]) and np.isfinite(g["views_psnr_test"])


@pytest.mark.parametrize("tag", CASES + VIEWS)
def test_oracle64_agrees_with_the_golden_case(tag):
    g = np.load(GOLDEN)
    row = mnp.view_metrics(g[f"{tag}_image"], g[f"{tag}_gt_image"])
    P = g[f"{tag}_image"].shape[0]
    mse_c = mnp.plane_mse(g[f"{tag}_image"], g[f"{tag}_gt_image"], clamp=True)
    print(tag, dict(zip(mnp.ROW, row)))
    if tag in ("same", "nan"):     # +inf and NaN: the same entries, exactly
        assert np.array_equal(row[[0, 1]], [g[f"{tag}_l1"], g[f"{tag}_psnr"]], equal_nan=True)
        assert np.array_equal(np.isnan(row[4:4 + P]), np.isnan(g[f"{tag}_psnr_c"]))
        assert np.array_equal(np.isposinf(row[4:4 + P]), np.isposinf(g[f"{tag}_psnr_c"]))
        assert np.array_equal(np.isnan(row[2]), np.isnan(g[f"{tag}_ssim"]))
        fin = np.isfinite(g[f"{tag}_psnr_c"])
        assert np.abs(row[4:4 + P][fin] - g[f"{tag}_psnr_c"][fin]).max(initial=0.0) <= ABS_PSNR
        if tag == "same":
            assert row[2] == 1.0 and g["same_ssim"] == 1.0 and row[3] == 0.0
        return
    assert abs(row[0] - g[f"{tag}_l1"]) <= REL_MEAN * row[0]
    assert abs(row[1] - g[f"{tag}_psnr"]) <= ABS_PSNR
    assert np.abs(row[4:4 + P] - g[f"{tag}_psnr_c"]).max() <= ABS_PSNR
    assert np.abs(mse_c - g[f"{tag}_mse_c"]).max() <= REL_MEAN * mse_c.max()
    assert abs(row[3] - mse_c.mean()) <= 1e-15
    assert abs(row[2] - g[f"{tag}_ssim"]) <= ABS_SSIM
    assert np.isnan(row[4 + P:]).all()
    assert np.isnan(mnp.view_metrics(g[f"{tag}_image"], g[f"{tag}_gt_image"], ssim=False)[2])


def test_oracle64_reproduces_the_two_means_training_report_prints():
    g = np.load(GOLDEN)
    rows = np.stack([mnp.view_metrics(g[f"{v}_image"], g[f"{v}_gt_image"]) for v in VIEWS])
    s = mnp.summarise(rows)
    assert s["n"] == 3
    assert abs(s["l1"] - g["views_l1_test"]) <= REL_MEAN * s["l1"]
    assert abs(s["psnr"] - g["views_psnr_test"]) <= ABS_PSNR
    assert s["psnr_std"] == pytest.approx(np.std(rows[:, 1]), abs=0, rel=1e-15) and s["psnr_std"] > 0   # population std


def test_the_clamp_keeps_nan():
    x = np.array([-1.0, 0.25, 2.0, np.nan, np.inf, -np.inf])
    assert np.array_equal(mnp.clamp01(x), torch.clamp(torch.tensor(x), 0.0, 1.0).numpy(), equal_nan=True)


# ---- sfgs.metrics: validation and the hook ---------------------------------------------------------------------------------------
def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    from sfgs import metrics
    assert set(metrics.__all__) >= {"view_metrics", "Evaluator", "psnr", "mse", "install", "uninstall"}

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load", no_library)
    x = torch.zeros(3, 6, 8)
    ev = metrics.Evaluator(2)
    for call in (metrics.view_metrics, ev.add):
        with pytest.raises(ValueError, match="image must be a tensor"):
            call(np.zeros((3, 6, 8), np.float32), x)
        for bad in (x.double(), x.half(), x.long()):
            with pytest.raises(ValueError, match="image must be float32"):
                call(bad, x)
        for bad in (torch.zeros(6, 8), torch.zeros(1, 3, 6, 8), torch.zeros(3, 0, 8), torch.zeros(5, 6, 8)):
            with pytest.raises(ValueError, match=r"image must be \[C,H,W\] with 1 <= C <= 4"):
                call(bad, bad)
        with pytest.raises(ValueError, match="gt_image must be a tensor"):
            call(x, None)
        with pytest.raises(ValueError, match="gt_image must be float32"):
            call(x, x.double())
        for bad in (torch.zeros(3, 6, 9), torch.zeros(1, 6, 8), torch.zeros(3, 48)):
            with pytest.raises(ValueError, match=r"gt_image must be \(3, 6, 8\) like image"):
                call(x, bad)
        # device: everything else is right, the tensors are on the CPU -- no fallback, by design
        with pytest.raises(ValueError, match="image must be a GPU tensor"):
            call(x, x)
    assert ev.n == 0
    for bad in (np.zeros(8), torch.zeros(8), torch.zeros(9, dtype=torch.float64), torch.zeros(2, 8, dtype=torch.float64)[:, 0]):
        with pytest.raises(ValueError, match="out must be"):
            metrics.view_metrics(x, x, out=bad)
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="capacity must be a positive integer"):
            metrics.Evaluator(bad)
    with pytest.raises(ValueError, match="device must be a GPU"):
        metrics.Evaluator(2, device="cpu")
    for fn in (metrics.psnr, metrics.mse):
        with pytest.raises(ValueError, match="img1 must be a tensor"):
            fn(None, x)
        with pytest.raises(ValueError, match="img1 must be float32"):
            fn(x.double(), x.double())
        with pytest.raises(ValueError, match="img1 must be a non-empty tensor"):
            fn(torch.zeros(()), torch.zeros(()))
        with pytest.raises(ValueError, match=r"img2 must be \(3, 6, 8\) like img1"):
            fn(x, torch.zeros(3, 8, 6))
        with pytest.raises(ValueError, match="at most 4 planes"):
            fn(torch.zeros(5, 6, 8), torch.zeros(5, 6, 8))
        with pytest.raises(ValueError, match="img1 must be a GPU tensor"):
            fn(x, x)
        with pytest.raises(ValueError, match="img1 must be a GPU tensor"):
            fn(torch.zeros(1, 3, 6, 8), torch.zeros(1, 3, 6, 8))          # the reference's batched form: planes = shape[0]


def test_an_empty_evaluator_reports_nothing_without_a_device():
    from sfgs import metrics
    ev = metrics.Evaluator(4)
    r = ev.result()
    assert r["n"] == 0 and r["per_view"].shape == (0, 8) and np.isnan(r["psnr"]) and np.isnan(r["l1_std"])
    ev.reset()
    assert ev.n == 0 and ev.capacity == 4


def test_install_and_uninstall_rebind_one_name():
    from sfgs import metrics

    def original(img1, img2):
        return "original"

    def other(img1, img2):
        return "other"
    mod = types.ModuleType("train_stand_in")
    mod.psnr, mod.l1_loss, mod.training_report, mod.torch = original, other, other, torch
    before = dict(vars(mod))
    metrics.install(mod)
    assert mod.psnr is metrics.psnr
    changed = {k for k in vars(mod) if vars(mod)[k] is not before.get(k)}
    assert changed == {"psnr"}
    hooked = mod.psnr
    metrics.install(mod)                                      # a second install is a no-op ...
    assert mod.psnr is hooked
    metrics.uninstall(mod)                                    # ... and one uninstall restores the original
    assert mod.psnr is original and dict(vars(mod)) == before
    metrics.uninstall(mod)
    assert mod.psnr is original
    # the reference's signatures (utils/image_utils.py)
    assert str(inspect.signature(metrics.psnr)) == str(inspect.signature(original)) == str(inspect.signature(metrics.mse))
    with pytest.raises(AttributeError):
        metrics.install(types.ModuleType("no_such_function_here"))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfgs.h"
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    declared_version = int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1))
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() and L.ABI_VERSION >= 25
    for cite in ("train.py:1064,1075,1090-1091", "utils/image_utils.py:14-19", "utils/loss_utils.py:17-18,33-63"):
        assert cite in hdr, cite
    assert re.search(r"#define SFGS_METRICS_CLAMP 1\b", hdr) and re.search(r"#define SFGS_METRICS_SSIM 2\b", hdr)
    assert (L.METRICS_CLAMP, L.METRICS_SSIM) == (1, 2)
    fields = [f for f, _ in L.SfgsMetricsArgs._fields_]
    assert fields == ["struct_size", "P", "H", "W", "a", "b", "flags", "reserved"]
    body = re.search(r"typedef struct SfgsMetricsArgs \{(.*?)\} SfgsMetricsArgs;", hdr, re.S).group(1)
    declared = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert declared == fields
    src = tmp_path / "layout.c"
    prints = "\n".join(f'  printf("{f} %zu\\n", offsetof(SfgsMetricsArgs, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                   f'  printf("sizeof %zu\\n", sizeof(SfgsMetricsArgs));\n{prints}\n  return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SfgsMetricsArgs)
    for f in fields:
        assert int(out[f]) == getattr(L.SfgsMetricsArgs, f).offset, f


def test_the_metrics_kernels_have_no_profiler_id():
    lib = L.load()
    names = [lib.sfgs_profile_kernel_name(i).decode() for i in range(lib.sfgs_profile_kernel_count())]
    assert not any("metrics" in n for n in names) and names[-1] == "loss_depth_bwd"


def test_gpu_free_entry_points_validate_their_arguments():
    lib = L.load()
    dummy = C.c_double(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value

    def args(**kw):
        a = L.SfgsMetricsArgs(C.sizeof(L.SfgsMetricsArgs), 3, 1080, 1920, fp, fp, L.METRICS_CLAMP | L.METRICS_SSIM, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    tiles = 3 * ((1920 + 31) // 32) * ((1080 + 21) // 22)
    up = lambda v: (v + 255) // 256 * 256
    full = lib.sfgs_metrics_scratch_bytes(C.byref(args()))
    assert full == 3 * up(4 * tiles)                                # three float partials per 32 x 22 tile
    blocks = 3 * ((1080 * 1920 + 1023) // 1024)                     # sized for the scalar route: 1024 elements per block
    stream = lib.sfgs_metrics_scratch_bytes(C.byref(args(flags=L.METRICS_CLAMP)))
    assert stream == up(16 * blocks)                                # two doubles per block
    assert lib.sfgs_metrics_scratch_bytes(C.byref(args(P=1, H=1, W=1))) == 3 * 256
    assert lib.sfgs_metrics_scratch_bytes(None) == 0
    assert lib.sfgs_metrics_scratch_bytes(C.byref(args(struct_size=8))) == 0
    assert b"struct_size" in lib.sfgs_last_error()
    for bad in (dict(P=0), dict(P=5), dict(H=0), dict(W=0), dict(H=-2), dict(a=None), dict(b=None), dict(flags=8), dict(flags=-1)):
        assert lib.sfgs_metrics_scratch_bytes(C.byref(args(**bad))) == 0, bad
        # status codes before any HIP call: the pointers are never dereferenced
        assert lib.sfgs_metrics_view(C.byref(args(**bad)), fp, fp, full, None) == -1, bad
    assert lib.sfgs_metrics_scratch_bytes(C.byref(args(H=32768, W=32768))) == 0             # a plane of 2^32 bytes
    assert lib.sfgs_metrics_view(C.byref(args(H=32768, W=32768)), fp, fp, full, None) == -4
    assert b"2^30" in lib.sfgs_last_error()
    assert lib.sfgs_metrics_scratch_bytes(C.byref(args(H=32768, W=32767))) > 0
    assert lib.sfgs_metrics_view(C.byref(args()), None, fp, full, None) == -1
    assert lib.sfgs_metrics_view(C.byref(args()), fp, None, full, None) == -1
    assert lib.sfgs_metrics_view(C.byref(args()), fp, fp, full - 1, None) == -3              # SFGS_E_CAPACITY
    assert b"scratch too small" in lib.sfgs_last_error()
