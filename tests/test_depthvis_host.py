"""sfgs.depthvis without a GPU: the float32 restatement of the reference's colorize_depth_torch (tests/depthvis_np.py, what
the kernels are held to) equals every golden case bit for bit, quantiles included; spectral_lut() is the reference's table;
where the reference tree and matplotlib exist, the restatement equals the LIVE reference on fresh full-size frames; the
argument checks run before the library is loaded; install / uninstall rebind one name; the C header, the library and the
ctypes binding agree. The kernels themselves: tests/test_gpu_depthvis.py."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest
import torch

import depthvis_np as dnp
from sfgs import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_depthvis.npz")
ENTRY_POINTS = ("sfgs_depthvis_scratch_bytes", "sfgs_depthvis_forward", "sfgs_frame_quantize")


def golden_cases():
    g = np.load(GOLDEN)
    tags = sorted(k[:-len("_depth")] for k in g.files if k.endswith("_depth"))
    return g, tags


def same_bits(a, b):
    """float32 arrays equal bit for bit, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    canon = lambda v: np.where(np.isnan(v), np.uint32(0x7fc00000), v.view(np.uint32))
    return a.shape == b.shape and np.array_equal(canon(a), canon(b))


# ---- the restatement against the golden and the live reference -------------------------------------------------------------------
def test_golden_covers_the_cases_it_promises():
    g, tags = golden_cases()
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert g["spectral_lut"].shape == (256, 3) and g["spectral_lut"].dtype == np.uint8
    shapes = {g[f"{t}_depth"].shape for t in tags}
    assert {(1, 1), (2, 1), (37, 53), (135, 240)} <= shapes
    for kind in dnp.KINDS:
        assert f"{kind}_n" in tags and f"{kind}_m" in tags, kind
    assert any(not bool(g[f"{t}_normalize"]) for t in tags)
    special = g["special_n_depth"]
    assert np.isnan(special).any() and np.isposinf(special).any() and np.isneginf(special).any()


def test_numpy_restatement_equals_every_golden_case_bit_for_bit():
    g, tags = golden_cases()
    lut = g["spectral_lut"]
    assert len(tags) >= 20
    for t in tags:
        depth = g[f"{t}_depth"]
        mask = g[f"{t}_mask"] if f"{t}_mask" in g.files else None
        rgb, lo, hi = dnp.colorize(depth, lut, mask, bool(g[f"{t}_normalize"]))
        assert same_bits(dnp.to_float_chw(rgb), g[f"{t}_result"]), t
        assert same_bits(np.asarray(dnp.quantiles(dnp.disparity(depth, mask))), g[f"{t}_quantiles"]), t
        if bool(g[f"{t}_normalize"]):
            assert same_bits(np.asarray([lo, hi]), g[f"{t}_quantiles"]), t


def test_spectral_lut_is_the_reference_table():
    from sfgs import depthvis
    g, _ = golden_cases()
    lut = depthvis.spectral_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    np.testing.assert_array_equal(lut, g["spectral_lut"])
    np.testing.assert_array_equal(lut[0], depthvis._SPECTRAL_ANCHORS[0])
    np.testing.assert_array_equal(lut[255], depthvis._SPECTRAL_ANCHORS[-1])


@pytest.fixture()
def reference_colorize():
    saved_path, saved_mods = list(sys.path), set(sys.modules)
    for name in ("plyfile", "OpenEXR", "Imath", "mediapy"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF)
    import render_video
    yield render_video.colorize_depth_torch
    sys.path[:] = saved_path
    for m in set(sys.modules) - saved_mods:
        del sys.modules[m]


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "render_video.py")) or importlib.util.find_spec("matplotlib") is None,
                    reason="reference tree or matplotlib not present (GPU box)")
@pytest.mark.parametrize("H,W", [(1080, 1920), (1024, 1024)])
def test_restatement_equals_the_live_reference_on_fresh_full_size_frames(reference_colorize, H, W):
    from sfgs import depthvis
    lut = depthvis.spectral_lut()
    seed = int.from_bytes(os.urandom(4), "little")            # fresh every run; printed so that a failure can be replayed
    print(f"seed {seed}")
    for i, kind in enumerate(("smooth", "uniform", "tied", "special")):
        depth = dnp.make_depth(kind, H, W, seed + i)
        for mask in (None, dnp.make_mask(H, W, seed + i)):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                want = reference_colorize(torch.from_numpy(depth)[None], None if mask is None else torch.from_numpy(mask)[None])
            rgb, _, _ = dnp.colorize(depth, lut, mask)
            assert same_bits(dnp.to_float_chw(rgb), want.numpy()), (kind, mask is not None, seed)


def test_quantize_frame_restatement_is_the_numpy_formula():
    rng = np.random.default_rng(5)
    img = rng.uniform(-0.2, 1.2, (3, 19, 23)).astype(np.float32)
    want = (img.transpose(1, 2, 0) * 255 + 0.5).clip(0, 255).astype(np.uint8)      # render_video.py:264
    assert (img.transpose(1, 2, 0) * 255 + 0.5).dtype == np.float32
    np.testing.assert_array_equal(dnp.quantize_frame(img), want)
    img[0, 0, 0] = np.nan
    assert dnp.quantize_frame(img)[0, 0, 0] == 0


# ---- sfgs.depthvis: validation and the hook --------------------------------------------------------------------------------------
def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    from sfgs import depthvis
    assert set(depthvis.__all__) >= {"colorize_depth", "quantize_frame", "spectral_lut", "install", "uninstall"}

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "load", no_library)
    d = torch.ones(1, 6, 8)
    with pytest.raises(ValueError, match="depth must be a tensor"):
        depthvis.colorize_depth(np.ones((6, 8), np.float32))
    for bad in (d.double(), d.half(), d.long()):
        with pytest.raises(ValueError, match="depth must be float32"):
            depthvis.colorize_depth(bad)
    for bad in (torch.ones(2, 6, 8), torch.ones(6), torch.ones(1, 1, 6, 8), torch.ones(1, 0, 8), torch.ones(())):
        with pytest.raises(ValueError, match=r"\[1,H,W\] or \[H,W\]"):
            depthvis.colorize_depth(bad)
    with pytest.raises(ValueError, match="mask must be a tensor or None"):
        depthvis.colorize_depth(d, mask=np.ones((6, 8), bool))
    for bad in (torch.ones(1, 6, 8), torch.ones(6, 8, dtype=torch.int32)):
        with pytest.raises(ValueError, match="mask must be bool or uint8"):
            depthvis.colorize_depth(d, mask=bad)
    for bad in (torch.ones(6, 9, dtype=torch.bool), torch.ones(2, 6, 8, dtype=torch.bool), torch.ones(48, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"mask must be \[6,8\] or \[1,6,8\]"):
            depthvis.colorize_depth(d, mask=bad)
    with pytest.raises(ValueError, match="out must be"):
        depthvis.colorize_depth(d, out="uint8_chw")
    for bad in (torch.zeros(256, 3), torch.zeros(256, 4, dtype=torch.uint8), np.zeros((256, 3), np.uint8)):
        with pytest.raises(ValueError, match="lut must be a uint8 tensor"):
            depthvis.colorize_depth(d, lut=bad)
    with pytest.raises(ValueError, match="cmap must be a colormap name"):
        depthvis.colorize_depth(d, cmap=None)
    # device: everything else is right, the tensor is on the CPU -- no fallback, by design
    for ok in (d, d[0]):
        with pytest.raises(ValueError, match="depth must be a GPU tensor"):
            depthvis.colorize_depth(ok, mask=torch.ones(6, 8, dtype=torch.bool), out="uint8_hwc")
    with pytest.raises(ValueError, match="depth must be a GPU tensor"):
        depthvis.colorize_depth_torch(d)
    with pytest.raises(ValueError, match="image must be a tensor"):
        depthvis.quantize_frame(np.zeros((3, 4, 4), np.float32))
    with pytest.raises(ValueError, match="image must be float32"):
        depthvis.quantize_frame(torch.zeros(3, 4, 4, dtype=torch.float64))
    for bad in (torch.zeros(4, 4, 3), torch.zeros(1, 4, 4), torch.zeros(3, 0, 4), torch.zeros(3, 4)):
        with pytest.raises(ValueError, match=r"\[3,H,W\]"):
            depthvis.quantize_frame(bad)
    with pytest.raises(ValueError, match="image must be a GPU tensor"):
        depthvis.quantize_frame(torch.zeros(3, 4, 4))


def test_unknown_colormap_names_raise_value_error():
    from sfgs import depthvis
    with pytest.raises(ValueError, match="cmap"):
        depthvis._named_lut("no_such_colormap_anywhere")
    if importlib.util.find_spec("matplotlib") is not None:
        lut = depthvis._named_lut("viridis")
        assert lut.shape == (256, 3) and lut.dtype == np.uint8 and tuple(lut[0]) == (68, 1, 84)


def test_install_and_uninstall_rebind_one_name():
    from sfgs import depthvis

    def original(depth_tensor, mask=None, normalize=True, cmap='Spectral'):
        return "original"

    def other():
        return "other"
    mod = types.ModuleType("render_video_stand_in")
    mod.colorize_depth_torch, mod.render_set, mod.torch = original, other, torch
    before = dict(vars(mod))
    depthvis.install(mod)
    assert mod.colorize_depth_torch is depthvis.colorize_depth_torch
    changed = {k for k in vars(mod) if vars(mod)[k] is not before.get(k)}
    assert changed == {"colorize_depth_torch"}
    hooked = mod.colorize_depth_torch
    depthvis.install(mod)                                     # a second install is a no-op ...
    assert mod.colorize_depth_torch is hooked
    depthvis.uninstall(mod)                                   # ... and one uninstall restores the original
    assert mod.colorize_depth_torch is original and dict(vars(mod)) == before
    depthvis.uninstall(mod)
    assert mod.colorize_depth_torch is original
    # the reference's signature
    import inspect
    assert str(inspect.signature(depthvis.colorize_depth_torch)) == str(inspect.signature(original))
    with pytest.raises(AttributeError):
        depthvis.install(types.ModuleType("no_such_function_here"))


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
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() and L.ABI_VERSION >= 21
    assert "render_video.py:129-170" in hdr and "render_video.py:264" in hdr
    assert re.search(r"#define SFGS_DEPTHVIS_FLOAT_CHW 0", hdr) and re.search(r"#define SFGS_DEPTHVIS_UINT8_HWC 1", hdr)
    assert (L.DEPTHVIS_FLOAT_CHW, L.DEPTHVIS_UINT8_HWC) == (0, 1)
    fields = [f for f, _ in L.SfgsDepthVisArgs._fields_]
    assert fields == ["struct_size", "H", "W", "depth", "mask", "lut", "normalize", "out_kind"]
    body = re.search(r"typedef struct SfgsDepthVisArgs \{(.*?)\} SfgsDepthVisArgs;", hdr, re.S).group(1)
    declared = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert declared == fields
    src = tmp_path / "layout.c"
    prints = "\n".join(f'  printf("{f} %zu\\n", offsetof(SfgsDepthVisArgs, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                   f'  printf("sizeof %zu\\n", sizeof(SfgsDepthVisArgs));\n{prints}\n  return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SfgsDepthVisArgs)
    for f in fields:
        assert int(out[f]) == getattr(L.SfgsDepthVisArgs, f).offset, f


def test_gpu_free_entry_points_validate_their_arguments():
    lib = L.load()
    dummy = C.c_double(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value

    def args(**kw):
        a = L.SfgsDepthVisArgs(C.sizeof(L.SfgsDepthVisArgs), 1080, 1920, fp, None, fp, 1, L.DEPTHVIS_FLOAT_CHW)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    full = lib.sfgs_depthvis_scratch_bytes(C.byref(args()))
    # the state block and the histograms of the three passes (1 + 4 + 4 slots): nothing frame-sized
    assert full == 256 + 4 * (2048 + 4 * 2048 + 4 * 1024)
    assert lib.sfgs_depthvis_scratch_bytes(C.byref(args(H=2160, W=3840))) == full
    assert lib.sfgs_depthvis_scratch_bytes(C.byref(args(H=1, W=1, mask=fp, out_kind=L.DEPTHVIS_UINT8_HWC))) == full
    assert lib.sfgs_depthvis_scratch_bytes(None) == 0
    assert lib.sfgs_depthvis_scratch_bytes(C.byref(args(struct_size=8))) == 0
    assert b"struct_size" in lib.sfgs_last_error()
    for bad in (dict(H=0), dict(W=-3), dict(depth=None), dict(lut=None), dict(out_kind=2), dict(out_kind=-1)):
        assert lib.sfgs_depthvis_scratch_bytes(C.byref(args(**bad))) == 0, bad
        # status codes before any HIP call: the pointers are never dereferenced
        assert lib.sfgs_depthvis_forward(C.byref(args(**bad)), fp, fp, full, None) == -1, bad
    assert lib.sfgs_depthvis_forward(C.byref(args(H=32768, W=32769)), fp, fp, full, None) == -4
    assert b"2^30" in lib.sfgs_last_error()
    assert lib.sfgs_depthvis_forward(C.byref(args()), None, fp, full, None) == -1
    assert lib.sfgs_depthvis_forward(C.byref(args()), fp, None, full, None) == -1
    assert lib.sfgs_depthvis_forward(C.byref(args()), fp, fp, full - 1, None) == -3            # SFGS_E_CAPACITY
    assert b"scratch too small" in lib.sfgs_last_error()
    assert lib.sfgs_frame_quantize(None, 4, 4, fp, None) == -1
    assert lib.sfgs_frame_quantize(fp, 4, 4, None, None) == -1
    assert lib.sfgs_frame_quantize(fp, 0, 4, fp, None) == -1
    assert lib.sfgs_frame_quantize(fp, 32768, 32769, fp, None) == -4
