"""sfgs.ortho without a GPU: the restatement tests/ortho_np.py (what tests/test_gpu_ortho.py holds the kernels to) checked
against independent spellings -- the float32 key is strictly monotone, never 0 and invertible; its heights are float32 of
geometry_np.dsm_max; its resolve equals a per-cell loop --, the header, the library and the binding agree on the two new
symbols and on SfgsOrthoViewArgs with the ABI version unchanged, both entry points refuse every bad argument before any GPU
work, and the wrapper's argument checks run before the library is loaded."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import geometry_np as gnp
import ortho_np as onp
from sfgs import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sfgs_ortho_accumulate", "sfgs_ortho_resolve")
E_ARG = -1


def header():
    return open(os.path.join(ROOT, "include", "sfgs.h")).read()


def base_views(mask=None):
    grid, cams, depths, images, origin = onp.base_scene()
    return grid, [onp.View(d, i, c, mask if k == 1 else None, k + 1) for k, (d, i, c) in enumerate(zip(depths, images, cams))], origin


# ---- the key ---------------------------------------------------------------------------------------------------------------------
def test_key32_is_strictly_monotone_never_zero_and_invertible():
    f = np.float32
    tiny, big = f(1e-45), np.finfo(np.float32).max
    seq = [f(-np.inf), -big, np.nextafter(-big, f(0)), f(-4096.5), np.nextafter(f(-4096.0), f(-np.inf)), f(-4096.0), f(-1.0),
           -np.finfo(np.float32).tiny, -f(3) * tiny, -tiny, f(-0.0), f(0.0), tiny, f(2) * tiny, np.finfo(np.float32).tiny, f(1.0),
           np.nextafter(f(1.0), f(2.0)), f(60.0), np.nextafter(f(60.0), f(61.0)), f(4096.0), np.nextafter(f(4096.0), f(5000.0)), big,
           f(np.inf)]
    seq = np.array(seq, dtype=np.float32)
    assert (np.diff(seq.astype(np.float64)) >= 0).all() and seq[10] == seq[11] and np.signbit(seq[10]) and not np.signbit(seq[11])
    k = onp.key32(seq)
    assert k.dtype == np.uint32 and (k != 0).all()
    assert (np.diff(k.astype(np.int64)) > 0).all()         # strictly: -0 sorts just below +0, denormals and infinities in place
    back = onp.unkey32(k)
    np.testing.assert_array_equal(back.view(np.uint32), seq.view(np.uint32))
    rnd = np.random.default_rng(5).integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)
    np.testing.assert_array_equal(onp.unkey32(onp.key32(rnd.view(np.float32))).view(np.uint32), rnd)
    assert (onp.key32(rnd.view(np.float32)) != 0).all()
    assert onp.key32(np.array([np.uint32(0xffffffff)]).view(np.float32))[0] == 0                       # the only pattern that would be 0 ...
    assert np.isnan(np.array([np.uint32(0xffffffff)]).view(np.float32))[0]                              # ... is a NaN: no number maps to 0


def test_quantize_is_the_frame_quantisers_rule():
    v = np.array([np.nan, -1.0, 2.0, 0.0, 1.0, 0.5, 0.998, 1 / 255, 0.5 / 255], dtype=np.float32)
    np.testing.assert_array_equal(onp.quantize(v), [0, 0, 255, 0, 255, 128, 254, 1, 1])


# ---- the restatement against independent spellings ----------------------------------------------------------------------------
def test_heights_are_float32_of_the_dsm_maximum_on_the_base_scene():
    grid, views, origin = base_views()
    acc, n = onp.keys(views, grid, origin)
    pts = np.vstack([onp.unproject(v.depth, v.camera, origin) for v in views])
    dsm, landed = gnp.dsm_max(pts, grid)
    res = onp.resolve(acc, 0)
    assert n == landed == 5294 and int((acc != 0).sum()) == 487 and acc.shape == (24, 24)
    np.testing.assert_array_equal(res.height, dsm.astype(np.float32))           # NaN pattern included
    assert 10.8 < n / 487 < 11.0                                                # the atomics contend
    # the winner per cell, spelled as a loop over the points: maximum of (float32 height, r, g, b, tag) as a tuple
    best = {}
    for v in views:
        p = onp.unproject(v.depth, v.camera, origin)
        col = onp.quantize(v.image)[:, onp.used_pixels(v.depth)].T
        gx, gy, inside = gnp.cells(p, grid)
        for x, y, h, c in zip(gx, gy, p[inside, 2].astype(np.float32), col[inside]):
            t = (float(h), int(c[0]), int(c[1]), int(c[2]), v.tag)
            if (y, x) not in best or t > best[(y, x)]:
                best[(y, x)] = t
    assert len(best) == 487
    for (y, x), t in best.items():
        assert (float(res.height[y, x]),) + tuple(int(c) for c in res.rgb[y, x]) + (int(res.source[y, x]),) == t


@pytest.mark.parametrize("fill", [0, 1, 2, 3])
def test_resolve_equals_a_per_cell_loop(fill):
    grid, views, origin = base_views(mask=np.random.default_rng(3).random((40, 48)) > 0.3)
    acc, _ = onp.keys(views, grid, origin)
    res = onp.resolve(acc, fill)
    ysize, xsize = acc.shape
    empty = donated = 0
    cover = np.zeros(256, dtype=np.int64)
    for y in range(ysize):
        for x in range(xsize):
            k, st = int(acc[y, x]), 1
            if k == 0:
                window = acc[max(0, y - fill):y + fill + 1, max(0, x - fill):x + fill + 1]
                k = int(window.max())
                st = 2 if k else 0
            empty += st == 0
            donated += st == 2
            cover[k & 0xff] += 1
            assert res.state[y, x] == st and res.source[y, x] == (k & 0xff)
            assert tuple(res.rgb[y, x]) == ((k >> 24) & 0xff, (k >> 16) & 0xff, (k >> 8) & 0xff)
            if k:
                assert onp.key32(res.height[y:y + 1, x])[0] == k >> 32
            else:
                assert np.isnan(res.height[y, x]) and res.height[y, x:x + 1].view(np.uint32)[0] == 0x7fc00000
    np.testing.assert_array_equal(res.coverage, cover)
    assert res.coverage.sum() == ysize * xsize and res.coverage[0] == empty and (res.coverage[4:] == 0).all()
    assert (fill == 0) == (donated == 0)
    assert res.rgb.dtype == np.uint8 and res.height.dtype == np.float32 and res.source.dtype == np.uint8 and res.state.dtype == np.uint8


def test_the_base_scene_runs_both_branches_of_the_resolve():
    grid, views, origin = base_views()
    acc, _ = onp.keys(views, grid, origin)
    got = [(int((r.state == 0).sum()), int((r.state == 2).sum())) for r in (onp.resolve(acc, f) for f in range(4))]
    assert got == [(89, 0), (32, 57), (10, 79), (0, 89)]


# ---- header, library, binding ---------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(tmp_path):
    hdr = header()
    lib = L.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfgs.h"
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    declared_version = int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1))
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() == 28         # symbols were added, nothing else moved
    struct, name = L.SfgsOrthoViewArgs, "SfgsOrthoViewArgs"
    fields = [f for f, _ in struct._fields_]
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    declared = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert declared == fields
    dsm = [f for f, _ in L.SfgsDsmViewArgs._fields_]
    assert fields == [f for f in dsm if f not in ("mode", "radius")] + ["image", "tag"]
    src = tmp_path / f"{name}.c"
    prints = "\n".join(f'  printf("{f} %zu\\n", offsetof({name}, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                   f'  printf("sizeof %zu\\n", sizeof({name}));\n{prints}\n  return 0;\n}}\n')
    exe = tmp_path / name
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == C.sizeof(struct)
    for f in fields:
        assert int(out[f]) == getattr(struct, f).offset, f


def test_every_bad_argument_is_refused_with_the_dsm_entry_points_codes():
    lib = L.load()
    unsupported = int(re.search(r"SFGS_E_UNSUPPORTED\s*=\s*(-\d+)", header()).group(1))
    dummy = C.c_double(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value        # never dereferenced: every call below is refused first

    def view(**kw):
        a = L.SfgsOrthoViewArgs(C.sizeof(L.SfgsOrthoViewArgs), 64, 64, fp, None, (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1),
                                (C.c_double * 3)(), (C.c_double * 3)(), 32.0, 32.0, 100.0, 100.0, 0.0, 16.0, 0.5, 32, 32, fp, 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(rc, what, code=E_ARG):
        assert rc == code, what
        assert lib.sfgs_last_error(), what

    for bad in ({"struct_size": 8}, {"struct_size": C.sizeof(L.SfgsOrthoViewArgs) + 8}, {"H": 0}, {"W": -1}, {"xsize": 0}, {"ysize": -3},
                {"depth": None}, {"image": None}, {"focal_x": 0.0}, {"focal_y": 0.0}, {"resolution": 0.0}, {"resolution": -1.0},
                {"tag": 0}, {"tag": 256}, {"tag": -1}):
        refused(lib.sfgs_ortho_accumulate(C.byref(view(**bad)), fp, fp, None), bad)
    assert b"tag" in lib.sfgs_last_error()
    refused(lib.sfgs_ortho_accumulate(C.byref(view(H=1 << 16, W=1 << 15)), fp, fp, None), "H * W", unsupported)
    refused(lib.sfgs_ortho_accumulate(C.byref(view(xsize=1 << 15, ysize=1 << 14)), fp, fp, None), "cells", unsupported)
    refused(lib.sfgs_ortho_accumulate(None, fp, fp, None), "args")
    refused(lib.sfgs_ortho_accumulate(C.byref(view()), None, fp, None), "acc")
    refused(lib.sfgs_ortho_accumulate(C.byref(view()), fp, None, None), "num_points")
    ok = [32, 32, 0, fp, fp, fp, fp, fp, fp, None]
    for fill in (-1, 4, 100):
        refused(lib.sfgs_ortho_resolve(*(ok[:2] + [fill] + ok[3:])), fill)
    assert b"fill" in lib.sfgs_last_error()
    for xsize, ysize, code in ((0, 4, E_ARG), (4, -1, E_ARG), (1 << 15, 1 << 14, unsupported)):
        refused(lib.sfgs_ortho_resolve(*([xsize, ysize] + ok[2:])), (xsize, ysize), code)
    for i in range(3, 9):
        refused(lib.sfgs_ortho_resolve(*(ok[:i] + [None] + ok[i + 1:])), f"argument {i}")
    with pytest.raises(RuntimeError, match="libsfgs error -1"):
        L.check(lib.sfgs_ortho_resolve(*(ok[:2] + [7] + ok[3:])))


def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    from sfgs import geometry as geo
    from sfgs import ortho as om
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    assert set(om.__all__) >= {"OrthoAccumulator"}
    grid = geo.DsmGrid(0.0, 8.0, 8, 8, 1.0)
    for kw in ({"grid": (0.0, 8.0, 8, 8, 1.0)}, {"grid": grid, "device": "cpu"}):
        with pytest.raises(ValueError):
            om.OrthoAccumulator(**kw)
    cam = dict(R=np.eye(3), T=np.zeros(3), focal_x=100.0, focal_y=100.0)
    d, img = torch.ones(6, 8), torch.ones(3, 6, 8)
    o = object.__new__(om.OrthoAccumulator)               # the checks of add_depth need no device
    o.grid, o.device, o.num_views = grid, torch.device("cuda:0"), 0
    for bad in (np.ones((6, 8), np.float32), d.double(), torch.ones(2, 6, 8), torch.ones(0, 8)):
        with pytest.raises(ValueError):
            o.add_depth(bad, img, **cam)
    for bad in (None, np.ones((3, 6, 8), np.float32), img.double(), torch.ones(3, 6, 7), torch.ones(1, 6, 8), torch.ones(6, 8)):
        with pytest.raises(ValueError, match="image"):
            o.add_depth(d, bad, **cam)
    for kw in ({"mask": torch.ones(6, 8)}, {"mask": torch.ones(6, 7, dtype=torch.bool)}, {"origin": [1.0, 2.0]},
               {"origin": [1.0, 2.0, np.nan]}, {"focal_x": 0.0}, {"R": np.eye(2)}, {"T": [0.0, 1.0]}, {"tag": 0}, {"tag": 256},
               {"tag": 1.5}, {"tag": True}):
        with pytest.raises(ValueError):
            o.add_depth(d, img, **{**cam, **kw})
    with pytest.raises(ValueError, match="GPU"):
        o.add_depth(d, img, **cam)
    assert o.num_views == 0                                # a refused view is not counted
    o.num_views = 254
    with pytest.raises(ValueError, match="GPU"):           # the 255th implicit tag passes the tag check ...
        o.add_depth(d, img, **cam)
    o.num_views = 255
    with pytest.raises(ValueError, match="255"):           # ... the 256th does not
        o.add_depth(d, img, **cam)
    with pytest.raises(ValueError, match="GPU"):           # an explicit tag is still welcome
        o.add_depth(d, img, **cam, tag=7)
    for fill in (-1, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="fill"):
            o.result(fill=fill)
        with pytest.raises(ValueError, match="fill"):
            o.save_png("never_written.png", fill=fill)
    assert not os.path.exists("never_written.png")
    ns = type("Cam", (), cam)
    with pytest.raises(ValueError, match="OrthoAccumulator"):
        geo.evaluate_dsm([d], [ns], grid, torch.ones(8, 8), ortho=object(), images=[img])
    with pytest.raises(ValueError, match="images"):
        geo.evaluate_dsm([d], [ns], grid, torch.ones(8, 8), ortho=o)
    with pytest.raises(ValueError, match="images"):
        geo.evaluate_dsm([d], [ns], grid, torch.ones(8, 8), ortho=o, images=[img, img])


def test_world_file_lines_are_exact():
    from sfgs import geometry as geo
    from sfgs import ortho as om
    g = geo.DsmGrid(400000.1, 3300012.3, 24, 20, 0.3)
    lines = om.world_file_lines(g)
    assert lines == [repr(0.3), "0.0", "0.0", repr(-0.3), repr(400000.1 + 0.3 / 2), repr(3300012.3 - 0.3 / 2)]
    assert [float(s) for s in lines] == [0.3, 0.0, 0.0, -0.3, 400000.1 + 0.15, 3300012.3 - 0.15]
