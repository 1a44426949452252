"""sfgs.geometry without a GPU: the numpy restatement of the reference's geometry evaluation (tests/geometry_np.py, what the
kernels are held to) agrees with the reference's own run (tests/golden/make_golden_geometry.py); the two conditions the golden
was made under hold on the recorded values; the downsample corner rule; DsmGrid.from_metadata; the argument checks run before
the library is loaded; the C header, the library and the ctypes binding agree on ABI 22. The kernels: tests/test_gpu_geometry.py.

Tolerances. Points: the float64 coordinate error of a re-ordered evaluation is <= ~8 roundings x 3.3e6 m x 2^-53 ~ 3e-9 m
(east, north at UTM magnitude); heights (<= 1e3 m): 8 x 1e3 x 2^-53 ~ 1e-12, bound 1e-10 m. Statistics of the registration:
<= 5e4 float64 terms, worst case n 2^-53 ~ 6e-12 relative, bound 1e-10. Shifts, counts, NaN patterns: exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import geometry_np as gnp
from sfgs import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_geometry.npz")
ENTRY_POINTS = ("sfgs_dsm_accumulate", "sfgs_dsm_finalize", "sfgs_dsmr_scratch_bytes", "sfgs_dsmr_register",
                "sfgs_dsm_apply_shift", "sfgs_dsm_metrics_scratch_bytes", "sfgs_dsm_metrics")
G = np.load(GOLDEN)
REG_TAGS = sorted(k[len("reg_"):-len("_shift")] for k in G.files if k.startswith("reg_") and k.endswith("_shift"))
REL = 1e-10


def f64(a):
    return np.asarray(a).astype(np.float64)


def test_golden_covers_the_cases_it_promises():
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert {"9x7", "100x101", "101x102", "110x130_shapes", "205x210", "101x102_negodd_init", "40x50_irange1", "40x50_irange7",
            "40x50_scaling"} <= set(REG_TAGS)
    assert G["reg_110x130_shapes_ref"].shape != G["reg_110x130_shapes_sec"].shape
    np.testing.assert_array_equal(G["reg_110x130_shapes_shift"], [7, -3])
    assert len(G["reg_205x210_margins"]) == 3 and len(G["reg_101x102_margins"]) == 2 and len(G["reg_100x101_margins"]) == 1
    s = G["reg_101x102_negodd_init_shift"]
    assert s[0] < 0 and s[0] % 2 == 1 and tuple(G["reg_101x102_negodd_init_params"][2:]) == (-3, 3)
    for t in ("110x130_shapes", "205x210"):
        for name in ("ref", "sec"):
            nan = np.isnan(f64(G[f"reg_{t}_{name}"])).mean()
            assert 0.05 <= nan <= 0.10, (t, name, nan)
    d = G["pc_depth"]
    assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (d == 0).any() and (d < 0).any()
    assert G["city_origin"][0] == 4.0e5 and G["city_origin"][1] == 3.3e6


def test_the_two_conditions_hold_on_the_recorded_values():
    assert G["pc_cell_margin"] >= 1e-6 and G["city_cell_margin"] >= 1e-6
    pts = np.concatenate([G["pc_points"], G["pc_points_masked"]])
    qx, qy = gnp.cell_coords(pts, tuple(G["pc_grid"]))
    q = np.concatenate([qx, qy])
    assert np.abs(q - np.rint(q)).min() >= 1e-6
    for t in REG_TAGS:
        m = G[f"reg_{t}_margins"]
        assert (m[:, 0] - m[:, 1] >= 1e-6).all(), (t, m)


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------------
def assert_points_close(got, want):
    assert got.shape == want.shape
    np.testing.assert_allclose(got[:, :2], want[:, :2], rtol=0, atol=3e-9)
    np.testing.assert_allclose(got[:, 2], want[:, 2], rtol=0, atol=1e-10)


def test_unproject_equals_the_reference_points():
    fx, fy, cx, cy = G["pc_intr"]
    for mask, want in ((None, G["pc_points"]), (G["pc_mask"], G["pc_points_masked"])):
        got = gnp.unproject(G["pc_depth"], G["pc_R"], G["pc_T"], fx, fy, cx, cy, origin=G["pc_origin"], mask=mask)
        assert_points_close(got, want)
    # the planted +inf is dropped here (the reference's caller scrubs it), the other planted values by `depth > 0`
    assert len(G["pc_points"]) == int(((G["pc_depth"] > 0) & np.isfinite(G["pc_depth"])).sum())


def city():
    grid = gnp_grid_from_metadata(G["city_meta"])
    cams = [(R, T) + tuple(i) for R, T, i in zip(G["city_R"], G["city_T"], G["city_intr"])]
    return grid, cams


def gnp_grid_from_metadata(m):
    from sfgs.geometry import DsmGrid
    return tuple(DsmGrid.from_metadata(m))


def test_max_dsm_of_the_stacked_cloud_equals_the_reference():
    grid, cams = city()
    clouds = [gnp.unproject(d, *cam, origin=G["city_origin"]) for d, cam in zip(G["city_depths"], cams)]
    for cloud, want, n in ((np.vstack(clouds), G["city_dsm"], int(G["city_num_points"])), (clouds[0], G["city_dsm_view0"], None)):
        got, landed = gnp.dsm_max(cloud, grid)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)
        assert landed <= len(cloud) and (n is None or len(cloud) == n)
    assert 0.3 < (~np.isnan(G["city_dsm"])).mean()


def test_mean_rule_is_the_one_written_down():
    grid = (10.0, 20.0, 4, 3, 2.0)                     # cells of 2 m; x in [10, 18), y in (14, 20]
    pts = np.array([[11.0, 19.0, 5.0], [11.5, 19.5, 7.0], [17.9, 14.1, 1.0], [9.0, 19.0, 100.0], [30.0, 19.0, 9.0]])
    got0, n0 = gnp.dsm_mean(pts, grid, 0)
    assert n0 == 4                                      # (9, 19) is in the (-1, 0) band and lands in column 0; (30, 19) is outside
    np.testing.assert_array_equal(np.isnan(got0), ~np.isin(np.arange(12).reshape(3, 4), [0, 11]))
    assert got0[0, 0] == (5.0 + 7.0 + 100.0) / 3 and got0[2, 3] == 1.0
    got1, _ = gnp.dsm_mean(pts, grid, 1)
    assert got1[1, 1] == (5.0 + 7.0 + 100.0) / 3 and got1[1, 2] == 1.0 and np.isnan(got1[0, 2]) and np.isnan(got1[2, 0])
    mx, _ = gnp.dsm_max(pts, grid)
    assert mx[0, 0] == 100.0 and mx[2, 3] == 1.0 and np.isnan(mx).sum() == 10


def test_grid_from_metadata_reads_the_four_numbers_like_the_reference():
    from sfgs.geometry import DsmGrid
    g = DsmGrid.from_metadata([4.0e5, 3.3e6, 512.9, 0.5])
    assert g == (4.0e5, 3.3e6 + 512 * 0.5, 512, 512, 0.5) and isinstance(g.xsize, int)
    g = DsmGrid.from_metadata(np.array([1.0, 2.0, 64.0, 0.5]), resolution=0.25)
    assert g == (1.0, 2.0 + 64 * 0.25, 64, 64, 0.25)
    for bad in ([1, 2, 3], [1, 2, 0, 0.5], [1, 2, 8, 0.0], [1, 2, 8, -1.0], [np.nan, 2, 8, 1.0]):
        with pytest.raises(ValueError):
            DsmGrid.from_metadata(bad)
    with pytest.raises(ValueError):
        DsmGrid(0.0, 0.0, 2.5, 2, 1.0)


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------------
def test_downsample_corner_rule():
    out = gnp.downsample2x(np.arange(35, dtype=np.float64).reshape(5, 7))
    assert out.shape == (3, 4) and out[0, 0] == 12 and out[0, 3] == 16.5
    np.testing.assert_array_equal(out, G["ds_5x7_out"])
    got = gnp.downsample2x(G["ds_holes_in"])
    assert got.shape == (51, 51) and np.isinf(G["ds_holes_in"]).sum() == 3 and np.isfinite(got[~np.isnan(got)]).all()
    np.testing.assert_array_equal(got, G["ds_holes_out"])       # the same four terms in the same order: the same bits
    assert np.isnan(gnp.downsample2x(np.full((3, 3), np.inf))).all()
    assert gnp.downsample2x(np.array([[5.0]]))[0, 0] == 5.0


def test_mean_std_and_apply_shift_equal_the_reference():
    ref, sec = f64(G["ms_ref"]), f64(G["ms_sec"])
    assert ref.shape != sec.shape and np.isinf(sec).sum() == 2
    for (dx, dy), want in zip(G["ms_shifts"], G["ms_stats"]):
        got = gnp.mean_std(ref, sec, int(dx), int(dy))
        np.testing.assert_allclose(got[:5], want, rtol=REL, atol=0)
    assert gnp.mean_std(ref, sec, 500, 0)[5] == 0
    dx, dy, a, b = G["as_params"]
    got = gnp.apply_shift(sec, int(dx), int(dy), a, b)
    np.testing.assert_array_equal(got, G["as_out"])
    assert np.isnan(got[:2]).all() and np.isnan(got[:, -3:]).all()      # (dx, dy) = (3, -2): rows above, columns right of sec


@pytest.mark.parametrize("tag", REG_TAGS)
def test_registration_restatement_equals_the_reference(tag):
    irange, scaling, ix, iy = (int(v) for v in G[f"reg_{tag}_params"])
    margins = []
    dx, dy, a, b, stats = gnp.compute_shift(f64(G[f"reg_{tag}_ref"]), f64(G[f"reg_{tag}_sec"]), irange, bool(scaling), (ix, iy),
                                            margins)
    assert (dx, dy) == tuple(G[f"reg_{tag}_shift"])
    np.testing.assert_allclose([a, b], G[f"reg_{tag}_ab"], rtol=REL, atol=1e-12)
    np.testing.assert_allclose(stats, G[f"reg_{tag}_stats"], rtol=REL, atol=0)
    np.testing.assert_allclose(np.asarray(margins), G[f"reg_{tag}_margins"], rtol=1e-9, atol=0)


def test_skipped_shifts():
    one = np.array([[3.0]])
    assert gnp.compute_shift(one, one)[:2] == (0, 0) and np.isnan(gnp.compute_shift(one, one)[3])
    assert gnp.compute_shift(one, one, scaling=False)[2] == 1.0 and np.isnan(gnp.compute_shift(one, one, scaling=True)[2])
    ref, _ = gnp.shifted_pair(30, 40, 3, 0, 0, 0.0)
    dx, dy, a, b, _ = gnp.compute_shift(ref, np.full((30, 40), np.nan), init=(2, -1))
    assert (dx, dy, a) == (2, -1, 1.0) and np.isnan(b)
    flat = np.full((20, 20), 7.0)                       # sigma_u = 0 at every shift
    assert gnp.compute_shift(flat, ref[:20, :20])[:2] == (0, 0)


# ---- stage 3 ---------------------------------------------------------------------------------------------------------------------
def test_metrics_equal_the_reference():
    pred, gt, keep = f64(G["met_pred"]), f64(G["met_gt"]), G["met_keep"]
    for tag, mask in (("plain", None), ("masked", keep)):
        got = gnp.dsm_metrics(pred, gt, mask)
        want = G[f"met_{tag}"]
        np.testing.assert_allclose([got["mae"], got["rmse"]], want[:2], rtol=REL, atol=0)
        assert got["valid_pixels"] == want[2] and got["completeness"] == want[3]
        assert np.isfinite(want).all() and want[2] > 1000
    with np.errstate(invalid="ignore"):
        inf = gnp.dsm_metrics(f64(G["met_pred_inf"]), gt)         # an infinite height is valid (`~isnan`): counted, and mae = inf
    assert inf["valid_pixels"] == G["met_inf"][2] > G["met_plain"][2] and inf["completeness"] == G["met_inf"][3]
    assert np.isinf(inf["mae"]) and np.isinf(G["met_inf"][0]) and np.isfinite(G["met_dz"])
    none = gnp.dsm_metrics(np.full_like(pred, np.nan), gt)
    assert np.isnan(none["mae"]) and np.isnan(none["rmse"]) and none["valid_pixels"] == 0 and none["completeness"] == 0.0
    np.testing.assert_array_equal(G["met_none"][2:], [0, 0])
    np.testing.assert_allclose(gnp.register_simple(pred, gt), G["met_dz"], rtol=REL, atol=0)
    assert gnp.dsm_metrics(pred, np.full_like(gt, np.nan))["completeness"] == 0.0
    shifted = gnp.dsm_metrics(pred, gt, keep, shift=(1, -2, 1.0, 0.5))
    assert shifted == gnp.dsm_metrics(gnp.apply_shift(pred, 1, -2, 1.0, 0.5), gt, keep)


# ---- sfgs.geometry: validation ---------------------------------------------------------------------------------------------------
def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    from sfgs import geometry as geo
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    assert set(geo.__all__) >= {"DsmGrid", "DsmAccumulator", "register", "apply_shift", "dsm_metrics", "register_simple", "evaluate_dsm"}
    grid = geo.DsmGrid(0.0, 8.0, 8, 8, 1.0)
    for kw in ({"mode": "min"}, {"radius": 4}, {"radius": -1}, {"radius": 1.5}, {"device": "cpu"}):
        with pytest.raises(ValueError):
            geo.DsmAccumulator(grid, **kw)
    with pytest.raises(ValueError):
        geo.DsmAccumulator((0.0, 8.0, 8, 8, 1.0))
    acc = object.__new__(geo.DsmAccumulator)              # the checks of add_depth need no device
    acc.grid, acc.mode, acc.radius, acc.device = grid, "max", 1, torch.device("cuda:0")
    cam = dict(R=np.eye(3), T=np.zeros(3), focal_x=100.0, focal_y=100.0)
    d = torch.ones(6, 8)
    for bad in (np.ones((6, 8), np.float32), d.double(), torch.ones(2, 6, 8), torch.ones(0, 8)):
        with pytest.raises(ValueError):
            acc.add_depth(bad, **cam)
    for kw in ({"mask": torch.ones(6, 8)}, {"mask": torch.ones(6, 7, dtype=torch.bool)}, {"origin": [1.0, 2.0]},
               {"origin": [1.0, 2.0, np.nan]}, {"focal_x": 0.0}, {"R": np.eye(2)}, {"T": [0.0, 1.0]}):
        with pytest.raises(ValueError):
            acc.add_depth(d, **{**cam, **kw})
    with pytest.raises(ValueError, match="GPU"):
        acc.add_depth(d, **cam)
    r = torch.ones(9, 7, dtype=torch.float64)
    for kw in ({"irange": 0}, {"irange": 8}, {"irange": 2.0}, {"init": (1,)}, {"init": (1 << 21, 0)}):
        with pytest.raises(ValueError):
            geo.register(r, r, **kw)
    for bad in (r.numpy(), r.to(torch.int32), torch.ones(1, 9, 7), torch.ones(0, 7)):
        with pytest.raises(ValueError):
            geo.register(bad, r)
        with pytest.raises(ValueError):
            geo.register(r, bad)
        with pytest.raises(ValueError):
            geo.dsm_metrics(bad, r)
        with pytest.raises(ValueError):
            geo.apply_shift(bad, None)
    with pytest.raises(ValueError, match="GPU"):
        geo.register(r, r)
    with pytest.raises(ValueError):
        geo.dsm_metrics(r, torch.ones(9, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        geo.dsm_metrics(r, r, mask=torch.ones(9, 7))
    with pytest.raises(ValueError, match="GPU"):
        geo.dsm_metrics(r, r)
    with pytest.raises(ValueError, match="GPU"):
        geo.register_simple(r, r)
    with pytest.raises(ValueError):
        geo.evaluate_dsm([d], [], grid, torch.ones(8, 8))
    with pytest.raises(ValueError):
        geo.evaluate_dsm([d], [cam], grid, torch.ones(8, 9))
    assert not hasattr(geo, "install")


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
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() and L.ABI_VERSION >= 22
    assert re.search(r"#define SFGS_DSM_MAX 0", hdr) and re.search(r"#define SFGS_DSM_MEAN 1", hdr)
    assert (L.DSM_MAX, L.DSM_MEAN) == (0, 1)
    for struct in (L.SfgsDsmViewArgs, L.SfgsDsmrArgs):
        name = struct.__name__
        fields = [f for f, _ in struct._fields_]
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        declared = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                    for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
        assert declared == fields, name
        src = tmp_path / f"{name}.c"
        prints = "\n".join(f'  printf("{f} %zu\\n", offsetof({name}, {f}));' for f in fields)
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                       f'  printf("sizeof %zu\\n", sizeof({name}));\n{prints}\n  return 0;\n}}\n')
        exe = tmp_path / name
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
        assert int(out["sizeof"]) == C.sizeof(struct)
        for f in fields:
            assert int(out[f]) == getattr(struct, f).offset, (name, f)


def test_gpu_free_entry_points_validate_their_arguments():
    lib = L.load()
    dummy = C.c_double(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value

    def view(**kw):
        a = L.SfgsDsmViewArgs(C.sizeof(L.SfgsDsmViewArgs), 1024, 1024, fp, None, (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1),
                              (C.c_double * 3)(), (C.c_double * 3)(), 512.0, 512.0, 2000.0, 2000.0, 0.0, 512.0, 0.5, 1024, 1024,
                              L.DSM_MAX, 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for bad in ({"struct_size": 8}, {"H": 0}, {"W": -1}, {"depth": None}, {"xsize": 0}, {"ysize": -3}, {"mode": 2}, {"radius": 4},
                {"radius": -1}, {"resolution": 0.0}, {"focal_x": 0.0}):
        assert lib.sfgs_dsm_accumulate(C.byref(view(**bad)), fp, fp, fp, None) == -1, bad
    assert lib.sfgs_dsm_accumulate(None, fp, fp, fp, None) == -1
    assert lib.sfgs_dsm_accumulate(C.byref(view()), None, fp, fp, None) == -1
    assert lib.sfgs_dsm_accumulate(C.byref(view()), fp, fp, None, None) == -1
    assert lib.sfgs_dsm_accumulate(C.byref(view(mode=L.DSM_MEAN)), fp, None, fp, None) == -1
    assert lib.sfgs_dsm_accumulate(C.byref(view(H=32768, W=32769)), fp, fp, fp, None) == -4
    assert lib.sfgs_dsm_accumulate(C.byref(view(xsize=16385, ysize=16384)), fp, fp, fp, None) == -4
    assert lib.sfgs_dsm_finalize(L.DSM_MAX, 0, 4, fp, None, fp, None) == -1
    assert lib.sfgs_dsm_finalize(7, 4, 4, fp, None, fp, None) == -1
    assert lib.sfgs_dsm_finalize(L.DSM_MEAN, 4, 4, fp, None, fp, None) == -1
    assert lib.sfgs_dsm_finalize(L.DSM_MAX, 4, 4, fp, None, None, None) == -1

    def reg(**kw):
        a = L.SfgsDsmrArgs(C.sizeof(L.SfgsDsmrArgs), 1024, 1024, 1000, 1100, fp, fp, 5, 0, 0, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    full = lib.sfgs_dsmr_scratch_bytes(C.byref(reg()))
    # four half-size levels of both rasters (512 ... 64) and the level-0 partials: 3 sums x 32 x 32 tiles x 121 shifts
    assert full >= 3 * 1024 * 121 * 8 + sum(8 * (1024 >> k) ** 2 for k in range(1, 5))
    assert full < 16 << 20
    assert lib.sfgs_dsmr_scratch_bytes(C.byref(reg(ref_h=100, ref_w=100))) < 3 * 16 * 121 * 8 + 8192     # no pyramid: partials, means, per-level results
    assert lib.sfgs_dsmr_scratch_bytes(None) == 0
    i32, f8 = (C.c_int32 * 2)(), (C.c_double * 8)()
    for bad in ({"struct_size": 4}, {"ref_h": 0}, {"sec_w": 0}, {"irange": 0}, {"irange": 8}, {"ref": None}, {"sec": None},
                {"init_dx": 1 << 21}):
        assert lib.sfgs_dsmr_scratch_bytes(C.byref(reg(**bad))) == 0, bad
        assert lib.sfgs_dsmr_register(C.byref(reg(**bad)), i32, f8, fp, full, None) == -1, bad
    assert lib.sfgs_dsmr_register(C.byref(reg(ref_w=32769)), i32, f8, fp, full, None) == -4
    assert lib.sfgs_dsmr_register(C.byref(reg()), None, f8, fp, full, None) == -1
    assert lib.sfgs_dsmr_register(C.byref(reg()), i32, f8, None, full, None) == -1
    assert lib.sfgs_dsmr_register(C.byref(reg()), i32, f8, fp, full - 1, None) == -3
    assert lib.sfgs_dsm_apply_shift(None, 4, 4, i32, f8, fp, None) == -1
    assert lib.sfgs_dsm_apply_shift(fp, 4, 0, i32, f8, fp, None) == -1
    assert lib.sfgs_dsm_apply_shift(fp, 4, 4, None, f8, fp, None) == -1
    need = lib.sfgs_dsm_metrics_scratch_bytes(1024, 1024)
    assert 0 < need <= 64 << 10 and lib.sfgs_dsm_metrics_scratch_bytes(0, 4) == 0
    assert lib.sfgs_dsm_metrics(fp, fp, None, 0, 4, None, None, fp, fp, need, None) == -1
    assert lib.sfgs_dsm_metrics(fp, None, None, 4, 4, None, None, fp, fp, need, None) == -1
    assert lib.sfgs_dsm_metrics(fp, fp, None, 4, 4, i32, None, fp, fp, need, None) == -1
    assert lib.sfgs_dsm_metrics(fp, fp, None, 4, 4, None, None, fp, fp, need - 1, None) == -3
