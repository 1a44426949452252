"""sfgs.importance without a GPU: the conditions the reference of tests/importance_np.py has to meet (checked on references
alone), the committed K table against a re-measure, the ABI of the two entry points and their refusals (all made before any GPU
work), and the keep_mask / prune / prune_table logic on CPU tensors and arrays. The GPU side: tests/test_gpu_importance.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import grad_bounds as gb
import importance_np as inp
from sfgs import _lib as L
from sfgs import importance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", inp.CASES)
def test_reference_conditions(case):
    r = inp.reference(case)
    w = r["walk"]
    assert r["share"] <= gb.MASK_CAP, r["share"]
    # no decision of the unmasked pixels falls the other way under another exponential
    np.testing.assert_array_equal(inp.walk_jitter(case)["hits"], w["hits"])
    # the float32 restatement against the oracle's own double-precision red sum, in the oracle's units
    e = inp.in_units(w["sum"], r["osum"], r["ounit"])
    print(f"{case}: restatement against the oracle's sum {e.max():.3g} units; masked {r['share']:.3%}")
    assert e.max() <= 2.0, (int(e.argmax()), e.max())
    # ... and its unit sums against the oracle's
    seen = r["ounit"] > 0
    np.testing.assert_array_equal(seen, w["unit_sum"] > 0)
    assert (np.abs(w["unit_sum"] - r["ounit"])[seen] <= 1e-4 * r["ounit"][seen]).all()
    # what the sums are made of: the same rows, max <= sum <= hits * max, nothing negative
    assert ((w["hits"] > 0) == (w["sum"] > 0)).all() and (w["max"] <= w["sum"] * (1 + 1e-12)).all()
    assert (w["sum"] <= w["hits"] * w["max"] * (1 + 1e-12)).all() and (w["max"] <= 0.99).all()


def test_the_restatement_has_to_be_float32():
    """A chain of hundreds of small-alpha factors rounds at every step: in float64 the restatement is two orders of magnitude
    further from the oracle's own (float32-chain, double-sum) red sum than in float32."""
    r = inp.reference("sh3_jitter")
    w64 = inp.walk(r["R"], r["subpix"], r["keep"], dtype=np.float64)
    e64 = inp.in_units(w64["sum"], r["osum"], r["ounit"]).max()
    e32 = inp.in_units(r["walk"]["sum"], r["osum"], r["ounit"]).max()
    print(f"sh3_jitter: float64 restatement {e64:.3g} units from the oracle's sum, float32 {e32:.3g}")
    assert e64 > 50 * e32 and e32 <= 2.0


def test_cases_cover_the_paths_they_are_named_for():
    longest = {c: inp.reference(c)["R"].max_tile_list for c in inp.CASES}
    assert longest["lists_800"] >= 800 and longest["big_splats"] > 256 and longest["precomp_small"] > 128
    never = {c: int((inp.reference(c)["walk"]["hits"] == 0).sum()) for c in inp.CASES}
    assert never["big_splats"] > 100            # rows that must stay all-zero
    assert inp.reference("sh3_jitter")["subpix"] is not None
    for c in ("sh3_jitter", "sh1_ragged"):      # a ragged last tile row / column
        f = inp.reference(c)["frame"]
        assert f["H"] % 8 or f["W"] % 8


@pytest.mark.parametrize("case", inp.CASES)
def test_committed_k_covers_a_remeasure(case):
    s, m = inp.measure(case)
    cs, cm, K = inp.K_TABLE[case]
    print(f"{case}: re-measured sum {s:.3g} max {m:.3g} units; committed {cs:g} / {cm:g}, K = {K:g}")
    assert K == gb.choose_k(max(cs, cm))
    assert gb.choose_k(max(s, m)) <= K
    # the bound can see a lost row: every blended Gaussian's sum exceeds its tolerance
    r = inp.reference(case)
    tol_sum, _ = inp.bounds(case)
    blended = r["walk"]["hits"] > 0
    assert (r["osum"][blended] > tol_sum[blended]).mean() > 0.99


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_28_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    for name in ("sfgs_raster_blend_stats", "sfgs_blend_stats_views"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    declared_version = int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1))
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() == 28
    assert C.sizeof(L.SfgsBlendStats) == 32 and L.SfgsBlendStats.weight_sum_q32.offset == 8


def _fake_frame(keep, W=64, H=48):
    buf = (C.c_float * 16)()
    keep.append(buf)
    p = C.cast(buf, C.c_void_p)
    return L.SfgsFrame(C.sizeof(L.SfgsFrame), H, W, 0.5, 0.5, 0.1, 1.0, 0, 0, 0, 0, 0, 0, 0, None, p, p, p, p, 0, None)


def test_every_refusal_comes_before_gpu_work():
    """Pointers are host addresses that no refusal may dereference; this machine has no GPU to launch on."""
    lib = L.load()
    keep = []
    frame = _fake_frame(keep)
    word = (C.c_uint64 * 4)()
    p = C.cast(word, C.c_void_p)
    N = 10
    good = L.SfgsBlendStats(C.sizeof(L.SfgsBlendStats), N, p, p, p)
    big = C.c_size_t(1 << 40)

    def call(frame_=frame, n=N, geom=p, tiles=p, bins=p, bins_sz=big, cap=4096, ccap=256, mask=None, out=good):
        return lib.sfgs_raster_blend_stats(None if frame_ is None else C.byref(frame_), n, geom, tiles, bins, bins_sz, cap, ccap,
                                           mask, None if out is None else C.byref(out), None)

    assert call(frame_=None) == -1
    bad_frame = _fake_frame(keep)
    bad_frame.struct_size = 8
    assert call(frame_=bad_frame) == -1
    assert call(n=-1) == -1
    for kw in (dict(geom=None), dict(tiles=None), dict(bins=None), dict(out=None)):
        assert call(**kw) == -1, kw
        assert b"NULL" in lib.sfgs_last_error()
    assert call(out=L.SfgsBlendStats(4, N, p, p, p)) == -1
    assert b"struct_size" in lib.sfgs_last_error()
    assert call(out=L.SfgsBlendStats(C.sizeof(L.SfgsBlendStats), N + 1, p, p, p)) == -1
    for tables in ((None, p, p), (p, None, p), (p, p, None)):
        assert call(out=L.SfgsBlendStats(C.sizeof(L.SfgsBlendStats), N, *tables)) == -1
    assert call(cap=-1) == -1 and call(cap=1 << 32) == -1 and call(ccap=-1) == -1
    # the blob the render stage needs for (cap, ccap) on this frame: one byte less is refused
    sizes = L.SfgsRasterSizes(C.sizeof(L.SfgsRasterSizes))
    assert lib.sfgs_raster_sizes(N, 64, 48, 4096, 256, C.byref(sizes)) == 0
    assert call(bins_sz=C.c_size_t(1024)) == -3
    assert b"bins blob" in lib.sfgs_last_error()
    # N == 0: nothing to launch
    assert call(n=0, out=L.SfgsBlendStats(C.sizeof(L.SfgsBlendStats), 0, p, p, p)) == 0

    assert lib.sfgs_blend_stats_views(-1, p, p, p, None) == -1
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.sfgs_blend_stats_views(N, *args, None) == -1
    assert lib.sfgs_blend_stats_views(0, p, p, p, None) == 0


# ---- thresholds and pruning ---------------------------------------------------------------------------------------------
def _filled():
    s = importance.BlendStats(5, device="cpu")
    s._max.copy_(torch.tensor([0.0, 0.5, 0.01, 0.2, 0.9]))
    s._sum_q32.copy_((torch.tensor([0.0, 10.0, 0.01, 0.2, 3.0], dtype=torch.float64) * 2.0 ** 32).long())
    s._hits.copy_(torch.tensor([0, 40, 1, 1, 7]))
    s._views.copy_(torch.tensor([0, 3, 1, 1, 2], dtype=torch.int32))
    s.num_views = 3
    return s


def test_tables_and_keep_mask_on_cpu():
    s = importance.BlendStats(4, device="cpu")
    assert s.weight_sum.dtype == torch.float64 and s.weight_max.dtype == torch.float32
    assert s.hits.dtype == torch.int64 and s.views.dtype == torch.int32 and s.num_views == 0
    assert all(int(t.abs().sum()) == 0 and t.shape == (4,) for t in (s.weight_sum, s.weight_max, s.hits, s.views))
    assert s.keep_mask().all()                                   # no criterion: everything stays, blended or not
    s = _filled()
    torch.testing.assert_close(s.weight_sum, torch.tensor([0.0, 10.0, 0.01, 0.2, 3.0], dtype=torch.float64), rtol=0, atol=1e-9)
    assert s.keep_mask().tolist() == [True] * 5
    assert s.keep_mask(min_weight_max=0.2).tolist() == [False, True, False, True, True]
    assert s.keep_mask(min_weight_sum=1.0).tolist() == [False, True, False, False, True]
    assert s.keep_mask(min_hits=2).tolist() == [False, True, False, False, True]
    assert s.keep_mask(min_views=2).tolist() == [False, True, False, False, True]
    assert s.keep_mask(min_weight_max=0.6, min_views=3).tolist() == [False] * 5     # the AND of the criteria
    assert s.keep_mask(min_weight_max=1e-30).tolist() == [False, True, True, True, True]   # never blended: fails any positive one
    s.reset()
    assert s.num_views == 0 and int(s.hits.sum()) == 0 and float(s.weight_max.sum()) == 0 and int(s.views.sum()) == 0
    with pytest.raises(ValueError):
        importance.BlendStats(-1, device="cpu")


class _Model:
    def __init__(self, n):
        self._xyz = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
        self.calls = []

    def prune_points(self, mask):
        self.calls.append(mask.clone())
        self._xyz = self._xyz[~mask]


def test_prune_calls_the_models_own_method():
    s = _filled()
    m = _Model(5)
    assert importance.prune(m, s, min_hits=2) == 3
    assert len(m.calls) == 1 and m.calls[0].tolist() == [True, False, True, True, False]
    assert m._xyz[:, 0].tolist() == [3.0, 12.0]
    with pytest.raises(ValueError, match="2 Gaussians"):        # N changed since the statistics were taken
        importance.prune(m, s, min_hits=2)
    m = _Model(5)
    assert importance.prune(m, s) == 0 and m.calls == []


def test_prune_table_on_structured_arrays():
    rows = np.zeros(5, dtype=[("x", "f4"), ("opacity", "f4"), ("f_dc_0", "f4")])
    rows["x"] = np.arange(5)
    keep = _filled().keep_mask(min_views=2)
    out = importance.prune_table(rows, keep)
    assert out.dtype == rows.dtype and out["x"].tolist() == [1.0, 4.0]
    out["x"][0] = 99                                             # a copy
    assert rows["x"][1] == 1
    assert importance.prune_table(rows, keep.numpy())["x"].tolist() == [1.0, 4.0]
    with pytest.raises(ValueError):
        importance.prune_table(rows, np.ones(4, bool))
    with pytest.raises(ValueError):
        importance.prune_table(rows, np.ones(5, np.int32))


def test_add_needs_the_gpu_and_recording_is_not_reentrant():
    from diff_gauss import GaussianRasterizationSettings, GaussianRasterizer
    from sfgs.synth import scene
    frame, g = scene(8, 32, 32, seed=0)
    settings = GaussianRasterizationSettings(32, 32, frame["tanfovx"], frame["tanfovy"], 0.1, None, frame["bg"], 1.0,
                                             frame["view"], frame["proj"], 0, frame["campos"], False, False)
    s = importance.BlendStats(8, device="cpu")
    kw = dict(means3D=g["means3D"], scales=g["scales"], rotations=g["rotations"], opacities=g["opacities"],
              colors_precomp=g["colors_precomp"])
    with pytest.raises(ValueError, match="GPU"):                 # no CPU path
        s.add(settings, **kw)
    with pytest.raises(ValueError, match="set up for 9"):
        importance.BlendStats(9, device="cpu").add(settings, **kw)
    with pytest.raises(ValueError, match="pixel_mask"):
        s.add(settings, pixel_mask=torch.ones(3, 3, dtype=torch.bool), **kw)
    original = GaussianRasterizer.forward
    with importance.recording(s):
        assert GaussianRasterizer.forward is not original
        with pytest.raises(RuntimeError, match="re-entrant"):
            with importance.recording(s):
                pass
        assert GaussianRasterizer.forward is not original        # the refused one left the open one alone
    assert GaussianRasterizer.forward is original
    with pytest.raises(KeyError):                                # restored after an exception, too
        with importance.recording(s):
            raise KeyError("x")
    assert GaussianRasterizer.forward is original
