"""GPU tests of sfgs.tsdf (csrc/tsdf.hip): depth views -> TSDF volume -> triangle soup. The reference is the numpy restatement
tests/tsdf_np.py (held to its mesh properties and to the host build of the product's header by tests/test_tsdf_host.py).
Nothing here reads the reference tree.

Bounds. Every comparison is assert-equal on the BYTES: integration runs the same IEEE float64 sequence on both sides and
extraction the same float32 sequence, nothing contracted, and every decision is a comparison of those numbers, so there is
nothing to tolerate and no voxel, row or count is left out."""
import functools

import numpy as np
import pytest
import torch

import tsdf_np as tnp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))          # a copy: the shared scenes are read-only
    return (t if dtype is None else t.to(dtype)).to(DEV)


def same(t, want, what):
    assert t.device == torch.device(DEV) and t.dtype == torch.float32, what
    got = t.cpu().numpy()
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32), err_msg=what)


@functools.lru_cache(maxsize=None)
def fused(colors):
    """The fusion scene through the restatement, once -> (vol, views, images, state, counters)"""
    vol, views, images = tnp.fusion_scene()
    state, counters = tnp.empty_state(vol.dims, colors), {}
    tnp.integrate(state, vol, views, images if colors else None, counters)
    for a in (state.tsdf, state.weight, state.rgb):
        if a is not None:
            a.setflags(write=False)
    return vol, views, images, state, counters


def volume(vol, colors=False, **kw):
    from sfgs.tsdf import TsdfVolume
    return TsdfVolume(vol.origin, vol.dims, vol.voxel_size, vol.trunc, max_weight=vol.max_weight, colors=colors, device=DEV, **kw)


def add(v, views, images, which):
    v.add_views([dev(views[k].depth) for k in which], [views[k].camera for k in which],
                [None if views[k].mask is None else dev(views[k].mask) for k in which],
                None if images is None else [dev(images[k]) for k in which])


def check_state(v, state, what):
    same(v.tsdf, state.tsdf, f"tsdf, {what}")
    same(v.weight, state.weight, f"weight, {what}")
    if state.rgb is not None:
        same(v.rgb, state.rgb, f"rgb, {what}")
    else:
        assert v.rgb is None


def check_soup(soup, verts, cols, what):
    assert soup.num_triangles.device == torch.device(DEV) and soup.num_triangles.dtype == torch.int64 and soup.num_triangles.dim() == 0
    assert int(soup.num_triangles) == len(verts), what
    same(soup.vertices, verts, f"vertices, {what}")
    if cols is None:
        assert soup.colors is None
    else:
        same(soup.colors, cols, f"colors, {what}")


# ---- 1. integration ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colors", (False, True))
def test_fusion_scene_equals_the_restatement(colors):
    vol, views, images, state, counters = fused(colors)
    assert vol.dims == (24, 20, 16) and [v.depth.shape for v in views] == [(40, 48), (40, 48), (29, 37), (40, 48), (40, 48)]
    print(counters)
    assert all(counters[name] >= 200 for name in tnp.OUTCOMES), counters       # on the restatement's own counters
    v = volume(vol, colors)
    add(v, views, images if colors else None, range(5))
    check_state(v, state, "five views in one call")
    assert (state.weight == 0).any() and state.weight.max() == vol.max_weight


@pytest.mark.parametrize("colors", (False, True))
def test_any_split_of_the_view_list_gives_the_same_bytes(colors):
    vol, views, images, state, _ = fused(colors)
    images = images if colors else None
    one_by_one, split = volume(vol, colors), volume(vol, colors)
    for k in range(5):
        one_by_one.add_view(dev(views[k].depth)[None], views[k].camera, mask=None if views[k].mask is None else dev(views[k].mask, torch.uint8) * 9,
                            image=None if images is None else dev(images[k]))
    check_state(one_by_one, state, "five calls of one view, [1,H,W] depths, uint8 mask")
    add(split, views, images, (0, 1))
    add(split, views, images, (2, 3, 4))
    check_state(split, state, "2 + 3")
    # the order of the views is what a voxel depends on: another order gives other bits somewhere
    other = volume(vol, colors)
    add(other, views, images, (4, 3, 2, 1, 0))
    assert not torch.equal(other.tsdf, split.tsdf)


def test_reset_load_and_a_second_extract_after_more_views():
    vol, views, _, state, _ = fused(False)
    v = volume(vol)
    add(v, views, None, (0, 1))
    part = tnp.empty_state(vol.dims)
    tnp.integrate(part, vol, views[:2])
    check_state(v, part, "two views")
    first = v.extract(20000)
    check_soup(first, *tnp.extract(part.tsdf, part.weight, vol.origin, vol.voxel_size), "after two views")
    add(v, views, None, (2, 3, 4))
    check_state(v, state, "the rest")
    second = v.extract(20000)
    check_soup(second, *tnp.extract(state.tsdf, state.weight, vol.origin, vol.voxel_size), "after five views")
    assert int(first.num_triangles) != int(second.num_triangles)             # the first soup kept its own count and rows
    assert v.reset() is v and not v.tsdf.any() and not v.weight.any()
    assert int(v.extract(16).num_triangles) == 0                              # nothing observed: no cell is used
    add(v, views, None, range(5))
    check_state(v, state, "after reset")
    v.load(dev(part.tsdf), dev(part.weight))
    check_state(v, part, "load")


def test_non_default_stream():
    vol, views, images, state, _ = fused(True)
    verts, cols = tnp.extract(state.tsdf, state.weight, vol.origin, vol.voxel_size, state.rgb)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(DEV) == side and side.cuda_stream != 0
        v = volume(vol, True)
        add(v, views, images, range(5))
        soup = v.extract(len(verts))
    side.synchronize()
    check_state(v, state, "side stream")
    check_soup(soup, verts, cols, "side stream")


# ---- 2. extraction -----------------------------------------------------------------------------------------------------------------
def loaded(tsdf, weight, rgb, origin, voxel):
    from sfgs.tsdf import TsdfVolume
    nz, ny, nx = tsdf.shape
    v = TsdfVolume(origin, (nx, ny, nz), voxel, trunc=1.0, colors=rgb is not None, device=DEV)
    return v.load(dev(tsdf), dev(weight), None if rgb is None else dev(rgb))


@pytest.mark.parametrize("colors", (False, True))
def test_sphere_through_load(colors):
    case = tnp.sphere_volume(colors)
    verts, cols = tnp.extract(case[0], case[1], case[3], case[4], case[2])
    assert len(verts) == 2012
    soup = loaded(*case).extract(2012)                                        # capacity == count: the last row is written
    check_soup(soup, verts, cols, "sphere")
    V, F = soup.weld()
    wantV, wantF = tnp.weld(verts)
    assert V.tobytes() == wantV.tobytes() and (F == wantF).all() and len(V) == 1008


def test_fused_volume_is_an_open_mesh_with_interpolated_colours():
    vol, _, _, state, _ = fused(True)
    verts, cols = tnp.extract(state.tsdf, state.weight, vol.origin, vol.voxel_size, state.rgb)
    r = tnp.mesh_report(verts)
    assert len(verts) > 1000 and set(r.undirected.tolist()) == {1, 2} and np.ptp(cols) > 0.5
    v = volume(vol, True).load(dev(state.tsdf), dev(state.weight), dev(state.rgb))
    check_soup(v.extract(len(verts) + 100), verts, cols, "fused volume")


@functools.lru_cache(maxsize=None)
def wavy():
    case = tnp.wavy_volume((72, 64, 64), colors=True)
    return case, tnp.extract(case[0], case[1], case[3], case[4], case[2])


def test_wavy_height_field_scan_takes_a_second_round():
    case, (verts, cols) = wavy()
    assert (72 - 1) * (64 - 1) * (64 - 1) > 1024 * 256                        # more than 1024 workgroups of 256 cells: a carry
    assert len(verts) > 50000 and set(tnp.mesh_report(verts).undirected.tolist()) == {1, 2}     # open at the unobserved block
    # triangles on both sides of the scan's round boundary (cell 1024 * 256 lies in layer z = 58)
    assert (verts[:, :, 2].min(axis=1) < case[3][2] + 58 * case[4]).any() and (verts[:, :, 2].max(axis=1) > case[3][2] + 59.5 * case[4]).any()
    check_soup(loaded(*case).extract(len(verts) + 7), verts, cols, "wavy")
    check_soup(loaded(case[0], case[1], None, case[3], case[4]).extract(len(verts)), verts, None, "wavy, no colours")


def test_no_crossing_gives_no_triangles():
    tsdf = np.full((9, 10, 11), 0.75, np.float32)
    tsdf[4, 5, 6] = 0.0                                                       # exactly 0 is outside
    soup = loaded(tsdf, np.ones_like(tsdf), None, (0.0, 0.0, 0.0), 1.0).extract(8)
    assert int(soup.num_triangles) == 0 and tuple(soup.vertices.shape) == (0, 3, 3)
    flat = np.full((1, 10, 11), -1.0, np.float32)                             # one voxel thick: no cell at all
    flat[0, :, 5:] = 1.0
    assert int(loaded(flat, np.ones_like(flat), None, (0.0, 0.0, 0.0), 1.0).extract(8).num_triangles) == 0


def test_capacity_below_the_count():
    case, (verts, cols) = wavy()
    capacity = 40001                                                          # odd: it ends inside some workgroup's run
    v = loaded(*case)
    from sfgs import _call
    from sfgs import _lib as L
    canary = 4096
    vbuf = torch.full((capacity + canary, 3, 3), -7.0, dtype=torch.float32, device=DEV)
    cbuf = torch.full((capacity + canary, 3, 3), -7.0, dtype=torch.float32, device=DEV)
    state = torch.zeros(1, dtype=torch.int64, device=DEV)
    lib = L.load()
    scratch = _call.scratch(lib.sfgs_tsdf_scratch_bytes(*v.dims), v.device, refused_if_zero=True)
    vol = v._struct()
    L.check(lib.sfgs_tsdf_extract(L.C.byref(vol), L.ptr(vbuf), L.ptr(cbuf), capacity, L.ptr(state), L.ptr(scratch), scratch.numel(),
                                  _call.stream(v.device)))
    assert int(state.item()) == len(verts) > capacity                         # the count is the full one
    same(vbuf[:capacity], verts[:capacity], "rows below the capacity")
    same(cbuf[:capacity], cols[:capacity], "colour rows below the capacity")
    assert bool((vbuf[capacity:] == -7.0).all()) and bool((cbuf[capacity:] == -7.0).all())     # nothing at or beyond it
    soup = v.extract(capacity)
    assert int(soup.num_triangles) == len(verts)
    with pytest.raises(ValueError, match=f"capacity of {len(verts)} would have sufficed"):
        soup.vertices
    same(soup.buffer, verts[:capacity], "the buffer of a soup that was too small")


def test_wrong_arguments_raise_value_error():
    vol, views, images, _, _ = fused(True)
    plain, coloured = volume(vol), volume(vol, True)
    d, cam, img = dev(views[0].depth), views[0].camera, dev(images[0])
    for call in (lambda: plain.add_views([d], [cam], images=[img]), lambda: coloured.add_views([d], [cam]),
                 lambda: plain.add_views([d] * 257, [cam] * 257), lambda: plain.add_views([d, d], [cam]),
                 lambda: plain.add_views([d.cpu()], [cam]), lambda: plain.add_views([d.double()], [cam]),
                 lambda: plain.add_views([d], [cam], masks=[torch.ones(40, 48, dtype=torch.bool)]),
                 lambda: coloured.add_views([d], [cam], images=[img.cpu()]), lambda: coloured.add_views([d], [cam], images=[img[:, :-1]]),
                 lambda: plain.extract(0), lambda: plain.load(plain.tsdf, plain.weight, coloured.rgb),
                 lambda: coloured.load(plain.tsdf, plain.weight)):
        with pytest.raises(ValueError):
            call()
    assert not plain.weight.any() and not coloured.weight.any()              # nothing was launched
