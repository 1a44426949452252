"""GPU tests of TsdfVolume.raycast and ray_skip (csrc/tsdf.hip: tsdf_raycast_kernel, tsdf_skip_kernel). The reference is the numpy
restatement tests/tsdf_raycast_np.py, which has the uniform march only (held to the host build of the product's header, to the
analytic sphere and to the fused depth maps by tests/test_tsdf_raycast_host.py). Nothing here reads the reference tree.

Bounds. Every comparison is assert-equal on the BYTES, with skip=False, skip=None and a prebuilt table alike: both sides run the
same IEEE float64 sequence on the same float32 values, nothing contracted, every decision is a comparison of those numbers, and
the one sqrt and the divisions are correctly rounded on both sides. No pixel is left out."""
import functools

import numpy as np
import pytest
import torch

import consistency_np as cnp
import tsdf_np as tnp
import tsdf_raycast_np as rnp
from tsdf_raycast_np import BRANCH_SCENES, WAVY, branch_scenes, volume_of, wavy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the shared scenes are read-only


def loaded(case):
    from sfgs.tsdf import TsdfVolume
    tsdf, weight, rgb, origin, voxel = case
    nz, ny, nx = tsdf.shape
    v = TsdfVolume(origin, (nx, ny, nz), voxel, trunc=1.0, colors=rgb is not None, device=DEV)
    return v.load(dev(tsdf), dev(weight), None if rgb is None else dev(rgb))


def same(t, want, what):
    if want is None:
        assert t is None, what
        return
    assert t.device == torch.device(DEV) and t.dtype == torch.float32 and tuple(t.shape) == want.shape, what
    np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32), err_msg=what)


def same_view(view, ref, what):
    same(view.depth, ref.depth, f"depth, {what}")
    same(view.normal, ref.normal, f"normal, {what}")
    same(view.rgb, ref.rgb, f"rgb, {what}")


def three_ways(case, cam, H, W, what, **kw):
    """skip=False, skip=None and a prebuilt table against the restatement -> (the restatement, the volume)"""
    ref = rnp.raycast(*case, cam, H, W, **kw)
    v = loaded(case)
    table = v.ray_skip()
    same_view(v.raycast(cam, H, W, skip=False, **kw), ref, f"{what}, skip=False")
    same_view(v.raycast(cam, H, W, **kw), ref, f"{what}, skip=None")
    same_view(v.raycast(cam, H, W, skip=table, **kw), ref, f"{what}, a prebuilt table")
    return ref, v


@functools.lru_cache(maxsize=None)
def fusion():
    vol, views, images, state = rnp.fused_volume()
    return volume_of(state, vol), views, images, vol


# ---- the kernel equals the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view, hits", ((0, 840), (2, 617), (3, 1920)))
def test_fused_volume_equals_the_restatement(view, hits):
    case, views, _, vol = fusion()
    assert vol.dims == (24, 20, 16)                                           # 23 x 19 x 15 cells: partial bricks on every axis
    H, W = views[view].depth.shape
    assert (H, W) == ((29, 37) if view == 2 else (40, 48))                    # 37 x 29: no multiple of the 8 x 8 wave, one partial tile row
    ref, _ = three_ways(case, views[view].camera, H, W, f"fusion scene from camera {view}")
    assert ref.hits == hits


def test_sphere_through_load_with_colours():
    ref, _ = three_ways(tnp.sphere_volume(colors=True), rnp.sphere_camera(), 20, 24, "sphere")
    assert ref.hits == 74 and ref.rgb is not None


def test_wavy_volume_where_runs_span_several_bricks():
    ref, v = three_ways(wavy(), rnp.wavy_top_camera(WAVY), 40, 48, "wavy from above")
    assert ref.hits == 896
    plain = loaded(wavy()[:2] + (None,) + wavy()[3:])                         # ... and without colours
    view = plain.raycast(rnp.wavy_top_camera(WAVY), 40, 48)
    assert view.rgb is None
    same(view.depth, ref.depth, "depth, no colours")
    same(view.normal, ref.normal, "normal, no colours")


def test_skip_tables_equal_the_numpy_table():
    from sfgs.tsdf import RaySkip
    for case, shape in ((fusion()[0], (2, 3, 3)), (wavy(), (8, 8, 9)), (tnp.sphere_volume(), (2, 2, 2))):
        table = loaded(case[:2] + (None,) + case[3:]).ray_skip()
        want = rnp.skip_table(case[0], case[1])
        assert isinstance(table, RaySkip) and table.table.dtype == torch.uint8 and tuple(table.table.shape) == shape == want.shape
        np.testing.assert_array_equal(table.table.cpu().numpy(), want)
    rng = np.random.default_rng(7)
    for nx, ny, nz in ((2, 9, 10), (10, 2, 17), (18, 11, 2), (26, 17, 10)):   # an axis of 2 voxels: one cell, one brick
        tsdf = np.where(rng.random((nz, ny, nx)) < 0.01, -0.5, 0.5).astype(np.float32)
        weight = (rng.random((nz, ny, nx)) < 0.7).astype(np.float32)
        table = loaded((tsdf, weight, None, (0.0, 0.0, 0.0), 1.0)).ray_skip()
        np.testing.assert_array_equal(table.table.cpu().numpy(), rnp.skip_table(tsdf, weight))


@pytest.mark.parametrize("name", BRANCH_SCENES)
def test_branch(name):
    case, cam, H, W, kw, counts = branch_scenes()[name]
    ref, _ = three_ways(case, cam, H, W, name, **kw)
    assert {n: rnp.count(ref.code, n) for n in counts} == counts, name


# ---- the interface -----------------------------------------------------------------------------------------------------------------
def test_normals_false_and_out():
    case, views, _, _ = fusion()
    cam = views[0].camera
    ref = rnp.raycast(*case, cam, 40, 48)
    v = loaded(case)
    bare = v.raycast(cam, 40, 48, normals=False)
    assert bare.normal is None
    same(bare.depth, ref.depth, "depth, normals=False")
    same(bare.rgb, ref.rgb, "rgb, normals=False")
    first = v.raycast(views[3].camera, 40, 48)                                 # another camera first: every pixel is written again
    pointers = [t.data_ptr() for t in (first.depth, first.normal, first.rgb)]
    again = v.raycast(cam, 40, 48, out=first)
    assert again is first and [t.data_ptr() for t in (first.depth, first.normal, first.rgb)] == pointers
    same_view(first, ref, "out=")
    # a stale table is the caller's: after a reset the volume has no surface, with a fresh table or none
    v.reset()
    assert not v.raycast(cam, 40, 48).depth.any() and not v.raycast(cam, 40, 48, skip=False, out=first).depth.any()


def test_non_default_stream():
    case, views, _, _ = fusion()
    ref = rnp.raycast(*case, views[2].camera, 29, 37)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(DEV) == side and side.cuda_stream != 0
        v = loaded(case)
        view = v.raycast(views[2].camera, 29, 37)
        kept = v.raycast(views[2].camera, 29, 37, skip=v.ray_skip(), normals=False)
    side.synchronize()
    same_view(view, ref, "side stream")
    same(kept.depth, ref.depth, "side stream, a prebuilt table")


def test_a_raycast_depth_goes_back_into_a_fresh_volume():
    from sfgs.tsdf import TsdfVolume
    case, views, _, vol = fusion()
    cam = views[0].camera
    view = loaded(case).raycast(cam, 40, 48)
    fresh = TsdfVolume(vol.origin, vol.dims, vol.voxel_size, vol.trunc, max_weight=vol.max_weight, colors=True, device=DEV)
    fresh.add_view(view.depth, cam, image=view.rgb)
    assert int((fresh.weight > 0).sum()) > 500                                # the misses are zeros: unused pixels, as everywhere
    # ... and by the restatement of the fusion: the two compose to the byte
    state = tnp.empty_state(vol.dims, True)
    tnp.integrate(state, vol, [cnp.View(view.depth[0].cpu().numpy(), cam, None)], [view.rgb.cpu().numpy()])
    same(fresh.tsdf, state.tsdf, "tsdf of the ray-cast view")
    same(fresh.weight, state.weight, "weight of the ray-cast view")
    assert int((fresh.raycast(cam, 40, 48).depth > 0).sum()) > 500            # ... and the new volume shows a surface again


def test_wrong_arguments_raise_value_error():
    from sfgs.tsdf import RaySkip, RayView
    case, views, _, _ = fusion()
    cam = views[0].camera
    v, plain = loaded(case), loaded(case[:2] + (None,) + case[3:])
    good = v.raycast(cam, 40, 48)
    before = [t.clone() for t in (good.depth, good.normal, good.rgb)]
    other = loaded(tnp.sphere_volume(True)).ray_skip()
    for call in (lambda: v.raycast(cam, 0, 48), lambda: v.raycast(cam, 40, 48, step=0.0), lambda: v.raycast(cam, 40, 48, step=float("nan")),
                 lambda: v.raycast(cam, 40, 48, near=-1.0), lambda: v.raycast(cam, 40, 48, near=2.0, far=2.0),
                 lambda: v.raycast(cam, 40, 48, step=1e-7), lambda: v.raycast(cam, 40, 48, skip=other),
                 lambda: v.raycast(cam, 40, 48, skip=RaySkip(v.ray_skip().table.cpu(), v.dims)),
                 lambda: v.raycast(cam, 40, 49, out=good), lambda: plain.raycast(cam, 40, 48, out=good),
                 lambda: v.raycast(cam, 40, 48, normals=False, out=good),
                 lambda: v.raycast(cam, 40, 48, out=RayView(good.depth.cpu(), good.normal, good.rgb)),
                 lambda: v.raycast(cam, 40, 48, out=RayView(good.depth, good.normal.cpu(), good.rgb))):
        with pytest.raises(ValueError):
            call()
    assert all(torch.equal(a, b) for a, b in zip(before, (good.depth, good.normal, good.rgb)))      # nothing was launched
