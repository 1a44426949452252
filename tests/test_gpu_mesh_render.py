"""GPU tests of Mesh.render (csrc/mesh_raster.hip). The reference is the numpy restatement tests/mesh_render_np.py (held to the host
build of the product's header and to independent spellings by tests/test_mesh_render_host.py). Nothing here reads the reference tree.

Bounds. Every comparison is assert-equal on the BYTES of depth, face, normal and rgb and on the four counts, no pixel left out:
coverage is integer arithmetic, the winner an integer minimum, and depth, weights and attributes are float64 expressions written
once for the device, the host build and numpy -- there is nothing to tolerate.

Routes. A face whose clipped box holds at most small_max pixels is rasterised by its own thread, a larger one by waves over 8 x 8
tiles -- one wave per face up to 64 tiles, 256 waves per face beyond. Every scene runs with _small_max = 0 (every face with a
pixel takes the large route), the default (64: the height field mixes both routes in one frame, tests/test_mesh_render_host.py
guards that) and 2^30 (every face the small route), twice each, and must give the same bytes.
Shapes: 40 x 48, 29 x 37, 70 x 130, 32 x 40, 72 x 96, 20 x 24, 16 x 16 and 9 x 11 -- partial 8-pixel tiles and partial 16-pixel
workgroups of resolve on both axes; 17 338 faces and 8 704 vertices span many workgroups of 256 and are no multiples of it; the
frame-filling quad puts 2 faces over 9 x 17 = 153 tiles each, beyond the 64 of the one-wave route, so its tiles are dealt to 256
waves; the height field and the fan have faces of 2 ... 64 tiles; the fan sends 5 000 faces to one pixel's key."""
import numpy as np
import pytest
import torch

import consistency_np as cnp
import mesh_render_np as mr
import tsdf_np as tnp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = (0, None, 1 << 30)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the shared scenes are read-only


def device_mesh(V, F, Cc=None):
    from sfgs.mesh import Mesh
    return Mesh(dev(np.asarray(V, np.float32)), dev(np.asarray(F, np.int32)), dev(Cc))


def same(t, want, what, dtype=torch.float32):
    if want is None:
        assert t is None, what
        return
    assert t is not None and t.device == torch.device(DEV) and t.dtype == dtype and tuple(t.shape) == want.shape, what
    np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32), err_msg=what)


def same_view(view, ref, what):
    same(view.depth, ref.depth, f"depth, {what}")
    same(view.face, ref.face, f"face, {what}", torch.int32)
    same(view.normal, ref.normal, f"normal, {what}")
    same(view.rgb, ref.rgb, f"rgb, {what}")
    assert view.counts.dtype == torch.int64 and view.counts.device == torch.device(DEV)
    assert view.counts.tolist() == ref.counts.tolist(), f"counts, {what}"
    assert view.check() == tuple(ref.counts.tolist())


def keywords(kw):
    kw = dict(kw)
    if isinstance(kw.get("normals"), np.ndarray):
        kw["normals"] = dev(kw["normals"])
    return kw


# ---- the kernels equal the restatement, by every route, run after run --------------------------------------------------------------
@pytest.mark.parametrize("name", list(mr.scenes()))
def test_every_scene_equals_the_restatement_by_every_route(name):
    V, F, Cc, cam, H, W, kw = mr.scenes()[name]
    ref = mr.rendered(name)
    mesh, kw = device_mesh(V, F, Cc), keywords(kw)
    for small_max in ROUTES:
        for run in (1, 2):
            same_view(mesh.render(cam, H, W, _small_max=small_max, **kw), ref, f"{name}, _small_max {small_max}, run {run}")


def test_the_mesh_of_the_device_pipeline_renders_as_the_restatement():
    """extract -> mesh() -> clean -> render: buffers longer than their counts, sizes read once"""
    from sfgs.tsdf import TsdfVolume
    tsdf, weight, rgb, origin, voxel = mr.mnp.islands_volume(True)
    nz, ny, nx = tsdf.shape
    v = TsdfVolume(origin, (nx, ny, nz), voxel, trunc=1.0, colors=True, device=DEV)
    v.load(dev(tsdf), dev(weight), dev(rgb))
    mesh = v.extract(20000).mesh()
    assert mesh.vertex_buffer.shape[0] > 8704
    same_view(mesh.render(mr.islands_orbit_camera(), 40, 48), mr.rendered("islands, orbit"), "the device's own mesh")
    Vn, Fn, Cn = mr.mnp.clean(*mr.islands_mesh(), min_triangles=64)
    cleaned = mesh.clean(min_triangles=64)
    ref = mr.render(Vn, Fn, Cn, mr.islands_orbit_camera(), 40, 48, cull="back")
    same_view(cleaned.render(mr.islands_orbit_camera(), 40, 48, cull="back"), ref, "the cleaned mesh")
    normals = cleaned.vertex_normals()
    ref = mr.render(Vn, Fn, Cn, mr.islands_orbit_camera(), 40, 48, normals=mr.snp.vertex_normals(Vn, Fn))
    same_view(cleaned.render(mr.islands_orbit_camera(), 40, 48, normals=normals), ref, "the cleaned mesh, its vertex normals")


@pytest.mark.parametrize("cut, whole, far", (("sphere, far through the near cap", "sphere", mr.SPHERE_CAP_FAR),
                                              ("stacked faces, far behind the front face", "stacked faces", 3.5)))
def test_far_empties_the_pixels_behind_it_by_every_route(cut, whole, far):
    """On the device itself: with far inside the visible depths pixels that the uncut view fills come out empty, by each route"""
    V, F, Cc, cam, H, W, _ = mr.scenes()[whole]
    mesh = device_mesh(V, F, Cc)
    full = mesh.render(cam, H, W)
    for small_max in ROUTES:
        view = mesh.render(cam, H, W, far=far, _small_max=small_max)
        gone = (full.depth > 0) & (view.depth == 0)
        assert int(gone.sum()) >= 10 and bool((full.depth[gone] > far).all()) and bool((view.depth <= far).all())
        assert bool((view.face[gone[0]] == -1).all()) and not bool(view.rgb[:, gone[0]].any()) and not bool(view.normal[:, gone[0]].any())
        same_view(view, mr.rendered(cut), f"{cut}, _small_max {small_max}")


def test_a_bad_face_index_is_not_drawn_and_check_reports_it():
    from sfgs.mesh import Mesh
    V, F, Cc, cam, H, W, _ = mr.scenes()["stacked faces"]
    bad = np.array(F)
    bad[2, 1] = len(V)
    mesh = device_mesh(V, F, Cc)
    broken = Mesh._made(mesh.vertex_buffer, dev(bad), mesh.color_buffer, torch.tensor([len(V), len(F), 0, 0], device=DEV), "test")
    ref = mr.render(V, bad, Cc, cam, H, W)
    assert ref.status == mr.ST_BAD_INDEX and ref.counts.tolist() == [3, 0, 1, 0]
    view = broken.render(cam, H, W)
    same(view.depth, ref.depth, "depth"), same(view.face, ref.face, "face", torch.int32), same(view.rgb, ref.rgb, "rgb")
    assert view.counts.tolist() == [3, 0, 1, 0]
    with pytest.raises(ValueError, match="face index"):
        view.check()


# ---- interface -----------------------------------------------------------------------------------------------------------------------
def test_out_keeps_its_pointers_and_every_pixel_is_rewritten():
    V, F, Cc = mr.islands_mesh()
    mesh = device_mesh(V, F, Cc)
    first = mesh.render(mr.islands_orbit_camera(), 40, 48)
    same_view(first, mr.rendered("islands, orbit"), "the first camera")
    pointers = [t.data_ptr() for t in (first.depth, first.face, first.normal, first.rgb, first.counts)]
    cam, H, W = mr.island_camera(0)
    again = mesh.render(cam, H, W, out=first)
    assert again is first and [t.data_ptr() for t in (first.depth, first.face, first.normal, first.rgb, first.counts)] == pointers
    same_view(first, mr.rendered("islands, fused camera 0"), "another camera into the same view")
    for t in (first.depth, first.normal, first.rgb):
        t.fill_(float("nan"))
    first.face.fill_(7)
    same_view(mesh.render(mr.islands_orbit_camera(), 40, 48, out=first), mr.rendered("islands, orbit"), "after garbage")


def test_non_default_stream():
    V, F, Cc, cam, H, W, kw = mr.scenes()["height field"]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(DEV) == side and side.cuda_stream != 0
        mesh = device_mesh(V, F, Cc)
        view = mesh.render(cam, H, W)
        large = mesh.render(cam, H, W, _small_max=0, normals=False)
    side.synchronize()
    same_view(view, mr.rendered("height field"), "side stream")
    same(large.depth, mr.rendered("height field").depth, "side stream, the large route")


def test_wrong_arguments_raise_value_error_and_launch_nothing():
    from sfgs.mesh import MeshView
    V, F, Cc = mr.sphere_mesh()
    mesh, plain, cam = device_mesh(V, F, Cc), device_mesh(V, F), mr.rnp.sphere_camera()
    good = mesh.render(cam, 20, 24)
    tensors = (good.depth, good.face, good.normal, good.rgb, good.counts)
    before = [t.clone() for t in tensors]
    vn = torch.zeros((len(V), 3), device=DEV)
    cpu = MeshView(good.depth.cpu(), good.face, good.normal, good.rgb, good._state)
    for call in (lambda: mesh.render(cam, 0, 24), lambda: mesh.render(cam, 20, -3), lambda: mesh.render(cam, 1 << 16, 1 << 15),
                 lambda: mesh.render(cam, 20, 24, near=2.0, far=2.0), lambda: mesh.render(cam, 20, 24, near=3.0, far=1.0),
                 lambda: mesh.render(cam, 20, 24, near=-1.0), lambda: mesh.render(cam, 20, 24, cull="front"),
                 lambda: mesh.render(cam, 20, 24, normals=vn[:, :2]), lambda: mesh.render(cam, 20, 24, normals=vn[:-1], out=good),
                 lambda: mesh.render(cam, 20, 24, normals=vn.double()), lambda: mesh.render(cam, 20, 24, normals=vn.cpu(), out=good),
                 lambda: mesh.render(cam, 20, 25, out=good), lambda: plain.render(cam, 20, 24, out=good),
                 lambda: mesh.render(cam, 20, 24, normals=False, out=good), lambda: mesh.render(cam, 20, 24, out=cpu),
                 lambda: mesh.render(object(), 20, 24, out=good), lambda: mesh.render(cam, 20, 24, out=good, _small_max=-1)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    for t, b in zip(tensors, before):
        assert torch.equal(t, b)                                             # nothing was launched into the view
    # list overflow cannot be forced: the large route's list holds one entry per face and a face is appended at most once
    # (csrc/mesh_raster.hip), so there is no capacity to make small; check() of a full large-route run reports no status
    assert mesh.render(cam, 20, 24, _small_max=0).check() == tuple(mr.rendered("sphere").counts.tolist())


# ---- composition -----------------------------------------------------------------------------------------------------------------------
def test_a_rendered_depth_goes_into_a_fresh_volume():
    from sfgs.tsdf import TsdfVolume
    V, F, Cc = mr.islands_mesh()
    cam = mr.islands_orbit_camera()
    view = device_mesh(V, F, Cc).render(cam, 40, 48)
    vol = tnp.Volume(origin=(0.0, 0.0, 0.0), dims=mr.mnp.ISLAND_DIMS, voxel_size=0.5, trunc=1.5, max_weight=2.0)
    fresh = TsdfVolume(vol.origin, vol.dims, vol.voxel_size, vol.trunc, max_weight=vol.max_weight, colors=True, device=DEV)
    fresh.add_view(view.depth, cam, image=view.rgb)
    assert int((fresh.weight > 0).sum()) > 500                                # the empty pixels are zeros: unused, as everywhere
    state = tnp.empty_state(vol.dims, True)
    tnp.integrate(state, vol, [cnp.View(view.depth[0].cpu().numpy(), cam, None)], [view.rgb.cpu().numpy()])
    same(fresh.tsdf, state.tsdf, "tsdf of the rendered view")
    same(fresh.weight, state.weight, "weight of the rendered view")
    same(fresh.rgb, state.rgb, "rgb of the rendered view")
