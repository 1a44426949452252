"""GPU tests of sfgs.consistency (csrc/consistency.hip): depth maps -> multi-view consistency masks. The reference is the numpy
restatement tests/consistency_np.py (held to a scalar spelling and to the figures of its scene by tests/test_consistency_host.py).
Nothing here reads the reference tree.

Bounds. `count` and `keep` equal the restatement EXACTLY (assert_array_equal on the bytes): both sides run the same IEEE float64
sequence, nothing contracted, and every decision is a comparison of those doubles, so there is nothing to tolerate and no pixel
is left out. Where a case is built so that the outcome is known in closed form, that outcome is asserted as well."""
import functools
import types

import numpy as np
import pytest
import torch

import consistency_np as cnp
import geometry_np as gnp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = ((0.01, 1.0, 2), (0.005, 2.0, 1))


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))          # a copy: the shared scenes are read-only
    return (t if dtype is None else t.to(dtype)).to(DEV)


def view_set(views):
    from sfgs.consistency import ViewSet
    return ViewSet([dev(v.depth) for v in views], [v.camera for v in views], [None if v.mask is None else dev(v.mask) for v in views])


def host(pair):
    count, keep = pair
    assert count.device == keep.device == torch.device(DEV) and count.dtype == keep.dtype == torch.uint8
    return count.cpu().numpy(), keep.cpu().numpy()


def check_against_restatement(views, params=PARAMS, refs=None):
    """Every reference view of `refs` (default: all) at every parameter triple -> {(i, triple): count}"""
    vs = view_set(views)
    out = {}
    for i in range(len(views)) if refs is None else refs:
        for triple in params:
            count, keep = host(vs.check(i, *triple))
            want_count, want_keep = cnp.check(views, i, *triple)
            assert count.shape == keep.shape == views[i].depth.shape
            np.testing.assert_array_equal(count, want_count, err_msg=f"count of view {i} at {triple}")
            np.testing.assert_array_equal(keep, want_keep, err_msg=f"keep of view {i} at {triple}")
            out[i, triple] = count
    return out


@functools.lru_cache(maxsize=None)
def reference_scene():
    return tuple(cnp.city(5, 48, 64)[2])


@functools.lru_cache(maxsize=None)
def mixed_scene():
    """The reference scene's terrain and camera ring, the views of different sizes, each with a seeded mask (about 10 % off)"""
    terrain = gnp.make_terrain(64, 64, 3)
    sizes = ((48, 64), (33, 40), (5, 7), (64, 1), (48, 64))
    rng = np.random.default_rng(11)
    views = []
    for k, (H, W) in enumerate(sizes):
        cam = gnp.look_down_camera(np.array([16.0, 16.0, 12.0]), 62.0 + 3.0 * (k % 3), 360.0 * k / len(sizes) + 11.0, 96.0,
                                   focal=2.6 * max(H, W), cx=0.02 * (k % 2), cy=-0.01 * (k % 3))
        views.append(cnp.View(gnp.render_depth(terrain, 0.5, cam, H, W), cam, rng.random((H, W)) > 0.1))
    return tuple(views)


# ---- 1. the shared scenes --------------------------------------------------------------------------------------------------------
def test_reference_scene_every_view_at_both_parameter_sets():
    views = reference_scene()
    counts = check_against_restatement(views)
    hist = sum(np.bincount(counts[i, PARAMS[0]][cnp.used_pixels(views[i].depth, None)], minlength=5) for i in range(5))
    assert hist.tolist() == [2988, 4284, 3178, 2506, 771]                     # the scene reaches every branch (the host test)


def test_views_of_different_sizes_with_input_masks():
    views = mixed_scene()
    assert [v.depth.shape for v in views] == [(48, 64), (33, 40), (5, 7), (64, 1), (48, 64)]
    assert all(0.05 < 1 - v.mask.mean() < 0.2 for v in views[:2])
    counts = check_against_restatement(views)
    for i, v in enumerate(views):
        c = counts[i, PARAMS[1]]
        assert not c[~cnp.used_pixels(v.depth, v.mask)].any()                 # a masked reference pixel has count 0
        assert c.any(), f"view {i} is confirmed nowhere: the case tests nothing"
    # every small view is met as a source: some pixel of a large view is confirmed by more sources than the large views alone
    assert counts[0, PARAMS[1]].max() >= 2
    # bool and uint8 masks, [1,H,W] depths: the same bytes
    from sfgs.consistency import ViewSet
    vs = ViewSet([dev(v.depth)[None] for v in views], [v.camera for v in views], [dev(v.mask, torch.uint8) * 7 for v in views])
    for i in (0, 2, 3):
        np.testing.assert_array_equal(host(vs.check(i, *PARAMS[1]))[0], counts[i, PARAMS[1]])


def test_smallest_set_one_source():
    views = reference_scene()[:2]
    counts = check_against_restatement(views)
    assert all(c.max() == 1 for c in counts.values())
    assert not host(view_set(views).check(0, 0.01, 1.0, 2))[1].any()          # two confirmations cannot come from one source


def test_two_runs_give_the_same_bytes():
    views = mixed_scene()
    a, b = view_set(views), view_set(views)
    for i in range(len(views)):
        first, again, other = (host(vs.check(i, *PARAMS[0])) for vs in (a, a, b))
        for x, y in zip(first, again):
            assert x.tobytes() == y.tobytes()
        for x, y in zip(first, other):
            assert x.tobytes() == y.tobytes()
    for x, y in zip(a.masks(*PARAMS[1]), b.masks(*PARAMS[1])):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ---- 2. cases with a known outcome -----------------------------------------------------------------------------------------------
def plain_camera(tx=0.0, ty=0.0, focal=64.0, cx=0.0, cy=0.0, R=None):
    """World axes = camera axes (or R), the camera at (-tx, -ty, 0): with focal 64 and depths of 64 every number below is exact"""
    return types.SimpleNamespace(R=np.eye(3) if R is None else R, T=np.array([tx, ty, 0.0]), focal_x=focal, focal_y=focal, cx=cx, cy=cy)


def flat(H, W, d=64.0):
    return np.full((H, W), d, dtype=np.float32)


def test_identical_cameras_the_depth_test_is_a_tie_and_one_ulp_beyond():
    cam = types.SimpleNamespace(R=np.eye(3), T=np.zeros(3), focal_x=100.0, focal_y=101.0, cx=0.02, cy=-0.01)
    tie = [cnp.View(flat(9, 11), cam, None), cnp.View(flat(9, 11, 64.5), cam, None)]
    counts = check_against_restatement(tie, params=((2.0 ** -7, 1.0, 1),), refs=(0,))
    assert (counts[0, (2.0 ** -7, 1.0, 1)] == 1).all()                        # |64.5 - 64| == 2^-7 * 64: <= holds
    beyond = [tie[0], cnp.View(flat(9, 11, np.nextafter(np.float32(64.5), np.float32(np.inf))), cam, None)]
    counts = check_against_restatement(beyond, params=((2.0 ** -7, 1.0, 1),), refs=(0,))
    assert not counts[0, (2.0 ** -7, 1.0, 1)].any()


def test_a_source_behind_the_points_confirms_nothing():
    back = plain_camera(R=np.diag([-1.0, 1.0, -1.0]))                         # turned round: every point has z = -64 there
    views = [cnp.View(flat(8, 12), plain_camera(), None), cnp.View(flat(8, 12), back, None)]
    z = cnp.project(cnp.constants(back, 8, 12), cnp.unproject_pixels(cnp.constants(views[0].camera, 8, 12), np.array([3]), np.array([5]),
                                                                     np.array([64.0], dtype=np.float32)))[2]
    assert z[0] == -64.0
    counts = check_against_restatement(views, params=((0.01, np.inf, 1),), refs=(0,))
    assert not counts[0, (0.01, np.inf, 1)].any()
    on_the_plane = plain_camera()                                             # z == 0 exactly is rejected too
    on_the_plane.T = np.array([0.0, 0.0, -64.0])
    views[1] = cnp.View(flat(8, 12), on_the_plane, None)
    assert not check_against_restatement(views, params=((0.01, np.inf, 1),), refs=(0,))[0, (0.01, np.inf, 1)].any()


def test_points_leave_the_source_image_on_each_of_its_four_sides():
    """Reference 12 x 12, source 8 x 8, both looking along +z at the plane z = 64 with focal 64, the source's principal point
    moved so that u = col - 2.5 - 2^-30 and v = row - 2.5 - 2^-30, exactly. Column 2 has u + 0.5 just below 0 (out), column 3
    lands in source column 0, column 10 has u + 0.5 just below W = 8 (source column 7), column 11 is out; rows alike."""
    e = 2.0 ** -30
    src = plain_camera(cx=-(0.5 + e) / 4, cy=-(0.5 + e) / 4)
    ks, kr = cnp.constants(src, 8, 8), cnp.constants(plain_camera(), 12, 12)
    assert ks.cx_pix == ks.cy_pix == 3.5 - e and kr.cx_pix == kr.cy_pix == 6.0
    views = [cnp.View(flat(12, 12), plain_camera(), None), cnp.View(flat(8, 8), src, None)]
    row, col = np.mgrid[0:12, 0:12].reshape(2, -1)
    u, v, z = cnp.project(ks, cnp.unproject_pixels(kr, row, col, np.full(row.size, 64.0, dtype=np.float32)))
    np.testing.assert_array_equal(u, col - 2.5 - e)
    np.testing.assert_array_equal(v, row - 2.5 - e)
    assert (u[col == 2] + 0.5 == -e).all() and (u[col == 10] + 0.5 == 8 - e).all() and (z == 64.0).all()
    counts = check_against_restatement(views, params=((0.01, 1.0, 1),))
    want = np.zeros((12, 12), dtype=np.uint8)
    want[3:11, 3:11] = 1
    np.testing.assert_array_equal(counts[0, (0.01, 1.0, 1)], want)
    assert (counts[1, (0.01, 1.0, 1)] == 1).all()                             # every source pixel is met by one reference pixel


def test_unused_source_pixels_and_unused_reference_pixels():
    cam = plain_camera()
    src = flat(8, 12)
    src[1, 2], src[3, 4], src[5, 6] = 0.0, np.nan, np.inf
    src_mask = np.ones((8, 12), dtype=bool)
    src_mask[6, 9] = False
    ref = flat(8, 12)
    ref[0, 0], ref[7, 11], ref[2, 2] = 0.0, np.nan, -64.0
    ref_mask = np.ones((8, 12), dtype=np.uint8)
    ref_mask[4, 1] = 0
    views = [cnp.View(ref, cam, ref_mask), cnp.View(src, cam, src_mask)]
    counts = check_against_restatement(views, params=((0.01, 1.0, 1),))
    want = np.ones((8, 12), dtype=np.uint8)
    for r, c in ((1, 2), (3, 4), (5, 6), (6, 9), (0, 0), (7, 11), (2, 2), (4, 1)):
        want[r, c] = 0
    np.testing.assert_array_equal(counts[0, (0.01, 1.0, 1)], want)
    np.testing.assert_array_equal(counts[1, (0.01, 1.0, 1)], want)            # the test is symmetric here
    assert not host(view_set(views).check(0, 0.01, 1.0, 1))[1][0, 0]          # unused reference pixel: keep 0 as well


def test_a_wall_in_one_source_is_inconsistent_there_and_consistent_in_another():
    """Three cameras side by side over the plane z = 64 (focal 64: one unit of baseline is one pixel). Source A has a wall at
    depth 40 in front of a block of its pixels; source B sees the ground everywhere."""
    a = flat(10, 16)
    a[3:7, 5:9] = 40.0
    views = [cnp.View(flat(10, 16), plain_camera(), None), cnp.View(a, plain_camera(tx=2.0), None),
             cnp.View(flat(10, 16), plain_camera(tx=-3.0), None)]
    counts = check_against_restatement(views, params=((0.01, 1.0, 2), (0.01, 1.0, 1)))
    c = counts[0, (0.01, 1.0, 2)]
    want = np.zeros((10, 16), dtype=np.uint8)
    want[:, 0:14] += 1                                                        # A sees reference column c at c + 2
    want[:, 3:16] += 1                                                        # B at c - 3
    want[3:7, 3:7] -= 1                                                       # behind A's wall: columns 5 ... 8 of A
    np.testing.assert_array_equal(c, want)
    vs = view_set(views)
    keep2, keep1 = host(vs.check(0, 0.01, 1.0, 2))[1], host(vs.check(0, 0.01, 1.0, 1))[1]
    assert not keep2[3:7, 3:7].any() and keep1[3:7, 3:7].all() and keep2[3:7, 7:14].all()
    # the wall itself, seen from A, is confirmed by nobody: the others see the ground behind it
    assert not counts[1, (0.01, 1.0, 1)][3:7, 5:9].any()


def test_min_views():
    views = reference_scene()
    vs = view_set(views)
    for i in (0, 3):
        count, keep1 = host(vs.check(i, 0.01, 1.0, 1))
        np.testing.assert_array_equal(keep1, count > 0)
        assert 0 < keep1.sum() < keep1.size
        count5, keep5 = host(vs.check(i, 0.01, 1.0, 5))
        np.testing.assert_array_equal(count5, count)
        assert not keep5.any()
        assert not host(vs.check(i, 0.01, 1.0, 10 ** 12))[1].any()
    keeps = vs.masks(0.01, 1.0, 2)
    assert len(keeps) == 5
    for i, k in enumerate(keeps):
        np.testing.assert_array_equal(k.cpu().numpy(), cnp.check(views, i, 0.01, 1.0, 2)[1])


# ---- 3. size ---------------------------------------------------------------------------------------------------------------------
def plate_depth(cam, H, W, plate=(40.0, 110.0, 55.0, 125.0, 30.0)):
    """float32 [H,W] depth of the ground plane up = 0 with one thin raised plate (east0, east1, north0, north1, up) above it, by
    ray-plane intersection: the ray of a pixel is centre + t * dir with dir's forward component 1, so t IS the depth."""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    dirs = np.stack([(u - gnp.pixel_centre(cam.cx, W)) / cam.focal_x, (v - gnp.pixel_centre(cam.cy, H)) / cam.focal_y,
                     np.ones_like(u)], axis=-1) @ cam.axes.T
    e0, e1, n0, n1, up = plate
    t_plate = (up - cam.centre[2]) / dirs[..., 2]
    p = cam.centre + dirs * t_plate[..., None]
    on_plate = (t_plate > 0) & (p[..., 0] >= e0) & (p[..., 0] <= e1) & (p[..., 1] >= n0) & (p[..., 1] <= n1)
    t_ground = -cam.centre[2] / dirs[..., 2]
    return np.where(on_plate, t_plate, np.where(t_ground > 0, t_ground, 0.0)).astype(np.float32)


def test_three_views_of_600_by_700():
    """1672 tiles of 16 x 16 per launch, the last tile row and the last tile column partial (600 = 37.5 tiles, 700 = 43.75)"""
    target = np.array([80.0, 90.0, 10.0])
    cams = [gnp.look_down_camera(target, 58.0 + 5.0 * k, 120.0 * k + 20.0, 400.0, focal=1500.0, cx=0.01 * k, cy=-0.02 * k) for k in range(3)]
    views = [cnp.View(plate_depth(c, 600, 700), c, None) for c in cams]
    assert all(len(np.unique(np.round(v.depth / 20.0))) > 2 for v in views)   # ground and plate are both in the picture
    counts = check_against_restatement(views, params=((0.01, 1.0, 2),))
    for i in range(3):
        c = counts[i, (0.01, 1.0, 2)]
        assert c[-1].any() and c[:, -1].any() and (c == 2).mean() > 0.5 and (c < 2).sum() > 2000      # plate edges hide ground


# ---- 4. wiring -------------------------------------------------------------------------------------------------------------------
def test_evaluate_dsm_with_consistency_equals_evaluate_dsm_with_the_masks():
    from sfgs.consistency import ViewSet
    from sfgs.geometry import DsmGrid, evaluate_dsm
    from sfgs.ortho import OrthoAccumulator
    from sfgs.pointcloud import PointCloud
    grid, terrain, views, origin = cnp.city(5, 48, 64, blurred=True)
    g = DsmGrid(*grid)
    rng = np.random.default_rng(4)
    gt = dev(terrain + origin[2] + rng.normal(0, 0.05, terrain.shape))
    depths, cams = [dev(v.depth) for v in views], [v.camera for v in views]
    images = [dev(rng.random((3, 48, 64)), torch.float32) for _ in views]
    in_masks = [dev(rng.random((48, 64)) > 0.1) for _ in views]
    d = {"rel_tol": 0.01, "px_tol": 1.0, "min_views": 2}
    reports, clouds, orthos = [], [], []
    for how in ("consistency", "view_masks", "unfiltered"):
        cloud, ortho = PointCloud(5 * 48 * 64, colors=False, device=DEV), OrthoAccumulator(g, device=DEV)
        kw = {"consistency": d, "view_masks": in_masks} if how == "consistency" else \
            {"view_masks": ViewSet(depths, cams, in_masks).masks(**d)} if how == "view_masks" else {"view_masks": in_masks}
        reports.append(evaluate_dsm(depths, cams, g, gt, origin=origin, cloud=cloud, ortho=ortho, images=images, **kw))
        clouds.append(cloud)
        orthos.append(ortho)
    assert reports[0] == reports[1] and reports[0]["valid_pixels"] > 1000
    assert reports[0]["total_points"] < reports[2]["total_points"]
    assert clouds[0].result()[0].cpu().numpy().tobytes() == clouds[1].result()[0].cpu().numpy().tobytes()
    assert int(clouds[0].num_points) == int(clouds[1].num_points) < int(clouds[2].num_points)
    assert orthos[0]._acc.cpu().numpy().tobytes() == orthos[1]._acc.cpu().numpy().tobytes()
    assert int(orthos[0].num_points) == int(orthos[1].num_points) == reports[0]["total_points"]
    # the masks it used are the restatement's, the input masks folded in
    np_views = [cnp.View(v.depth, v.camera, m.cpu().numpy()) for v, m in zip(views, in_masks)]
    for i, k in enumerate(ViewSet(depths, cams, in_masks).masks(**d)):
        np.testing.assert_array_equal(k.cpu().numpy(), cnp.check(np_views, i, 0.01, 1.0, 2)[1])


def test_wrong_arguments_raise_value_error():
    from sfgs.consistency import ViewSet
    views = reference_scene()[:3]
    depths, cams = [dev(v.depth) for v in views], [v.camera for v in views]
    for bad_depths, masks in (([depths[0], depths[1].cpu(), depths[2]], None), ([depths[0].cpu(), depths[1], depths[2]], None),
                              (depths, [None, torch.ones(48, 64, dtype=torch.bool), None]), ([d.double() for d in depths], None),
                              (depths, [None, None, dev(np.ones((48, 63), dtype=bool))])):
        with pytest.raises(ValueError):
            ViewSet(bad_depths, cams, masks)
    for n in (1, 257):
        with pytest.raises(ValueError, match="2 ... 256"):
            ViewSet([depths[0]] * n, [cams[0]] * n)
    vs = ViewSet(depths, cams)
    for kw in ({"i": 3}, {"i": -1}, {"rel_tol": 0.0}, {"rel_tol": np.inf}, {"px_tol": np.nan}, {"px_tol": -1.0}, {"min_views": 0}):
        with pytest.raises(ValueError):
            vs.check(**{"i": 0, **kw})
    count_inf, _ = host(vs.check(0, 0.01, np.inf, 1))                        # px_tol = inf: the round-trip bound is off
    count_one, _ = host(vs.check(0, 0.01, 1.0, 1))
    np.testing.assert_array_equal(count_inf, cnp.check(views, 0, 0.01, np.inf, 1)[0])
    assert (count_inf >= count_one).all() and (count_inf > count_one).any()
