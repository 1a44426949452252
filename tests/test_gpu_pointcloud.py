"""GPU tests of sfgs.pointcloud (csrc/pointcloud.hip): depth maps -> one merged point cloud, its colours, bounds and file.
The reference is the numpy restatement tests/geometry_np.unproject (held to the reference's own run by
tests/test_geometry_host.py) and, for the planted 37 x 53 case, the reference's own points in the golden. Nothing here reads
the reference tree.

Bounds. Rows against the restatement: the same bits (assert_array_equal) -- the kernel performs the restatement's float64
operations in its order, nothing contracted. Rows against the reference's own output: 2 ulp, the distance the restatement
itself keeps from it (z column only; measured when the golden was made). Colours, counts, bounds, file contents: exact."""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import geometry_np as gnp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "reference_geometry.npz"))
KERNELS = open(os.path.join(ROOT, "skyfall-gs_amd", "csrc", "pointcloud.hip")).read()
# the kernel file's own constants: pixels per workgroup of the count / scatter kernels, counts per round of the scan's loop
PC_THREADS = int(re.search(r"constexpr int PC_THREADS = (\d+);", KERNELS).group(1))
PC_SCAN_THREADS = int(re.search(r"constexpr int PC_SCAN_THREADS = (\d+);", KERNELS).group(1))
NAN_PATTERN = np.array([0x7ff8dead0000beef], dtype=np.uint64).view(np.float64)[0]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def cam_of(R, T, intr):
    return types.SimpleNamespace(R=R, T=T, focal_x=intr[0], focal_y=intr[1], cx=intr[2], cy=intr[3])


def restate(views, origin=None):
    """views: [(depth, camera, mask)] -> the reference's np.vstack of the per-view clouds"""
    return np.vstack([gnp.unproject(d, c.R, c.T, c.focal_x, c.focal_y, c.cx, c.cy, origin=origin, mask=m) for d, c, m in views])


def build(views, origin=None, capacity=None, colors=False, images=None, wrap=lambda k, d: d):
    """-> PointCloud with every view appended; wrap(k, depth tensor) reshapes view k's depth on its way in"""
    from sfgs.pointcloud import PointCloud
    if capacity is None:
        capacity = max(1, sum(d.size for d, _, _ in views))
    pc = PointCloud(capacity, colors=colors, device=DEV)
    for k, (depth, cam, mask) in enumerate(views):
        pc.add_view(wrap(k, dev(depth)), cam, origin=origin, mask=None if mask is None else dev(mask),
                    image=None if images is None else dev(images[k]))
    return pc


def rows_of(pc):
    points, colors = pc.result()
    assert points.dtype == torch.float64 and points.device == torch.device(DEV) and points.dim() == 2 and points.shape[1] == 3
    return points.cpu().numpy(), None if colors is None else colors.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def within_ulps(got, want, ulps):
    return got.shape == want.shape and bool((np.abs(got - want) <= ulps * np.spacing(np.abs(want))).all())


@functools.lru_cache(maxsize=None)
def golden_city():
    views = tuple((d, cam_of(R, T, i), None) for d, R, T, i in zip(G["city_depths"], G["city_R"], G["city_T"], G["city_intr"]))
    want = restate(views, G["city_origin"])
    want.setflags(write=False)
    return views, G["city_origin"], want


CAM = gnp.look_down_camera(np.array([16.0, 16.0, 12.0]), 64.0, 23.0, 96.0, focal=400.0, cx=0.02, cy=-0.01)


def seeded_depth(H, W, seed):
    """every pixel used: float32 depths around the camera's distance"""
    return np.random.default_rng(seed).uniform(60.0, 130.0, (H, W)).astype(np.float32)


# ---- 1. golden -------------------------------------------------------------------------------------------------------------------
def test_planted_depths_are_bit_equal_to_the_restatement_and_within_2_ulp_of_the_reference():
    from sfgs.pointcloud import depth_to_points
    depth, cam, origin = G["pc_depth"], cam_of(G["pc_R"], G["pc_T"], G["pc_intr"]), G["pc_origin"]
    assert depth.shape == (37, 53) and np.isnan(depth).any() and np.isposinf(depth).any() and np.isneginf(depth).any()
    assert (depth < 0).any() and (depth == 0).any()
    masks = ((None, G["pc_points"], 1853), (G["pc_mask"], G["pc_points_masked"], 1294),
             (G["pc_mask"].astype(np.uint8) * 5, G["pc_points_masked"], 1294))
    for mask, reference, n in masks:
        want = restate([(depth, cam, mask)], origin)
        pc = build([(depth, cam, mask)], origin)
        got, colors = rows_of(pc)
        assert colors is None and len(got) == n == len(reference) == int(pc.num_points)
        np.testing.assert_array_equal(got, want)
        assert same_bits(got + 0.0, want + 0.0)
        assert within_ulps(got, reference, 2)
        np.testing.assert_array_equal(got[:, :2], reference[:, :2])          # the restatement differs from the reference in z only
        one = depth_to_points(dev(depth), cam, origin=origin, mask=None if mask is None else dev(mask))
        assert one.dtype == torch.float64 and tuple(one.shape) == (n, 3)
        np.testing.assert_array_equal(one.cpu().numpy(), want)


# ---- 2. append order and carry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["plain", "leading_axis_on_alternate_views", "non_contiguous"])
def test_three_views_at_utm_magnitude_equal_the_vstack(how):
    views, origin, want = golden_city()
    assert views[0][0].shape == (70, 130) and origin[0] == 4.0e5 and origin[1] == 3.3e6
    if how == "plain":
        pc = build(views, origin)
    elif how == "leading_axis_on_alternate_views":
        pc = build(views, origin, wrap=lambda k, d: d[None] if k % 2 else d)
    else:
        def strided(k, d):
            wide = torch.zeros((d.shape[0], 2 * d.shape[1]), dtype=d.dtype, device=d.device)
            wide[:, ::2] = d
            out = wide[:, ::2]
            assert not out.is_contiguous()
            return out
        pc = build(views, origin, wrap=strided)
    got, _ = rows_of(pc)
    assert len(got) == len(want) == int(G["city_num_points"]) and pc.num_points.dtype == torch.int64 and pc.num_points.is_cuda
    np.testing.assert_array_equal(got, want)


# ---- 3. boundary sizes -----------------------------------------------------------------------------------------------------------
def checkerboard(H, W):
    return (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(bool)


def only(H, W, index):
    m = np.zeros(H * W, dtype=bool)
    m[index] = True
    return m.reshape(H, W)


SCAN_ROUND_SHAPE = (PC_SCAN_THREADS * PC_THREADS // 512 + 1, 512)       # one row more than a round of the scan's loop covers
BOUNDARY_CASES = {
    "1x1_used": (1, 1, None), "1x1_unused": (1, 1, np.zeros((1, 1), dtype=bool)),
    "1x255": (1, PC_THREADS - 1, None), "1x256": (1, PC_THREADS, None), "1x257": (1, PC_THREADS + 1, None), "2x1": (2, 1, None),
    "every_pixel": (37, 53, None), "no_pixel": (37, 53, np.zeros((37, 53), dtype=bool)),
    "first_pixel_only": (37, 53, only(37, 53, 0)), "last_pixel_only": (37, 53, only(37, 53, -1)),
    "checkerboard": (37, 53, checkerboard(37, 53)),
    "half_random": (37, 53, np.random.default_rng(8).random((37, 53)) < 0.5),
    "more_workgroups_than_one_scan_round": SCAN_ROUND_SHAPE + (np.random.default_rng(9).random(SCAN_ROUND_SHAPE) < 0.5,),
}


def test_the_scan_round_shape_follows_the_kernel_constants():
    H, W = SCAN_ROUND_SHAPE
    blocks = -(-H * W // PC_THREADS)
    assert (PC_THREADS, PC_SCAN_THREADS) == (256, 1024) and (H, W) == (513, 512)
    assert PC_SCAN_THREADS < blocks <= 2 * PC_SCAN_THREADS and (H - 1) * W == PC_SCAN_THREADS * PC_THREADS


@pytest.mark.parametrize("case", sorted(BOUNDARY_CASES))
def test_boundary_sizes_equal_the_restatement(case):
    H, W, mask = BOUNDARY_CASES[case]
    depth = seeded_depth(H, W, H * 1000 + W)
    lead, tail = seeded_depth(3, 5, 1), seeded_depth(2, 300, 2)
    # a view before and a view behind: the case starts at a carried row, and the next view starts where the case ended
    views = [(lead, CAM, None), (depth, CAM, mask), (tail, CAM, None)]
    want = restate(views)
    used = H * W if mask is None else int(mask.sum())
    assert len(want) == 15 + used + 600
    pc = build(views[:2], capacity=len(want))
    assert int(pc.num_points) == 15 + used                # no pixel used: nothing appended, the next view starts at the same row
    pc.add_view(dev(tail), CAM)
    got, _ = rows_of(pc)
    np.testing.assert_array_equal(got, want)
    alone, _ = rows_of(build(views[1:2]))
    np.testing.assert_array_equal(alone, want[15:15 + used])
    assert int(pc.reset().num_points) == 0 and rows_of(pc)[0].shape == (0, 3)
    pc.add_view(dev(lead), CAM)
    np.testing.assert_array_equal(rows_of(pc)[0], want[:15])


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------------
def test_exact_fit_passes_and_one_row_too_few_is_reported_not_written():
    views, origin, want = golden_city()
    n = len(want)
    got, _ = rows_of(build(views, origin, capacity=n))
    np.testing.assert_array_equal(got, want)
    pc = build(views, origin, capacity=n - 1)
    assert int(pc.num_points) == n
    with pytest.raises(ValueError, match=rf"\b{n}\b"):
        pc.result()
    assert tuple(pc.points.shape) == (n - 1, 3)
    np.testing.assert_array_equal(pc.points.cpu().numpy(), want[:n - 1])
    small = build(views, origin, capacity=100)              # the buffer ends inside the first view, in the middle of a workgroup's run
    assert int(small.num_points) == n
    np.testing.assert_array_equal(small.points.cpu().numpy(), want[:100])


def test_raw_binding_leaves_the_rows_behind_capacity_untouched():
    from sfgs import _call
    from sfgs import _lib as L
    from sfgs.geometry import _check_view
    views, origin, want = golden_city()
    lib = L.load()
    image = np.random.default_rng(4).random((3, 70, 130)).astype(np.float32)
    for capacity in (len(want) - 1, 1000, 1):
        points = torch.full((capacity + 16, 3), float("nan"), dtype=torch.float64, device=DEV)
        points.view(torch.int64).fill_(int(NAN_PATTERN.view(np.int64)))
        colors = torch.full((capacity + 16, 3), 0xA5, dtype=torch.uint8, device=DEV)
        state = torch.zeros(1, dtype=torch.int64, device=DEV)
        for depth, cam, _ in views:
            d, img = dev(depth), dev(image)
            H, W, numbers = _check_view(torch.device(DEV), d, cam.R, cam.T, cam.focal_x, cam.focal_y, cam.cx, cam.cy, origin, None, centre_from_view=True)
            args = L.SfgsPointCloudViewArgs(L.C.sizeof(L.SfgsPointCloudViewArgs), H, W, d.data_ptr(), None, img.data_ptr(), *numbers)
            scratch = _call.scratch(lib.sfgs_pointcloud_scratch_bytes(H, W), torch.device(DEV), refused_if_zero=True)
            L.check(lib.sfgs_pointcloud_append(L.C.byref(args), L.ptr(points), L.ptr(colors), capacity, L.ptr(state), L.ptr(scratch),
                                               scratch.numel(), _call.stream(torch.device(DEV))))
        torch.cuda.synchronize()
        assert int(state.item()) == len(want)
        np.testing.assert_array_equal(points[:capacity].cpu().numpy(), want[:capacity])
        tail = points[capacity:].cpu().numpy().view(np.uint64)
        assert (tail == NAN_PATTERN.view(np.uint64)).all()
        assert (colors[capacity:].cpu().numpy() == 0xA5).all()


# ---- 5. colours ------------------------------------------------------------------------------------------------------------------
def quantize_np(img):
    """sfgs_frame_quantize's rule in float32 numpy: img * 255 + 0.5, clip, truncate, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        t = img.astype(np.float32) * np.float32(255.0) + np.float32(0.5)
        return np.where(np.isnan(t), np.float32(0.0), np.clip(t, np.float32(0.0), np.float32(255.0))).astype(np.uint8)


def test_colours_equal_the_float32_quantiser_row_for_row():
    views, origin, want = golden_city()
    rng = np.random.default_rng(12)
    images = [rng.uniform(-0.25, 1.25, (3,) + d.shape).astype(np.float32) for d, _, _ in views]
    v, u = np.argwhere(views[1][0] > 0)[7]
    images[1][2, v, u] = np.nan                             # at a used pixel
    images[0][0].reshape(-1)[:300] = np.linspace(0.0, 1.0, 300, dtype=np.float32)
    assert any((im < 0).any() for im in images) and any((im > 1).any() for im in images)
    want_col = np.vstack([quantize_np(im)[:, (d > 0) & np.isfinite(d)].T for im, (d, _, _) in zip(images, views)])
    assert want_col.shape == want.shape and want_col.min() == 0 and want_col.max() == 255 and len(np.unique(want_col)) == 256
    got, col = rows_of(build(views, origin, colors=True, images=images))
    np.testing.assert_array_equal(got, want)
    assert col.dtype == np.uint8
    np.testing.assert_array_equal(col, want_col)
    assert rows_of(build(views, origin))[1] is None
    from sfgs.pointcloud import PointCloud
    with pytest.raises(ValueError, match="image"):
        PointCloud(8, colors=True, device=DEV).add_view(dev(views[0][0]), views[0][1])
    with pytest.raises(ValueError, match="image"):
        PointCloud(8, device=DEV).add_view(dev(views[0][0]), views[0][1], image=dev(images[0]))


# ---- 6. bounds -------------------------------------------------------------------------------------------------------------------
def test_bounds_equal_numpy_min_max_and_an_empty_cloud_gives_infinities():
    from sfgs.pointcloud import PointCloud
    views, origin, want = golden_city()
    pc = build(views, origin)
    b = pc.bounds()
    assert b.dtype == torch.float64 and tuple(b.shape) == (2, 3) and b.device == torch.device(DEV)
    assert same_bits(b.cpu().numpy(), np.stack([want.min(0), want.max(0)]))
    H, W = SCAN_ROUND_SHAPE                                 # more rows than one workgroup of the reduction strides over once
    big = [(seeded_depth(H, W, 5), CAM, None)]
    pts = restate(big)
    assert same_bits(build(big).bounds().cpu().numpy(), np.stack([pts.min(0), pts.max(0)]))
    cut = build(views, origin, capacity=1000)               # over the STORED rows when the buffer was too small
    assert same_bits(cut.bounds().cpu().numpy(), np.stack([want[:1000].min(0), want[:1000].max(0)]))
    empty = PointCloud(64, device=DEV)
    np.testing.assert_array_equal(empty.bounds().cpu().numpy(), [[np.inf] * 3, [-np.inf] * 3])
    np.testing.assert_array_equal(pc.reset().bounds().cpu().numpy(), [[np.inf] * 3, [-np.inf] * 3])


# ---- 7. evaluate_dsm(..., cloud=pc) ----------------------------------------------------------------------------------------------
def test_evaluate_dsm_with_a_cloud_reports_the_same_and_fills_the_cloud():
    from sfgs.geometry import DsmGrid, evaluate_dsm
    from sfgs.pointcloud import PointCloud
    views, origin, want = golden_city()
    grid = DsmGrid.from_metadata(G["city_meta"])
    rng = np.random.default_rng(1)
    gt = np.roll(np.nan_to_num(G["city_dsm"], nan=32.0), (1, -2), axis=(0, 1)) + 0.8 + rng.normal(0, 0.05, G["city_dsm"].shape)
    keep = rng.random(gt.shape) > 0.1
    masks = [None, rng.random(views[1][0].shape) > 0.3, None]
    depths, cams = [dev(d) for d, _, _ in views], [c for _, c, _ in views]
    for view_masks, want_rows in ((None, want), ([None if m is None else dev(m) for m in masks],
                                               restate([(d, c, m) for (d, c, _), m in zip(views, masks)], origin))):
        plain = evaluate_dsm(depths, cams, grid, dev(gt), origin=origin, keep_mask=dev(keep), view_masks=view_masks)
        pc = PointCloud(3 * 70 * 130, device=DEV)
        with_cloud = evaluate_dsm(depths, cams, grid, dev(gt), origin=origin, keep_mask=dev(keep), view_masks=view_masks, cloud=pc)
        assert plain["valid_pixels"] > 1000 and not any(np.isnan(v) for v in plain.values())
        assert with_cloud == plain
        np.testing.assert_array_equal(rows_of(pc)[0], want_rows)
        assert plain["total_points"] <= len(want_rows)      # the DSM counts the points that land in the grid


# ---- 8. determinism --------------------------------------------------------------------------------------------------------------
def test_two_builds_of_the_same_cloud_are_bit_identical():
    views, origin, _ = golden_city()
    images = [np.random.default_rng(k).random((3,) + d.shape).astype(np.float32) for k, (d, _, _) in enumerate(views)]
    a, b = (build(views, origin, colors=True, images=images) for _ in range(2))
    (pa, ca), (pb, cb) = rows_of(a), rows_of(b)
    assert same_bits(pa, pb) and np.array_equal(ca, cb) and int(a.num_points) == int(b.num_points)
    assert torch.equal(a.bounds().view(torch.int64), b.bounds().view(torch.int64))


# ---- 9. save ---------------------------------------------------------------------------------------------------------------------
def test_save_round_trips_through_read_ply(tmp_path):
    from sfgs.ply import read_ply
    views, origin, want = golden_city()
    images = [np.random.default_rng(20 + k).random((3,) + d.shape).astype(np.float32) for k, (d, _, _) in enumerate(views)]
    for colors in (False, True):
        pc = build(views, origin, colors=colors, images=images if colors else None)
        path = str(tmp_path / "sub" / f"cloud_{int(colors)}.ply")
        pc.save(path)
        head = open(path, "rb").read().split(b"end_header\n")[0].decode().splitlines()
        assert head[1] == "format binary_little_endian 1.0" and head[2] == f"element vertex {len(want)}"
        assert head[3:6] == ["property double x", "property double y", "property double z"]
        assert head[6:] == (["property uchar red", "property uchar green", "property uchar blue"] if colors else [])
        (name, table), = read_ply(path)
        assert name == "vertex" and len(table) == len(want)
        assert same_bits(np.stack([table[n] for n in "xyz"], axis=1), want)
        if colors:
            np.testing.assert_array_equal(np.stack([table[n] for n in ("red", "green", "blue")], axis=1), rows_of(pc)[1])
    short = build(views, origin, capacity=10)
    with pytest.raises(ValueError, match="capacity"):
        short.save(str(tmp_path / "short.ply"))
    assert not os.path.exists(tmp_path / "short.ply")
