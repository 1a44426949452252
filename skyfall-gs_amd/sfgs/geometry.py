"""sfgs.geometry -- the reference's geometry evaluation (evaluate_gs_geometry.py with dsmr.py) on HIP kernels
(csrc/geometry.hip through libsfgs.so): depth maps -> digital surface model (DSM) -> registration against the lidar DSM ->
altitude MAE / RMSE / completeness, with one host read at the end.

    acc = DsmAccumulator(DsmGrid.from_metadata(np.loadtxt("JAX_068_DSM.txt")), mode="max", device="cuda")
    for cam in cameras:                                   # the DSM needs no point cloud in between; the merged cloud the
        acc.add_view(render(cam)["render_depth"], cam, origin=(utm_x, utm_y, alt))   # script also saves: sfgs.pointcloud
    shift = register(gt_dsm, acc.result())                # dsmr.compute_shift(gt, pred, scaling=False) on the device
    m = dsm_metrics(acc.result(), gt_dsm, shift=shift, mask=cls != 9)
    report = evaluate_dsm(depths, cameras, grid, gt_dsm, origin=...)     # the three stages chained, Python numbers out

Where this differs from the reference (each on purpose, each tested):
  * a depth of +inf is NOT used (the reference's `depth > 0` accepts it; its caller scrubs +inf to 0 before the call);
  * a shift at which the reference divides by zero -- no overlapping finite pair, or sigma_u * sigma_v == 0 -- is skipped;
  * when every shift is skipped, (dx, dy) stay at their start and b (and a with scaling) is NaN;
  * float32 rasters are widened to float64 before any sum (what numba's typing does to the reference's accumulators).
mode="mean" is the flattening the reference gets from plyflatten(radius, sigma=inf) when that package is installed. Its cell
rule is UNPINNED (the package was not available): here every point adds its height to all cells within `radius` columns and
rows of its own cell, a point whose own cell is outside the grid is dropped, cell = sum / count. tests/geometry_np.py states it.

There is no torch fallback: without the HIP library every operator raises. There is no install(): the reference's script
passes GeoTIFF files between its stages, so there is no single name to rebind (INTEGRATION.md shows the edited call site)."""
import collections

import numpy as np
import torch

from . import _call
from . import _lib as L

__all__ = ["DsmGrid", "DsmAccumulator", "DsmShift", "register", "apply_shift", "dsm_metrics", "register_simple", "evaluate_dsm"]

_MODES = {"max": L.DSM_MAX, "mean": L.DSM_MEAN}
FIXED_POINT_UNIT = 2.0 ** -20      # metres per unit of the mean mode's int64 sums


class DsmGrid(collections.namedtuple("DsmGrid", "xoff yoff_top xsize ysize resolution")):
    """Cell (row gy, column gx) holds the points with gx = int((east - xoff) / resolution) and
    gy = int((yoff_top - north) / resolution)."""
    __slots__ = ()

    def __new__(cls, xoff, yoff_top, xsize, ysize, resolution):
        if int(xsize) != xsize or int(ysize) != ysize or xsize < 1 or ysize < 1:
            raise ValueError(f"DsmGrid: xsize, ysize must be positive integers, got {xsize!r}, {ysize!r}")
        if not (float(resolution) > 0 and np.isfinite(resolution) and np.isfinite(xoff) and np.isfinite(yoff_top)):
            raise ValueError(f"DsmGrid: needs finite offsets and resolution > 0, got {xoff!r}, {yoff_top!r}, {resolution!r}")
        if int(xsize) * int(ysize) > 1 << 28:
            raise ValueError(f"DsmGrid: xsize * ysize must not exceed 2^28, got {xsize} x {ysize}")
        return super().__new__(cls, float(xoff), float(yoff_top), int(xsize), int(ysize), float(resolution))

    @classmethod
    def from_metadata(cls, m, resolution=None):
        """The reference's reading of a `*_DSM.txt` 4-vector (xoff, yoff, size, resolution), evaluate_gs_geometry.py:236-240 and
        :279-283: the grid is SQUARE (ysize = xsize = int(m[2])), and yoff moves up by ysize * resolution."""
        m = np.asarray(m, dtype=np.float64).reshape(-1)
        if m.size != 4:
            raise ValueError(f"DsmGrid.from_metadata: 4 numbers expected, got {m.size}")
        size = int(m[2])
        res = np.float64(m[3] if resolution is None else resolution)
        return cls(m[0], m[1] + size * res, size, size, res)


def _check_raster(t, name):
    _call.check_tensor(name, t, "a non-empty [H,W]", lambda t: t.dim() == 2 and t.numel() > 0,
                       dtypes=(torch.float32, torch.float64))
    if max(t.shape) > 32768:
        raise ValueError(f"{name}: H and W must not exceed 32768, got {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[1])


def _f64(t):
    return t.detach().to(torch.float64).contiguous()     # float32 -> float64 is exact


def _u8(mask):
    return None if mask is None else mask.detach().contiguous()


def _vec(x, n, name):
    a = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(-1)
    if a.size != n or not np.isfinite(a).all():
        raise ValueError(f"{name}: {n} finite numbers expected, got {x!r}")
    return a


def _check_view(device, depth, R, T, focal_x, focal_y, cx, cy, origin, mask, centre_from_view=False, **more_on_device):
    """The checks of one view (DsmAccumulator.add_depth, PointCloud.add_depth), host checks first, and the camera as the
    library takes it -> (H, W, (M[9], c[3], origin[3], cx_pix, cy_pix, focal_x, focal_y)); all numbers formed in float64.
    centre_from_view: form c = -(M T) from the transposed VIEW of R, as tests/geometry_np.unproject does, instead of from a
    contiguous copy. The last bit of numpy's matrix product depends on the operand's memory order (1 ulp of c, measured);
    the DSM keeps the copy it always used, the point cloud -- held to that restatement bit for bit -- the view."""
    H, W = _call.check_depth_map(depth)
    _call.check_pixel_mask(mask, H, W)
    R = _vec(R, 9, "R").reshape(3, 3)
    T = _vec(T, 3, "T")
    org = np.zeros(3) if origin is None else _vec(origin, 3, "origin")
    fx, fy, cx, cy = (float(v) for v in (focal_x, focal_y, cx, cy))
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx != 0 and fy != 0):
        raise ValueError(f"focal_x, focal_y must be finite and non-zero, cx, cy finite: got {fx}, {fy}, {cx}, {cy}")
    _call.check_gpu(depth=depth)
    _call.same_device(device, "device", depth=depth, mask=mask, **more_on_device)
    M = np.ascontiguousarray(R.T)                     # evaluate_gs_geometry.py:198-201
    c = -(R.T if centre_from_view else M) @ T
    return H, W, ((L.C.c_double * 9)(*M.reshape(-1)), (L.C.c_double * 3)(*c), (L.C.c_double * 3)(*org),
                  cx / 2 * W + W / 2, cy / 2 * H + H / 2, fx, fy)


class DsmAccumulator:
    """Height grid that depth maps are scattered into, view after view (csrc/geometry.hip, stage 1).
    mode="max": the maximum height per cell (the reference's create_dsm_manual_satnerf_style); exact and order independent.
    mode="mean": the mean height of the points within `radius` cells (see the module docstring: unpinned); int64 fixed point
    of 2^-20 m and integer atomics, the same bits from run to run."""

    def __init__(self, grid, mode="max", radius=1, device="cuda"):
        if not isinstance(grid, DsmGrid):
            raise ValueError("grid must be a DsmGrid")
        if mode not in _MODES:
            raise ValueError(f"mode must be 'max' or 'mean', got {mode!r}")
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= 3:
            raise ValueError(f"radius must be an integer 0 ... 3, got {radius!r}")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"device must be a GPU, got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.grid, self.mode, self.radius, self.device = grid, mode, int(radius), device
        self._acc = torch.zeros((grid.ysize, grid.xsize), dtype=torch.int64, device=device)
        self._count = torch.zeros((grid.ysize, grid.xsize), dtype=torch.int32, device=device) if mode == "mean" else None
        self._num = torch.zeros(1, dtype=torch.int64, device=device)

    @property
    def num_points(self):
        """int64 [] on the device: the points that landed in the grid so far."""
        return self._num[0]

    def add_depth(self, depth, R, T, focal_x, focal_y, cx=0.0, cy=0.0, origin=None, mask=None):
        """Scatter one depth map. depth: float32 [1,H,W] or [H,W] on the GPU; R [3,3], T [3], focal_x, focal_y, cx, cy: the
        attributes of the reference's Camera (world-to-camera; cx, cy in normalised units); origin: the three numbers
        enu_to_utm_coordinates adds (UTM easting, northing, altitude of the ENU origin) or None; mask: bool / uint8, non-zero =
        use the pixel."""
        H, W, cam = _check_view(self.device, depth, R, T, focal_x, focal_y, cx, cy, origin, mask)
        lib = L.load()
        depth, mask = depth.detach().contiguous(), _u8(mask)
        g = self.grid
        args = L.SfgsDsmViewArgs(L.C.sizeof(L.SfgsDsmViewArgs), H, W, depth.data_ptr(), None if mask is None else mask.data_ptr(),
                                 *cam, g.xoff, g.yoff_top, g.resolution, g.xsize, g.ysize, _MODES[self.mode], self.radius)
        with torch.cuda.device(self.device):
            L.check(lib.sfgs_dsm_accumulate(L.C.byref(args), L.ptr(self._acc), L.ptr(self._count), L.ptr(self._num),
                                            _call.stream(self.device)))
        return self

    def add_view(self, depth, camera, origin=None, mask=None):
        """add_depth with R, T, focal_x, focal_y, cx, cy taken from a Camera-like object (cx, cy default to 0)."""
        return self.add_depth(depth, camera.R, camera.T, camera.focal_x, camera.focal_y, getattr(camera, "cx", 0.0),
                              getattr(camera, "cy", 0.0), origin=origin, mask=mask)

    def result(self):
        """-> float64 [ysize, xsize] on the device, NaN where no point fell. The accumulators stay: more views may follow."""
        lib = L.load()
        g = self.grid
        out = torch.empty((g.ysize, g.xsize), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            L.check(lib.sfgs_dsm_finalize(_MODES[self.mode], g.xsize, g.ysize, L.ptr(self._acc), L.ptr(self._count), L.ptr(out),
                                          _call.stream(self.device)))
        return out


class DsmShift(collections.namedtuple("DsmShift", "shift ab stats")):
    """Result of register(), on the device: shift int32 [2] = (dx, dy); ab float64 [2] = (a, b) of z -> a z + b;
    stats float64 [8] = a, b, mu_u, mu_v, sigma_u, sigma_v, xcorr, score at (dx, dy). cpu() is the host read."""
    __slots__ = ()

    def cpu(self):
        """-> (dx, dy, a, b) as Python numbers, the tuple dsmr.compute_shift returns."""
        s, ab = self.shift.cpu(), self.ab.cpu()
        return int(s[0]), int(s[1]), float(ab[0]), float(ab[1])


def register(ref, sec, irange=5, scaling=False, init=(0, 0)):
    """dsmr.compute_shift(ref, sec, scaling) on the device -> DsmShift: the (dx, dy, a, b) that registers `sec` on `ref`.
    ref, sec: float32 / float64 [H,W] on the GPU, shapes may differ; irange 1 ... 7 (the reference uses 5); init: the
    (dx, dy) recursive_ncc starts from (the reference passes none: 0, 0)."""
    Hu, Wu = _check_raster(ref, "ref")
    Hv, Wv = _check_raster(sec, "sec")
    if isinstance(irange, bool) or not isinstance(irange, (int, np.integer)) or not 1 <= irange <= 7:
        raise ValueError(f"irange must be an integer 1 ... 7, got {irange!r}")
    try:
        idx, idy = (int(v) for v in init)
    except (TypeError, ValueError):
        raise ValueError(f"init must be two integers, got {init!r}") from None
    if max(abs(idx), abs(idy)) > 1 << 20:
        raise ValueError(f"init beyond +-2^20: {init!r}")
    _call.check_gpu(ref=ref)
    _call.same_device(ref.device, "device", sec=sec)
    dev = ref.device
    lib = L.load()
    ref, sec = _f64(ref), _f64(sec)
    args = L.SfgsDsmrArgs(L.C.sizeof(L.SfgsDsmrArgs), Hu, Wu, Hv, Wv, ref.data_ptr(), sec.data_ptr(), int(irange),
                          int(bool(scaling)), idx, idy)
    with torch.cuda.device(dev):
        scratch = _call.scratch(lib.sfgs_dsmr_scratch_bytes(L.C.byref(args)), dev, refused_if_zero=True)
        shift = torch.empty(2, dtype=torch.int32, device=dev)
        stats = torch.empty(8, dtype=torch.float64, device=dev)
        L.check(lib.sfgs_dsmr_register(L.C.byref(args), L.ptr(shift), L.ptr(stats), L.ptr(scratch), scratch.numel(),
                                       _call.stream(dev)))
    return DsmShift(shift, stats[:2], stats)


def _check_shift(shift, dev):
    if not isinstance(shift, DsmShift):
        raise ValueError("shift must be a DsmShift (the result of register())")
    _call.same_device(dev, "device", shift=shift.shift, ab=shift.ab)


def apply_shift(sec, shift):
    """dsmr.apply_shift_ (c = d = 0) -> float64, sec's shape: out(i, j) = a * sec(i + dx, j + dy) + b, NaN outside."""
    H, W = _check_raster(sec, "sec")
    _call.check_gpu(sec=sec)
    _check_shift(shift, sec.device)
    dev = sec.device
    lib = L.load()
    sec = _f64(sec)
    s, ab = shift.shift.contiguous(), shift.ab.contiguous()
    out = torch.empty((H, W), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.sfgs_dsm_apply_shift(L.ptr(sec), H, W, L.ptr(s), L.ptr(ab), L.ptr(out), _call.stream(dev)))
    return out


def _metrics_raw(pred, gt, shift, mask):
    """-> float64 [5] on the device: mae, rmse, valid_pixels, completeness, mean(gt - pred)"""
    H, W = _check_raster(pred, "pred")
    if _check_raster(gt, "gt") != (H, W):
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have the same shape")
    _call.check_pixel_mask(mask, H, W)
    if mask is not None and mask.dim() == 3:
        mask = mask[0]
    _call.check_gpu(pred=pred)
    dev = pred.device
    _call.same_device(dev, "device", gt=gt, mask=mask)
    if shift is not None:
        _check_shift(shift, dev)
    lib = L.load()
    pred, gt, mask = _f64(pred), _f64(gt), _u8(mask)
    s = None if shift is None else shift.shift.contiguous()
    ab = None if shift is None else shift.ab.contiguous()
    with torch.cuda.device(dev):
        scratch = _call.scratch(lib.sfgs_dsm_metrics_scratch_bytes(H, W), dev, refused_if_zero=True)
        out = torch.empty(5, dtype=torch.float64, device=dev)
        L.check(lib.sfgs_dsm_metrics(L.ptr(pred), L.ptr(gt), L.ptr(mask), H, W, L.ptr(s), L.ptr(ab), L.ptr(out), L.ptr(scratch),
                                     scratch.numel(), _call.stream(dev)))
    return out


def dsm_metrics(pred, gt, shift=None, mask=None):
    """compute_dsm_metrics(pred, gt, mask) -> {"mae", "rmse", "valid_pixels", "completeness"} as device scalars (float64,
    valid_pixels int64). mask: True = keep (the caller passes `cls != 9` for water). With `shift` the prediction is
    a * pred(i + dx, j + dy) + b, formed on the fly. No pixel valid in both: NaN, NaN, 0, 0.0."""
    out = _metrics_raw(pred, gt, shift, mask)
    return {"mae": out[0], "rmse": out[1], "valid_pixels": out[2].to(torch.int64), "completeness": out[3]}


def register_simple(pred, gt):
    """register_dsms_simple's vertical-only offset -> float64 [] on the device: mean(gt - pred) over the pixels valid in both,
    0.0 when there is none."""
    return _metrics_raw(pred, gt, None, None)[4]


def evaluate_dsm(depths, cameras, grid, gt_dsm, origin=None, keep_mask=None, mode="max", irange=5, radius=1, view_masks=None,
                 cloud=None, ortho=None, images=None, consistency=None):
    """The whole chain with ONE host read: scatter every depth map into a DSM, blank the cells keep_mask excludes, register
    the DSM on gt_dsm (scaling off, as the reference calls dsmr), compare -> dict of Python numbers: mae, rmse, valid_pixels,
    completeness, dx_offset, dy_offset, dz_offset, total_points. gt_dsm: [grid.ysize, grid.xsize] on the GPU.
    cloud: a sfgs.pointcloud.PointCloud that every view is appended to as well (same pixels, same order, no host read), for
    the script's merged PLY and its bounds; the report does not depend on it.
    ortho: a sfgs.ortho.OrthoAccumulator that view k is scattered into as well, with tag k + 1 and images[k] (float32 [3,H,W],
    one per view, needed exactly then) as its colours; the report does not depend on it either.
    consistency: None, or {"rel_tol": ..., "px_tol": ..., "min_views": ...}: the multi-view consistency masks of
    sfgs.consistency are computed first, from depths, cameras and view_masks, and take the place of view_masks for the DSM, the
    cloud and the orthophoto -- evaluate_dsm(..., view_masks=ViewSet(depths, cameras, view_masks).masks(**consistency))."""
    depths, cameras = list(depths), list(cameras)
    if consistency is not None:
        from .consistency import ViewSet, check_options
        consistency = check_options(consistency)
    if cloud is not None:
        from .pointcloud import PointCloud
        if not isinstance(cloud, PointCloud):
            raise ValueError("cloud must be a sfgs.pointcloud.PointCloud or None")
    if ortho is not None:
        from .ortho import OrthoAccumulator
        if not isinstance(ortho, OrthoAccumulator):
            raise ValueError("ortho must be a sfgs.ortho.OrthoAccumulator or None")
        if images is None:
            raise ValueError("ortho needs images: one float32 [3,H,W] per view")
        images = list(images)
        if len(images) != len(depths):
            raise ValueError(f"{len(images)} images for {len(depths)} depth maps")
    elif images is not None:
        raise ValueError("images are used only with ortho")
    if len(depths) != len(cameras) or not depths:
        raise ValueError(f"{len(depths)} depth maps for {len(cameras)} cameras")
    if view_masks is not None and len(view_masks) != len(depths):
        raise ValueError(f"{len(view_masks)} view masks for {len(depths)} depth maps")
    if _check_raster(gt_dsm, "gt_dsm") != (grid.ysize, grid.xsize):
        raise ValueError(f"gt_dsm {tuple(gt_dsm.shape)} is not the grid's {(grid.ysize, grid.xsize)}")
    _call.check_pixel_mask(keep_mask, grid.ysize, grid.xsize, "keep_mask")
    _call.check_gpu(gt_dsm=gt_dsm)
    if consistency is not None:
        view_masks = ViewSet(depths, cameras, view_masks).masks(**consistency)
    acc = DsmAccumulator(grid, mode=mode, radius=radius, device=gt_dsm.device)
    for k, (depth, cam) in enumerate(zip(depths, cameras)):
        acc.add_view(depth, cam, origin=origin, mask=None if view_masks is None else view_masks[k])
        if cloud is not None:
            cloud.add_view(depth, cam, origin=origin, mask=None if view_masks is None else view_masks[k])
        if ortho is not None:
            ortho.add_view(depth, images[k], cam, origin=origin, mask=None if view_masks is None else view_masks[k], tag=k + 1)
    pred = acc.result()
    if keep_mask is not None:                             # evaluate_gs_geometry.py:455-469: water cells are NaN before dsmr
        keep = keep_mask.reshape(grid.ysize, grid.xsize) != 0
        pred = torch.where(keep, pred, torch.full_like(pred, float("nan")))
    shift = register(gt_dsm, pred, irange=irange, scaling=False)
    out = _metrics_raw(pred, gt_dsm, shift, keep_mask)
    host = torch.cat([out, shift.ab, shift.shift.to(torch.float64), acc.num_points.to(torch.float64)[None]]).cpu().tolist()
    return {"mae": host[0], "rmse": host[1], "valid_pixels": int(host[2]), "completeness": host[3], "dx_offset": int(host[7]),
            "dy_offset": int(host[8]), "dz_offset": host[6], "total_points": int(host[9])}
