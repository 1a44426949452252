"""sfgs.pointcloud -- the merged point cloud of the reference's geometry evaluation on HIP kernels (csrc/pointcloud.hip through
libsfgs.so): depth_to_point_cloud per view (evaluate_gs_geometry.py:132-215), np.vstack over the views (:776), the PLY file
(:779-784) and the bounds the script prints (:787-790), with no host read per view.

    pc = PointCloud(capacity=len(cameras) * H * W, device="cuda")
    for cam in cameras:
        pc.add_view(render(cam)["render_depth"], cam, origin=(utm_x, utm_y, alt))      # three launches, nothing read back
    points, _ = pc.result()                               # float64 [n,3] on the device: the reference's merged_point_cloud
    lo, hi = pc.bounds().cpu()                            # what the script prints as X / Y / Z bounds
    pc.save(f"{scene}_geometry_acc_point_cloud.ply")
    report = evaluate_dsm(depths, cameras, grid, gt_dsm, origin=..., cloud=pc)          # sfgs.geometry, with the cloud on the side

A pixel is used by sfgs.geometry's rule -- depth > 0, finite, mask non-zero -- and unprojected by the same float64 sequence
(one device function serves both modules; tests/geometry_np.unproject states it): rows are bit-equal to that restatement, in
the view's row-major pixel order, view after view. As in sfgs.geometry a depth of +inf is NOT used (the reference's caller
scrubs it to 0 before the call). With colors=True a row also gets three uint8 from the view's float32 [3,H,W] image, by
sfgs_frame_quantize's rule (float32 img * 255 + 0.5, clip, truncate, NaN -> 0).

The capacity is the caller's: a row beyond it is not written but still counted, and result() says which capacity would have
sufficed. There is no torch fallback: without the HIP library every operator raises."""
import os

import numpy as np
import torch

from . import _call
from . import _lib as L
from .geometry import _check_view, _u8

__all__ = ["PointCloud", "depth_to_points", "ply_table"]


def ply_table(points, colors=None):
    """numpy [n,3] float64 (and [n,3] uint8) -> the structured array save() writes: x, y, z as float64, then red, green, blue
    as uint8 when there are colours."""
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 3 or points.dtype != np.float64:
        raise ValueError(f"points must be float64 [n,3], got {points.dtype} {points.shape}")
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != points.shape or colors.dtype != np.uint8:
            raise ValueError(f"colors must be uint8 {points.shape}, got {colors.dtype} {colors.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    table = np.empty(len(points), dtype=fields)
    for j, name in enumerate("xyz"):
        table[name] = points[:, j]
    if colors is not None:
        for j, name in enumerate(("red", "green", "blue")):
            table[name] = colors[:, j]
    return table


class PointCloud:
    """Caller-sized buffer of world points that depth maps are appended to, view after view (csrc/pointcloud.hip).
    capacity: rows of the buffer (24 bytes each, 27 with colours); colors: keep a uint8 colour per row (add_* then needs
    `image`)."""

    def __init__(self, capacity, colors=False, device="cuda"):
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer, got {capacity!r}")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"device must be a GPU, got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.capacity, self.device = int(capacity), device
        self._points = torch.empty((self.capacity, 3), dtype=torch.float64, device=device)
        self._colors = torch.empty((self.capacity, 3), dtype=torch.uint8, device=device) if colors else None
        self._state = torch.zeros(1, dtype=torch.int64, device=device)

    @property
    def num_points(self):
        """int64 [] on the device: the points SEEN so far (more than `capacity` when the buffer was too small)."""
        return self._state[0]

    @property
    def points(self):
        """The whole buffer, float64 [capacity,3] on the device; rows at or beyond num_points were never written."""
        return self._points

    @property
    def colors(self):
        """uint8 [capacity,3] on the device, or None."""
        return self._colors

    def reset(self):
        """Forget every point; the buffers stay."""
        self._state.zero_()
        return self

    def add_depth(self, depth, R, T, focal_x, focal_y, cx=0.0, cy=0.0, origin=None, mask=None, image=None):
        """Append one view. The arguments of DsmAccumulator.add_depth, plus image: float32 [3,H,W] on the GPU, needed exactly
        when the cloud keeps colours."""
        H, W = _call.check_depth_map(depth)
        if (image is not None) != (self._colors is not None):
            raise ValueError("image is needed exactly when the cloud was made with colors=True")
        _call.check_tensor("image", image, f"[3,{H},{W}]", lambda t: tuple(t.shape) == (3, H, W), none_ok=True)
        H, W, cam = _check_view(self.device, depth, R, T, focal_x, focal_y, cx, cy, origin, mask, centre_from_view=True,
                                image=image)
        lib = L.load()
        depth, mask = depth.detach().contiguous(), _u8(mask)
        image = None if image is None else image.detach().contiguous()
        args = L.SfgsPointCloudViewArgs(L.C.sizeof(L.SfgsPointCloudViewArgs), H, W, depth.data_ptr(),
                                        None if mask is None else mask.data_ptr(), None if image is None else image.data_ptr(), *cam)
        with torch.cuda.device(self.device):
            scratch = _call.scratch(lib.sfgs_pointcloud_scratch_bytes(H, W), self.device, refused_if_zero=True)
            L.check(lib.sfgs_pointcloud_append(L.C.byref(args), L.ptr(self._points), L.ptr(self._colors), self.capacity,
                                               L.ptr(self._state), L.ptr(scratch), scratch.numel(), _call.stream(self.device)))
        return self

    def add_view(self, depth, camera, origin=None, mask=None, image=None):
        """add_depth with R, T, focal_x, focal_y, cx, cy taken from a Camera-like object (cx, cy default to 0)."""
        return self.add_depth(depth, camera.R, camera.T, camera.focal_x, camera.focal_y, getattr(camera, "cx", 0.0),
                              getattr(camera, "cy", 0.0), origin=origin, mask=mask, image=image)

    def result(self):
        """ONE host read (the count) -> (points[:n] float64 [n,3], colors[:n] uint8 [n,3] or None), views of the buffers on
        the device. ValueError, naming the capacity that would have sufficed, when more points were seen than stored."""
        n = int(self._state.item())
        if n > self.capacity:
            raise ValueError(f"PointCloud: {n} points seen, capacity {self.capacity}: the rows beyond it were dropped; "
                             f"a capacity of {n} would have sufficed")
        return self._points[:n], None if self._colors is None else self._colors[:n]

    def bounds(self):
        """-> float64 [2,3] on the device: (min, max) x (east, north, up) over the stored rows, what the reference prints
        from merged_point_cloud.min() / .max() per column; +inf / -inf for an empty cloud. No host read."""
        lib = L.load()
        out = torch.empty((2, 3), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            scratch = _call.scratch(lib.sfgs_pointcloud_scratch_bytes(1, 1), self.device, refused_if_zero=True)
            L.check(lib.sfgs_pointcloud_bounds(L.ptr(self._points), L.ptr(self._state), self.capacity, L.ptr(out),
                                               L.ptr(scratch), scratch.numel(), _call.stream(self.device)))
        return out

    def save(self, path):
        """Write the cloud as a PLY file through sfgs.ply.write_ply: binary little endian, `property double x / y / z`, then
        `property uchar red / green / blue` with colours -- the layout Open3D documents for write_point_cloud of a cloud whose
        points are float64 (what the reference calls, :779-783). UNPINNED: Open3D was not available to write a file to compare
        with; readers that go by the header (Open3D, plyfile, sfgs.ply.read_ply) do not depend on more than this."""
        from .ply import write_ply
        points, colors = self.result()
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        write_ply(path, ply_table(points.cpu().numpy(), None if colors is None else colors.cpu().numpy()))


def depth_to_points(depth, camera, origin=None, mask=None):
    """depth_to_point_cloud(depth, camera, enu_origin) for one view -> float64 [n,3] on the device, (east, north, up) of the
    used pixels in row-major order. A cloud of capacity H * W, one host read (the count)."""
    H, W = _call.check_depth_map(depth)
    _call.check_gpu(depth=depth)
    return PointCloud(H * W, device=depth.device).add_view(depth, camera, origin=origin, mask=mask).result()[0]
