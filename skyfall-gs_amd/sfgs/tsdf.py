"""sfgs.tsdf -- depth views fused into a truncated-signed-distance (TSDF) volume and a triangle mesh extracted from it, on HIP
kernels (csrc/tsdf.hip through libsfgs.so). The DSM of sfgs.geometry is 2.5-D and loses every facade, the cloud of sfgs.pointcloud
is unconnected points; this is the surface. The reference has no mesh step.

    vs = ViewSet(depths, cameras)                                      # sfgs.consistency: the masks a fusion wants
    vol = TsdfVolume(origin=(x0, y0, z0), dims=(512, 512, 128), voxel_size=0.5, trunc=1.5, colors=True)
    vol.add_views(depths, cameras, masks=vs.masks(), images=images)    # one launch per batch of <= 256 views
    soup = vol.extract(capacity=8_000_000)                             # three launches, nothing read back
    soup.save_ply("city.ply", origin=(utm_x, utm_y, alt))              # welded, binary, double vertices
    mesh = soup.mesh()                                                 # sfgs.mesh: welded on the device, to label and clean there

The volume is axis-aligned in the cameras' own frame; voxel (i, j, k) has its centre at origin + (i + 0.5, j + 0.5, k + 0.5) *
voxel_size. Integration (include/sfgs.h states it in full, tests/tsdf_np.py in numpy; the kernel equals that restatement byte
for byte): a voxel centre is projected into a view as sfgs.consistency projects a point; if it lies in front of the camera, its
nearest pixel is inside the image and used (depth > 0, finite, mask non-zero) and sdf = depth - z is not below -trunc, the voxel
takes the running mean of s = min(1, sdf / trunc) -- and of the image's pixel, with colours -- under a weight that grows by one
per view up to max_weight. A voxel's value depends on the order of the views alone: one call with all views, one view per call
and any split give the same bits.

Extraction is marching TETRAHEDRA over the cells whose eight corners were all observed: six tetrahedra per cell around the body
diagonal, no ambiguous case, a closed surface wherever the volume was observed. Every vertex is computed from its edge's two
voxels in a canonical order, so the soup welds by byte equality (TriangleSoup.weld). Triangles wind so that their normal points
toward positive distances (the free side).

Ray-casting is the third step: the volume seen from a camera, for a preview of the fused surface, a multi-view-consistent
depth map for a camera that was never rendered, or a pixel-for-pixel comparison with a Gaussian render's depth.

    view = vol.raycast(camera, 1024, 1024)                             # one launch, plus one for the empty-space table
    view.depth, view.normal, view.rgb                                  # [1,H,W], [3,H,W], [3,H,W]; zeros where no surface was found
    skip = vol.ray_skip()                                              # the table, reusable while the volume is unchanged
    views = [vol.raycast(cam, 1024, 1024, skip=skip) for cam in cameras]

A thread owns a pixel and marches its ray through the box of voxel centres on a lattice of depths `step` apart (voxel_size by
default, measured along the camera's forward axis like the project's depth maps), trilinear on the eight voxels around each
sample. The hit is the first pair of consecutive samples, both with all eight voxels observed, whose values go from >= 0 to
< 0; depth, normal (the trilinear gradient, unit length, world frame, toward the free side) and colour are interpolated
between the two. Empty-space skipping -- a byte per brick of 8 x 8 x 8 cells that says whether any of its voxels is observed and
inside; samples in bricks without one are jumped over -- changes no byte: skip=False, skip=None and a prebuilt table agree, and
the kernel equals the numpy restatement tests/tsdf_raycast_np.py byte for byte. Orthographic cameras, several views per launch
and gradients through the ray-cast are not there.

There is no sparse or hashed volume, no mesh simplification and no torch fallback: without the HIP library every operator raises."""
import math
import os

import numpy as np
import torch

from . import _call
from . import _lib as L
from .geometry import _check_view, _u8, _vec

__all__ = ["TsdfVolume", "TriangleSoup", "RayView", "RaySkip", "MAX_VIEWS", "MAX_VOXELS"]

MAX_VIEWS = 256
MAX_VOXELS = 1 << 30


def _positive(x, name, allow_inf=False, at_least=None):
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, got {x!r}") from None
    if isinstance(x, bool) or math.isnan(v) or (not allow_inf and math.isinf(v)):
        raise ValueError(f"{name} must be {'a' if allow_inf else 'a finite'} number, got {x!r}")
    if at_least is None and not v > 0:
        raise ValueError(f"{name} must be > 0, got {x!r}")
    if at_least is not None and not v >= at_least:
        raise ValueError(f"{name} must be >= {at_least}, got {x!r}")
    return v


class TsdfVolume:
    """Dense TSDF volume that depth views are fused into (csrc/tsdf.hip).
    origin: the corner of voxel (0, 0, 0), three finite numbers; dims: (nx, ny, nz) voxels, nx * ny * nz <= 2^30; voxel_size and
    trunc: finite, > 0, in the cameras' units; max_weight >= 1 (inf: a plain mean); colors: keep a float32 colour per voxel
    (add_views then needs `images`). Storage: float32 tsdf [nz,ny,nx], weight [nz,ny,nx] and rgb [3,nz,ny,nx], x fastest."""

    def __init__(self, origin, dims, voxel_size, trunc, max_weight=64.0, colors=False, device="cuda"):
        self.origin = tuple(float(v) for v in _vec(origin, 3, "origin"))
        try:
            dims = tuple(dims)
        except TypeError:
            raise ValueError(f"dims must be three positive integers, got {dims!r}") from None
        if len(dims) != 3 or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1 for n in dims):
            raise ValueError(f"dims must be three positive integers, got {dims!r}")
        self.dims = tuple(int(n) for n in dims)
        if self.dims[0] * self.dims[1] * self.dims[2] > MAX_VOXELS:
            raise ValueError(f"nx * ny * nz must not exceed 2^30, got {self.dims}")
        self.voxel_size = _positive(voxel_size, "voxel_size")
        self.trunc = _positive(trunc, "trunc")
        self.max_weight = _positive(max_weight, "max_weight", allow_inf=True, at_least=1.0)
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"device must be a GPU, got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        nx, ny, nz = self.dims
        self._tsdf = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self._weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self._rgb = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=device) if colors else None

    @property
    def colors(self):
        return self._rgb is not None

    @property
    def tsdf(self):
        """float32 [nz,ny,nx] on the device: the mean of min(1, sdf / trunc); meaningful where weight > 0."""
        return self._tsdf

    @property
    def weight(self):
        """float32 [nz,ny,nx] on the device: the views that updated a voxel, capped at max_weight."""
        return self._weight

    @property
    def rgb(self):
        """float32 [3,nz,ny,nx] on the device, or None."""
        return self._rgb

    def reset(self):
        """Forget every view; the buffers stay."""
        self._tsdf.zero_()
        self._weight.zero_()
        if self._rgb is not None:
            self._rgb.zero_()
        return self

    def load(self, tsdf, weight, rgb=None):
        """Set the state from float32 tensors of the volume's shapes (copied; any device)."""
        nx, ny, nz = self.dims
        _call.check_tensor("tsdf", tsdf, f"[{nz},{ny},{nx}]", lambda t: tuple(t.shape) == (nz, ny, nx))
        _call.check_tensor("weight", weight, f"[{nz},{ny},{nx}]", lambda t: tuple(t.shape) == (nz, ny, nx))
        if (rgb is not None) != self.colors:
            raise ValueError("rgb is needed exactly when the volume was made with colors=True")
        _call.check_tensor("rgb", rgb, f"[3,{nz},{ny},{nx}]", lambda t: tuple(t.shape) == (3, nz, ny, nx), none_ok=True)
        self._tsdf.copy_(tsdf.detach())
        self._weight.copy_(weight.detach())
        if rgb is not None:
            self._rgb.copy_(rgb.detach())
        return self

    def _struct(self):
        nx, ny, nz = self.dims
        return L.SfgsTsdfVolume(L.C.sizeof(L.SfgsTsdfVolume), nx, ny, nz, (L.C.c_double * 3)(*self.origin), self.voxel_size, self.trunc,
                                self.max_weight, self._tsdf.data_ptr(), self._weight.data_ptr(),
                                None if self._rgb is None else self._rgb.data_ptr())

    def add_views(self, depths, cameras, masks=None, images=None):
        """Fuse a batch of 1 ... 256 views, in the order given, with ONE launch. depths: float32 [1,H,W] or [H,W] on the volume's
        GPU, sizes may differ; cameras: Camera-like objects read as sfgs.consistency reads them (R, T, focal_x, focal_y; cx, cy
        default to 0); masks: None, or one entry per view, each None or bool / uint8 of the view's size (what ViewSet.masks()
        returns); images: one float32 [3,H,W] per view, needed exactly when the volume keeps colours."""
        try:
            depths, cameras = list(depths), list(cameras)
            masks = [None] * len(depths) if masks is None else list(masks)
            images = None if images is None else list(images)
        except TypeError:
            raise ValueError("depths, cameras, masks and images must be sequences") from None
        if (images is not None) != self.colors:
            raise ValueError("images are needed exactly when the volume was made with colors=True")
        if len(depths) != len(cameras) or len(masks) != len(depths) or (images is not None and len(images) != len(depths)):
            raise ValueError(f"{len(depths)} depth maps for {len(cameras)} cameras, {len(masks)} masks"
                             + ("" if images is None else f" and {len(images)} images"))
        if not 1 <= len(depths) <= MAX_VIEWS:
            raise ValueError(f"a batch has 1 ... {MAX_VIEWS} views, got {len(depths)}")
        records, held = (L.SfgsTsdfView * len(depths))(), []
        for k, (depth, cam, mask) in enumerate(zip(depths, cameras, masks)):
            image = None if images is None else images[k]
            try:
                H, W = _call.check_depth_map(depth, f"depths[{k}]")
                _call.check_tensor(f"images[{k}]", image, f"[3,{H},{W}]", lambda t: tuple(t.shape) == (3, H, W), none_ok=images is None)
                try:
                    cam = (cam.R, cam.T, cam.focal_x, cam.focal_y, getattr(cam, "cx", 0.0), getattr(cam, "cy", 0.0))
                except AttributeError as e:
                    raise ValueError(f"cameras[{k}]: {e}") from None
                H, W, (M, c, _, cx_pix, cy_pix, fx, fy) = _check_view(self.device, depth, *cam, None, mask, centre_from_view=True,
                                                                      image=image)
            except ValueError as e:
                raise ValueError(f"view {k}: {e}") from None
            depth, mask = depth.detach().contiguous(), _u8(mask)
            image = None if image is None else image.detach().contiguous()
            held.append((depth, mask, image))             # the table points into these until the launch is queued
            records[k] = L.SfgsTsdfView(depth.data_ptr(), None if mask is None else mask.data_ptr(),
                                        None if image is None else image.data_ptr(), H, W, M, c, cx_pix, cy_pix, fx, fy)
        lib = L.load()
        L.check(lib.sfgs_tsdf_table_check(records, len(depths), int(self.colors)))
        vol = self._struct()
        with torch.cuda.device(self.device):
            table = torch.frombuffer(bytearray(bytes(records)), dtype=torch.uint8).to(self.device)
            L.check(lib.sfgs_tsdf_integrate(L.C.byref(vol), L.ptr(table), len(depths), _call.stream(self.device)))
        del held                                          # the launch is queued on the stream their memory belongs to
        return self

    def add_view(self, depth, camera, mask=None, image=None):
        """The batch of one."""
        return self.add_views([depth], [camera], None if mask is None else [mask], None if image is None else [image])

    def extract(self, capacity):
        """-> TriangleSoup of at most `capacity` triangles (36 bytes each, 72 with colours), ordered by cell, tetrahedron,
        triangle. A triangle beyond the capacity is not written but still counted. Three launches, nothing read back."""
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer, got {capacity!r}")
        capacity = int(capacity)
        lib = L.load()
        vertices = torch.empty((capacity, 3, 3), dtype=torch.float32, device=self.device)
        colors = torch.empty((capacity, 3, 3), dtype=torch.float32, device=self.device) if self.colors else None
        state = torch.zeros(1, dtype=torch.int64, device=self.device)
        vol = self._struct()
        with torch.cuda.device(self.device):
            scratch = _call.scratch(lib.sfgs_tsdf_scratch_bytes(*self.dims), self.device, refused_if_zero=True)
            L.check(lib.sfgs_tsdf_extract(L.C.byref(vol), L.ptr(vertices), L.ptr(colors), capacity, L.ptr(state), L.ptr(scratch),
                                          scratch.numel(), _call.stream(self.device)))
        return TriangleSoup(vertices, colors, state, capacity)

    def ray_skip(self):
        """-> RaySkip: the empty-space table of the volume's PRESENT state for raycast(skip=...), one byte per brick of 8 x 8 x 8
        cells, non-zero where a voxel of the brick is observed and inside. One launch. It may be reused until the volume changes
        (add_views, load, reset); raycast cannot tell a stale one."""
        lib = L.load()
        nbytes = lib.sfgs_tsdf_skip_bytes(*self.dims)
        if nbytes == 0:
            raise RuntimeError(f"libsfgs: {lib.sfgs_last_error().decode(errors='replace')}")
        bricks = tuple(1 if n < 2 else (n + 6) // 8 for n in reversed(self.dims))
        assert nbytes == bricks[0] * bricks[1] * bricks[2], (nbytes, bricks)
        table = torch.empty(bricks, dtype=torch.uint8, device=self.device)
        vol = self._struct()
        with torch.cuda.device(self.device):
            L.check(lib.sfgs_tsdf_skip_build(L.C.byref(vol), L.ptr(table), nbytes, _call.stream(self.device)))
        return RaySkip(table, self.dims)

    def raycast(self, camera, height, width, step=None, near=0.0, far=math.inf, normals=True, skip=None, out=None):
        """-> RayView: the volume seen from `camera` at height x width pixels -- depth along the forward axis (0 where the ray
        finds no surface), the unit normal toward the free side in the world frame and, when the volume keeps colours, the
        colour -- with ONE launch and nothing read back. camera: read as add_views reads one (R, T, focal_x, focal_y; cx, cy
        default to 0). step: the spacing of the samples along the forward axis, voxel_size by default; near, far: the range of
        depths. A ray hits between the first two consecutive observed samples whose values go from >= 0 to < 0. skip: None
        builds the empty-space table in the call (one more launch), False marches every sample, a ray_skip() result is used as
        given; the three give the same bytes. out: a RayView of an earlier call with the same arguments, written again."""
        for name, v in (("height", height), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        H, W = int(height), int(width)
        if H * W > 1 << 30:
            raise ValueError(f"height * width must not exceed 2^30, got {H} x {W}")
        step = self.voxel_size if step is None else _positive(step, "step")
        near = _positive(near, "near", at_least=0.0)
        far = _positive(far, "far", allow_inf=True)
        if not far > near:
            raise ValueError(f"far must be above near, got near {near}, far {far}")
        diagonal = self.voxel_size * math.sqrt(sum((n - 1) ** 2 for n in self.dims))
        if diagonal / step > 1 << 20:
            raise ValueError(f"step {step}: the volume's diagonal {diagonal} holds more than 2^20 steps")
        if not (skip is None or skip is False or isinstance(skip, RaySkip)):
            raise ValueError(f"skip must be None, False or a ray_skip() result, got {skip!r}")
        if isinstance(skip, RaySkip):
            if skip.dims != self.dims:
                raise ValueError(f"skip was made for dims {skip.dims}, the volume has {self.dims}")
            _call.same_device(self.device, "device", skip=skip.table)
        if not isinstance(normals, (bool, np.bool_)):
            raise ValueError(f"normals must be a bool, got {normals!r}")
        normals = bool(normals)
        if out is not None:
            if not isinstance(out, RayView):
                raise ValueError(f"out must be a RayView, got {out!r}")
            if (out.normal is not None) != normals or (out.rgb is not None) != self.colors:
                raise ValueError("out was made with other normals or by a volume with other colours")
            _call.check_tensor("out.depth", out.depth, f"[1,{H},{W}]", lambda t: tuple(t.shape) == (1, H, W) and t.is_contiguous())
            for name, t in (("out.normal", out.normal), ("out.rgb", out.rgb)):
                _call.check_tensor(name, t, f"[3,{H},{W}]", lambda t: tuple(t.shape) == (3, H, W) and t.is_contiguous(), none_ok=True)
        try:
            cam = (camera.R, camera.T, camera.focal_x, camera.focal_y, getattr(camera, "cx", 0.0), getattr(camera, "cy", 0.0))
        except AttributeError as e:
            raise ValueError(f"camera: {e}") from None
        if out is None:
            out = RayView(torch.empty((1, H, W), dtype=torch.float32, device=self.device),
                          torch.empty((3, H, W), dtype=torch.float32, device=self.device) if normals else None,
                          torch.empty((3, H, W), dtype=torch.float32, device=self.device) if self.colors else None)
        # the view's checks on the depth map that will be written: its size, its device, the camera's numbers
        _, _, (M, c, _, cx_pix, cy_pix, fx, fy) = _check_view(self.device, out.depth, *cam, None, None, centre_from_view=True,
                                                              normal=out.normal, rgb=out.rgb)
        lib = L.load()
        if skip is None:
            skip = self.ray_skip()
        table = skip.table if isinstance(skip, RaySkip) else None
        ray = L.SfgsTsdfRay(L.C.sizeof(L.SfgsTsdfRay), H, W, M, c, cx_pix, cy_pix, fx, fy, near, far, step, out.depth.data_ptr(),
                            None if out.normal is None else out.normal.data_ptr(), None if out.rgb is None else out.rgb.data_ptr())
        vol = self._struct()
        with torch.cuda.device(self.device):
            L.check(lib.sfgs_tsdf_raycast(L.C.byref(vol), L.C.byref(ray), L.ptr(table), 0 if table is None else table.numel(),
                                          _call.stream(self.device)))
        return out


class RaySkip:
    """The result of TsdfVolume.ray_skip. table: uint8 [bz,by,bx] on the device, a byte per brick of 8 x 8 x 8 cells; dims: the
    volume's dims it was made for."""

    def __init__(self, table, dims):
        self.table, self.dims = table, tuple(dims)


class RayView:
    """The result of TsdfVolume.raycast, on the device. depth: float32 [1,H,W], 0 where the ray found no surface; normal: float32
    [3,H,W] in the world frame, unit length, toward the free side, zeros where depth is 0, or None; rgb: float32 [3,H,W], zeros
    where depth is 0, or None when the volume keeps no colours. An ordinary view: depth goes into add_views, evaluate_dsm,
    sfgs.pointcloud, sfgs.ortho and ViewSet as a rendered depth map does."""

    def __init__(self, depth, normal, rgb):
        self.depth, self.normal, self.rgb = depth, normal, rgb


class TriangleSoup:
    """The result of TsdfVolume.extract, on the device: three vertices per triangle, no sharing.
    buffer / color_buffer: float32 [capacity,3,3], rows at or beyond num_triangles never written."""

    def __init__(self, buffer, color_buffer, state, capacity):
        self.buffer, self.color_buffer, self._state, self.capacity = buffer, color_buffer, state, capacity
        self._n = None

    @property
    def num_triangles(self):
        """int64 [] on the device: the triangles FOUND (more than `capacity` when the buffer was too small)."""
        return self._state[0]

    def _valid(self):
        if self._n is None:                               # ONE host read
            n = int(self._state.item())
            if n > self.capacity:
                raise ValueError(f"TriangleSoup: {n} triangles found, capacity {self.capacity}: the rows beyond it were dropped; "
                                 f"a capacity of {n} would have sufficed")
            self._n = n
        return self._n

    @property
    def vertices(self):
        """float32 [n,3,3] on the device: a view of the valid rows. ValueError when more were found than stored."""
        return self.buffer[:self._valid()]

    @property
    def colors(self):
        """float32 [n,3,3] on the device (a colour per vertex), or None."""
        return None if self.color_buffer is None else self.color_buffer[:self._valid()]

    def _welded(self):
        flat = np.ascontiguousarray(self.vertices.cpu().numpy()).reshape(-1, 3)
        keys = flat.view(np.dtype((np.void, 12))).reshape(-1)
        _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
        return flat[first], inverse.reshape(-1, 3).astype(np.int64), first

    def weld(self):
        """On the host -> (V float32 [m,3], F int64 [n,3]): vertices with the same twelve bytes become one (np.unique over the
        bytes: V is in byte order). Every tetrahedron that shares an edge produced the same bytes for its point."""
        V, F, _ = self._welded()
        return V, F

    def mesh(self):
        """On the device -> sfgs.mesh.Mesh: the welded, indexed mesh (vertices in order of first appearance, int32 faces, the
        colour of a vertex's first appearance), to label and clean there. ValueError when more triangles were found than stored."""
        from . import mesh as _mesh
        return _mesh.weld(self.buffer, self.color_buffer, self._valid())

    def save_ply(self, path, weld=True, origin=None):
        """Binary little-endian PLY with a `vertex` and a `face` element (`property list uchar int vertex_indices`). Vertices
        are `double` with origin (three numbers, e.g. the UTM offset, added in float64) and `float` without; with colours,
        `uchar red / green / blue` by the reference's rule (x * 255 + 0.5).clip(0, 255) (train.py:440). weld=False writes the
        soup as it is, three vertices per triangle."""
        org = None if origin is None else _vec(origin, 3, "origin")
        if weld:
            V, F, first = self._welded()
        else:
            V = np.ascontiguousarray(self.vertices.cpu().numpy()).reshape(-1, 3)
            F, first = np.arange(len(V), dtype=np.int64).reshape(-1, 3), slice(None)
        if len(V) > np.iinfo(np.int32).max:
            raise ValueError(f"{len(V)} vertices do not fit the PLY's int indices")
        kind, ftype = ("double", "<f8") if org is not None else ("float", "<f4")
        fields = [(a, ftype) for a in "xyz"]
        header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(V)}"] + [f"property {kind} {a}" for a in "xyz"]
        if self.color_buffer is not None:
            fields += [(n, "u1") for n in ("red", "green", "blue")]
            header += [f"property uchar {n}" for n in ("red", "green", "blue")]
        header += [f"element face {len(F)}", "property list uchar int vertex_indices", "end_header"]
        vt = np.empty(len(V), dtype=fields)
        for j, a in enumerate("xyz"):
            vt[a] = V[:, j] if org is None else V[:, j].astype(np.float64) + org[j]
        if self.color_buffer is not None:
            c = np.ascontiguousarray(self.colors.cpu().numpy()).reshape(-1, 3)[first]
            with np.errstate(invalid="ignore"):
                q = np.where(np.isnan(c), np.float32(0), (c * np.float32(255) + np.float32(0.5)).clip(0, 255)).astype(np.uint8)
            for j, n in enumerate(("red", "green", "blue")):
                vt[n] = q[:, j]
        ft = np.empty(len(F), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        ft["n"], ft["i"] = 3, F
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, "wb") as f:
            f.write(("\n".join(header) + "\n").encode("ascii"))
            vt.tofile(f)
            ft.tofile(f)
