"""sfgs.ortho -- the true orthophoto on the DSM's grid from the rendered views, on HIP kernels (csrc/ortho.hip through
libsfgs.so). The reference's geometry evaluation renders depth AND colour for every camera (evaluate_gs_geometry.py:736-765),
keeps the depth (sfgs.geometry -> DSM, sfgs.pointcloud -> merged cloud) and forgets the colour; this module keeps it: per cell
of a sfgs.geometry.DsmGrid the colour seen from straight above, i.e. of the HIGHEST point any view put there.

    o = OrthoAccumulator(grid, device="cuda")             # grid: the DsmGrid of the DSM
    for cam in cameras:
        out = render(cam)
        o.add_view(out["render_depth"], out["render"], cam, origin=(utm_x, utm_y, alt))     # one launch, nothing read back
    res = o.result(fill=1)                                # rgb, height, source, state, coverage -- all on the device
    o.save_png(f"{scene}_ortho.png", fill=1)              # RGBA PNG + .pgw world file
    report = evaluate_dsm(depths, cameras, grid, gt_dsm, origin=..., ortho=o, images=images)   # with the orthophoto on the side

Rules (tests/ortho_np.py states them in numpy; the kernels are held to it bit for bit):
  * pixel, point and cell are sfgs.geometry's: depth > 0, finite, mask non-zero; the float64 unprojection; the DSM's cell rule.
    The camera centre is formed as DsmAccumulator forms it, so the cells agree with the DSM's bit for bit;
  * the winner of a cell is the maximum over (float32 height, r, g, b, tag), lexicographically, packed into one 64-bit key
    (height first, colour second, tag last) and taken with an integer atomic: any order of the views gives the same bits.
    Heights that differ only below float32 resolution tie and colour decides; float32(DSM max) == height in every cell;
  * r, g, b are quantised by sfgs_frame_quantize's rule (float32 img * 255 + 0.5, clip, truncate, NaN -> 0);
  * the tag, 1 ... 255, says which view won a cell: a seam between two merged tiles is visible in `source`;
  * result(fill=r), r = 0 ... 3: an EMPTY cell takes the maximum key among the non-empty cells of its (2r + 1)^2 window,
    clipped to the grid; a single pass: donated values do not propagate.

There is no torch fallback: without the HIP library every operator raises. There is no install(): the reference has no
orthophoto to rebind."""
import collections
import os

import numpy as np
import torch

from . import _call
from . import _lib as L
from .geometry import DsmGrid, _check_view, _u8

__all__ = ["OrthoAccumulator", "OrthoResult", "world_file_lines"]

MAX_TAG = 255
MAX_FILL = 3

OrthoResult = collections.namedtuple("OrthoResult", "rgb height source state coverage")
OrthoResult.__doc__ = """On the device: rgb uint8 [ysize,xsize,3] (0 where empty); height float32 [ysize,xsize] (NaN where empty);
source uint8 [ysize,xsize], the winning view's tag (0 where empty); state uint8 [ysize,xsize]: 0 empty, 1 own, 2 donated by
the fill; coverage int64 [256]: [0] = cells still empty, [t] = cells coloured by tag t, own or donated (sum = xsize * ysize)."""


def world_file_lines(grid):
    """The six lines of the .pgw next to the PNG: res, 0, 0, -res, then the CENTRE of the top-left cell; repr of the float64."""
    g = grid
    return [repr(float(v)) for v in (g.resolution, 0.0, 0.0, -g.resolution, g.xoff + g.resolution / 2, g.yoff_top - g.resolution / 2)]


def _check_fill(fill):
    if isinstance(fill, bool) or not isinstance(fill, (int, np.integer)) or not 0 <= fill <= MAX_FILL:
        raise ValueError(f"fill must be an integer 0 ... {MAX_FILL}, got {fill!r}")
    return int(fill)


class OrthoAccumulator:
    """Colour grid that rendered views are scattered into, view after view (csrc/ortho.hip): one uint64 key per cell."""

    def __init__(self, grid, device="cuda"):
        if not isinstance(grid, DsmGrid):
            raise ValueError("grid must be a sfgs.geometry.DsmGrid")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"device must be a GPU, got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.grid, self.device = grid, device
        self.num_views = 0
        self._acc = torch.zeros((grid.ysize, grid.xsize), dtype=torch.int64, device=device)
        self._num = torch.zeros(1, dtype=torch.int64, device=device)

    @property
    def num_points(self):
        """int64 [] on the device: the points that landed in the grid so far."""
        return self._num[0]

    def reset(self):
        """Forget every view; the buffers stay."""
        self._acc.zero_()
        self._num.zero_()
        self.num_views = 0
        return self

    def _tag(self, tag):
        if tag is None:
            tag = self.num_views + 1
            if tag > MAX_TAG:
                raise ValueError(f"this would be view {tag}: implicit tags end at {MAX_TAG}; pass tag= to share one among views")
            return tag
        if isinstance(tag, bool) or not isinstance(tag, (int, np.integer)) or not 1 <= tag <= MAX_TAG:
            raise ValueError(f"tag must be an integer 1 ... {MAX_TAG} or None, got {tag!r}")
        return int(tag)

    def add_depth(self, depth, image, R, T, focal_x, focal_y, cx=0.0, cy=0.0, origin=None, mask=None, tag=None):
        """Scatter one view. The arguments of DsmAccumulator.add_depth, plus image: float32 [3,H,W] on the GPU, the view's
        colours; tag: 1 ... 255, what `source` shows where this view wins (None: views added so far + 1)."""
        H, W = _call.check_depth_map(depth)
        _call.check_tensor("image", image, f"[3,{H},{W}]", lambda t: tuple(t.shape) == (3, H, W))
        tag = self._tag(tag)
        H, W, cam = _check_view(self.device, depth, R, T, focal_x, focal_y, cx, cy, origin, mask, image=image)
        lib = L.load()
        depth, mask, image = depth.detach().contiguous(), _u8(mask), image.detach().contiguous()
        g = self.grid
        args = L.SfgsOrthoViewArgs(L.C.sizeof(L.SfgsOrthoViewArgs), H, W, depth.data_ptr(), None if mask is None else mask.data_ptr(),
                                   *cam, g.xoff, g.yoff_top, g.resolution, g.xsize, g.ysize, image.data_ptr(), tag)
        with torch.cuda.device(self.device):
            L.check(lib.sfgs_ortho_accumulate(L.C.byref(args), L.ptr(self._acc), L.ptr(self._num), _call.stream(self.device)))
        self.num_views += 1
        return self

    def add_view(self, depth, image, camera, origin=None, mask=None, tag=None):
        """add_depth with R, T, focal_x, focal_y, cx, cy taken from a Camera-like object (cx, cy default to 0)."""
        return self.add_depth(depth, image, camera.R, camera.T, camera.focal_x, camera.focal_y, getattr(camera, "cx", 0.0),
                              getattr(camera, "cy", 0.0), origin=origin, mask=mask, tag=tag)

    def result(self, fill=0):
        """-> OrthoResult on the device, no host read. fill 0 ... 3: see the module docstring. The accumulator stays: more
        views may follow."""
        fill = _check_fill(fill)
        lib = L.load()
        g, dev = self.grid, self.device
        rgb = torch.empty((g.ysize, g.xsize, 3), dtype=torch.uint8, device=dev)
        height = torch.empty((g.ysize, g.xsize), dtype=torch.float32, device=dev)
        source = torch.empty((g.ysize, g.xsize), dtype=torch.uint8, device=dev)
        state = torch.empty((g.ysize, g.xsize), dtype=torch.uint8, device=dev)
        coverage = torch.zeros(256, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.sfgs_ortho_resolve(g.xsize, g.ysize, fill, L.ptr(self._acc), L.ptr(rgb), L.ptr(height), L.ptr(source),
                                           L.ptr(state), L.ptr(coverage), _call.stream(dev)))
        return OrthoResult(rgb, height, source, state, coverage)

    def save_png(self, path, fill=0):
        """Write result(fill) as an RGBA PNG (alpha 255 where state != 0, else 0) and, next to it, the world file: the
        PNG's path with the extension .pgw, six lines (world_file_lines)."""
        fill = _check_fill(fill)
        try:
            from PIL import Image
        except ImportError:
            raise ValueError("save_png needs PIL (Pillow), which is not importable here") from None
        res = self.result(fill)
        rgba = torch.cat([res.rgb, ((res.state != 0).to(torch.uint8) * 255)[..., None]], dim=-1).cpu().numpy()
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        Image.fromarray(rgba, "RGBA").save(path, format="PNG")
        with open(os.path.splitext(path)[0] + ".pgw", "w") as f:
            f.write("\n".join(world_file_lines(self.grid)) + "\n")
