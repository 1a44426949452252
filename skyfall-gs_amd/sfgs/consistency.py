"""sfgs.consistency -- multi-view depth consistency masks on a HIP kernel (csrc/consistency.hip through libsfgs.so): the
per-view pixel mask that sfgs.geometry, sfgs.pointcloud and sfgs.ortho take (`mask=` on every add_view, `view_masks=` on
evaluate_dsm) and that nothing produced so far. A rendered depth is an alpha-blended expectation: at a roof edge it mixes roof
and ground and unprojects to a point in mid-air, and under the DSM's mode="max" that point decides its cell. The remedy is the
geometric check of multi-view stereo fusion: keep a depth pixel only if enough OTHER views see the same surface there. The
reference has no such step.

    vs = ViewSet(depths, cameras, masks=None)             # host checks, then the device table; the tensors are held, not copied
    count, keep = vs.check(i, rel_tol=0.01, px_tol=1.0, min_views=2)      # uint8 [H_i, W_i] each, on the device; one launch
    keeps = vs.masks(rel_tol=0.01, px_tol=1.0, min_views=2)               # keep of every view: the view_masks of evaluate_dsm
    report = evaluate_dsm(depths, cameras, grid, gt_dsm, origin=..., consistency=dict(rel_tol=0.01, px_tol=1.0, min_views=2))

The pair test (include/sfgs.h states it in full, tests/consistency_np.py in numpy; the kernel equals that restatement byte for
byte). Pixel (r, c) of view i, if used (depth > 0, finite, mask non-zero), is unprojected by sfgs.geometry's float64 sequence
with the camera constants of sfgs.pointcloud and no origin. A source j != i confirms it when the point lies in front of j,
projects -- rounded to the nearest pixel -- inside j's image onto a used pixel whose depth d_j differs from the point's depth z
in j by at most rel_tol * z, and when THAT pixel of j, unprojected and projected back into i, lands within px_tol pixels of
(r, c). count = the confirming sources, keep = count >= min_views. Views may differ in size; 2 ... 256 views.

There is no fused depth and no source-subset option: a caller who wants fewer sources builds a smaller set. There is no torch
fallback: without the HIP library check() raises. There is no install(): the reference has nothing to rebind."""
import math

import numpy as np
import torch

from . import _call
from . import _lib as L
from .geometry import _check_view, _u8

__all__ = ["ViewSet", "MAX_VIEWS"]

MAX_VIEWS = 256
_KEYS = ("rel_tol", "px_tol", "min_views")


def _check_tolerances(rel_tol, px_tol, min_views):
    """-> (rel_tol, px_tol * px_tol, min_views) as the library takes them; the square is formed here, once, in float64"""
    try:
        rel, px = float(rel_tol), float(px_tol)
    except (TypeError, ValueError):
        raise ValueError(f"rel_tol, px_tol must be numbers, got {rel_tol!r}, {px_tol!r}") from None
    if not (math.isfinite(rel) and rel > 0):
        raise ValueError(f"rel_tol must be finite and > 0, got {rel_tol!r}")
    if not px > 0:                                        # NaN fails; +inf passes: no bound on the round trip
        raise ValueError(f"px_tol must be > 0 (inf: no bound), got {px_tol!r}")
    if isinstance(min_views, bool) or not isinstance(min_views, (int, np.integer)) or min_views < 1:
        raise ValueError(f"min_views must be an integer >= 1, got {min_views!r}")
    return rel, px * px, int(min(int(min_views), MAX_VIEWS))          # no count exceeds MAX_VIEWS - 1


def check_options(consistency):
    """The `consistency=` dict of evaluate_dsm -> its three values checked, as keyword arguments of ViewSet.masks."""
    if not isinstance(consistency, dict) or sorted(consistency) != sorted(_KEYS):
        raise ValueError(f"consistency must be a dict with the keys {', '.join(_KEYS)}, got {consistency!r}")
    _check_tolerances(**consistency)
    return dict(consistency)


class ViewSet:
    """Depth maps with their cameras, ready to be checked against each other (csrc/consistency.hip).
    depths: float32 [1,H,W] or [H,W] on one GPU, sizes may differ; cameras: Camera-like objects read as sfgs.pointcloud reads
    them (R, T, focal_x, focal_y, cx, cy; cx, cy default to 0); masks: None, or one entry per view, each None or bool / uint8
    of the view's size (non-zero = the pixel may be used, as a reference and as a source)."""

    def __init__(self, depths, cameras, masks=None):
        try:
            depths, cameras = list(depths), list(cameras)
            masks = [None] * len(depths) if masks is None else list(masks)
        except TypeError:
            raise ValueError("depths, cameras and masks must be sequences") from None
        if len(depths) != len(cameras) or len(masks) != len(depths):
            raise ValueError(f"{len(depths)} depth maps for {len(cameras)} cameras and {len(masks)} masks")
        if not 2 <= len(depths) <= MAX_VIEWS:
            raise ValueError(f"a ViewSet has 2 ... {MAX_VIEWS} views, got {len(depths)}")
        _call.check_depth_map(depths[0], "depths[0]")
        device = depths[0].device
        records = (L.SfgsConsistencyView * len(depths))()
        self.sizes, self._held = [], []
        for k, (depth, cam, mask) in enumerate(zip(depths, cameras, masks)):
            _call.check_depth_map(depth, f"depths[{k}]")
            try:
                cam = (cam.R, cam.T, cam.focal_x, cam.focal_y, getattr(cam, "cx", 0.0), getattr(cam, "cy", 0.0))
            except AttributeError as e:
                raise ValueError(f"cameras[{k}]: {e}") from None
            try:
                H, W, (M, c, _, cx_pix, cy_pix, fx, fy) = _check_view(device, depth, *cam, None, mask, centre_from_view=True)
            except ValueError as e:
                raise ValueError(f"view {k}: {e}") from None
            depth, mask = depth.detach().contiguous(), _u8(mask)
            self._held.append((depth, mask))              # the table points into these
            self.sizes.append((H, W))
            records[k] = L.SfgsConsistencyView(depth.data_ptr(), None if mask is None else mask.data_ptr(), H, W, M, c, cx_pix,
                                               cy_pix, fx, fy)
        self.device = device
        lib = L.load()
        L.check(lib.sfgs_consistency_table_check(records, len(depths)))
        self._table = torch.frombuffer(bytearray(bytes(records)), dtype=torch.uint8).to(device)      # ONE upload per set

    def __len__(self):
        return len(self.sizes)

    def _index(self, i):
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < len(self):
            raise ValueError(f"i must be an integer 0 ... {len(self) - 1}, got {i!r}")
        return int(i)

    def _launch(self, lib, i, rel, px2, min_views):
        H, W = self.sizes[i]
        count = torch.empty((H, W), dtype=torch.uint8, device=self.device)
        keep = torch.empty((H, W), dtype=torch.uint8, device=self.device)
        args = L.SfgsConsistencyArgs(L.C.sizeof(L.SfgsConsistencyArgs), len(self), i, H, W, min_views, self._table.data_ptr(), rel,
                                     px2)
        with torch.cuda.device(self.device):
            L.check(lib.sfgs_consistency_check(L.C.byref(args), L.ptr(count), L.ptr(keep), _call.stream(self.device)))
        return count, keep

    def check(self, i, rel_tol=0.01, px_tol=1.0, min_views=2):
        """View i against all the others -> (count, keep), uint8 [H_i, W_i] each, on the device: the sources that confirm a
        pixel, and count >= min_views. One launch, nothing read back. px_tol=inf switches the round-trip bound off."""
        i = self._index(i)
        rel, px2, min_views = _check_tolerances(rel_tol, px_tol, min_views)
        return self._launch(L.load(), i, rel, px2, min_views)

    def masks(self, rel_tol=0.01, px_tol=1.0, min_views=2):
        """-> [keep of view 0, keep of view 1, ...]: what add_view(mask=) and evaluate_dsm(view_masks=) take. The input masks
        are folded in: a pixel they exclude has count 0."""
        rel, px2, min_views = _check_tolerances(rel_tol, px_tol, min_views)
        lib = L.load()
        return [self._launch(lib, i, rel, px2, min_views)[1] for i in range(len(self))]
