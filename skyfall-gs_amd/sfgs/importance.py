"""Per-Gaussian blend-weight statistics over a set of views, and pruning by them (include/sfgs.h, ABI 28; kernels:
csrc/importance.hip).

Which Gaussians of a trained or merged scene show up in the views that matter? For every (pixel, Gaussian) pair the
rasterizer blends, with blend weight w = alpha T, a `BlendStats` table keeps per Gaussian the sum of w, the largest w, the
number of pairs (`hits`) and the number of views with at least one. Floaters, splats buried under opaque surfaces and the doubled
overlap of two merged tiles score low on all four. (The reference's only tool is GaussianModel.prune_by_radius,
scene/gaussian_model.py:752, which sets opacity by distance; it is commented out at render_video.py:239.)

    stats = BlendStats(model.get_xyz.shape[0])
    with recording(stats):                       # the reference's own render() feeds the statistics
        for cam in cameras:
            render(cam, model, pipe, background, kernel_size)
    removed = prune(model, stats, min_weight_max=0.02, min_views=2)

`stats.add(raster_settings, means3D=..., ...)` is the direct form: one inference render of the view (its images are returned)
followed by the statistics kernel on the same blobs. The decisions, T and w are those of the rendered image bit for bit; sums
are integers (floor(w 2^32)), so a table does not depend on the order of tiles or views and two runs give the same bits.
There is no CPU path for `add`; the tables themselves, `keep_mask` and `prune_table` work on any device."""
import contextlib

import numpy as np
import torch

from . import _call
from . import _lib as L

__all__ = ["BlendStats", "recording", "prune", "prune_table"]

Q32 = 2.0 ** -32


def _plain(t):
    """A deferred handle of one of the opt-in hooks (sfgs.prepass / sh / features / viewdirs) as the tensor it stands for."""
    t = t.materialise() if hasattr(t, "materialise") else t
    if isinstance(t, torch.Tensor) and t.dtype == torch.float64:   # a raw opacity after the reference's reset_opacity
        t = t.float()
    return t


class BlendStats:
    """The tables of one scene of `num_gaussians` Gaussians, all zero at first. Read them through the properties."""

    def __init__(self, num_gaussians, device="cuda"):
        n = int(num_gaussians)
        if n < 0:
            raise ValueError(f"num_gaussians must be >= 0, got {n}")
        dev = torch.device(device)
        self.num_gaussians = n
        # (uint64 on the device; their values stay far below 2^63)
        self._sum_q32 = torch.zeros(n, dtype=torch.int64, device=dev)
        self._hits = torch.zeros(n, dtype=torch.int64, device=dev)
        self._hits_seen = torch.zeros(n, dtype=torch.int64, device=dev)
        self._max = torch.zeros(n, dtype=torch.float32, device=dev)
        self._views = torch.zeros(n, dtype=torch.int32, device=dev)
        self.num_views = 0
        self.timing = None   # a list: every add() appends its (start, after the render, after the statistics) CUDA events

    device = property(lambda self: self._hits.device)
    weight_sum = property(lambda self: self._sum_q32.double() * Q32, doc="float64 [N]: sum of w over the blended pairs")
    weight_sum_q32 = property(lambda self: self._sum_q32, doc="int64 [N]: the exact integer sum of floor(w 2^32)")
    weight_max = property(lambda self: self._max, doc="float32 [N]: the largest w")
    hits = property(lambda self: self._hits, doc="int64 [N]: blended (pixel, Gaussian) pairs")
    views = property(lambda self: self._views, doc="int32 [N]: views with at least one blended pair")

    def reset(self):
        for t in (self._sum_q32, self._hits, self._hits_seen, self._max, self._views):
            t.zero_()
        self.num_views = 0

    @torch.no_grad()
    def add(self, raster_settings, *, means3D, scales, rotations, opacities, shs=None, colors_precomp=None, pixel_mask=None,
            means2D=None, cov3Ds_precomp=None):
        """Render one view (inference route, `raster_settings.tile_rows` honoured) and add its pairs to the tables. The
        keyword inputs are GaussianRasterizer.forward's (means2D is accepted and unused). pixel_mask: bool / uint8 [H,W] or
        [1,H,W]; pairs of pixels where it is zero are not counted. Returns (color [3,H,W], depth [1,H,W], alpha [1,H,W])."""
        from . import shard
        if cov3Ds_precomp is not None:
            raise ValueError("cov3Ds_precomp is not supported")
        if scales is None or rotations is None:
            raise ValueError("Please provide scales and rotations")
        inputs = dict(means3D=_plain(means3D), scales=_plain(scales), rotations=_plain(rotations),
                      opacities=_plain(opacities), shs=_plain(shs), colors_precomp=_plain(colors_precomp))
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        _call.check_pixel_mask(pixel_mask, H, W, "pixel_mask")
        n = int(inputs["means3D"].shape[0])
        if n != self.num_gaussians:
            raise ValueError(f"the view has {n} Gaussians, the statistics were set up for {self.num_gaussians}")
        _call.check_gpu(means3D=inputs["means3D"], pixel_mask=pixel_mask)
        dev = inputs["means3D"].device
        _call.same_device(dev, "the Gaussians' device", statistics=self._hits, pixel_mask=pixel_mask)
        lib = L.load()
        mask8 = None
        if pixel_mask is not None:
            mask8 = pixel_mask.contiguous()
            mask8 = mask8.view(torch.uint8) if mask8.dtype == torch.bool else mask8
        events = None
        if self.timing is not None:
            with torch.cuda.device(dev):
                events = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                events[0].record(torch.cuda.current_stream(dev))
        p = shard.plan_frame(raster_settings, inputs)
        frame, stream, cap, ccap = p["frame"], p["stream"], p["cap"], p["ccap"]
        geom, tiles, bins = p["geom"], p["tiles"], p["bins"]
        with torch.cuda.device(dev):
            band = getattr(raster_settings, "tile_rows", None)
            outs = (torch.zeros if band else torch.empty)(5, H, W, dtype=torch.float32, device=dev)
            L.check(lib.sfgs_raster_forward_render(L.C.byref(frame), n, L.ptr(geom), L.ptr(tiles), L.ptr(bins), bins.numel(),
                                                   cap, ccap, -1, L.ptr(outs[0:3]), L.ptr(outs[3:4]), L.ptr(outs[4:5]), None,
                                                   0, stream))
            if events:
                events[1].record(torch.cuda.current_stream(dev))
            tables = L.SfgsBlendStats(L.C.sizeof(L.SfgsBlendStats), n, L.ptr(self._sum_q32), L.ptr(self._hits),
                                      L.ptr(self._max))
            L.check(lib.sfgs_raster_blend_stats(L.C.byref(frame), n, L.ptr(geom), L.ptr(tiles), L.ptr(bins), bins.numel(),
                                                cap, ccap, L.ptr(mask8), L.C.byref(tables), stream))
            L.check(lib.sfgs_blend_stats_views(n, L.ptr(self._hits), L.ptr(self._hits_seen), L.ptr(self._views), stream))
            if events:
                events[2].record(torch.cuda.current_stream(dev))
                self.timing.append(events)
        self.num_views += 1
        self.last_duplicates = p["D"]     # list entries of the view (what the statistics kernel walked at most)
        return outs[0:3], outs[3:4], outs[4:5]

    def keep_mask(self, min_weight_max=0.0, min_weight_sum=0.0, min_hits=0, min_views=0):
        """bool [N]: weight_max >= min_weight_max AND weight_sum >= min_weight_sum AND hits >= min_hits AND views >=
        min_views. A Gaussian that was never blended fails as soon as any threshold is positive."""
        keep = ((self._max >= float(min_weight_max)) & (self.weight_sum >= float(min_weight_sum)) &
                (self._hits >= int(min_hits)) & (self._views >= int(min_views)))
        if min_weight_max > 0 or min_weight_sum > 0 or min_hits > 0 or min_views > 0:
            keep &= self._hits > 0
        return keep


_recording = []   # the one active recording() (the wrapped forward and its original)


@contextlib.contextmanager
def recording(stats, pixel_mask=None):
    """While the context is open every diff_gauss.GaussianRasterizer.forward -- the call inside the reference's render() --
    also does stats.add(self.raster_settings, ...) with the same inputs: a second, inference-only forward per call. The method
    is wrapped on enter and put back on exit. NOT re-entrant: a second recording() inside an open one raises."""
    import diff_gauss
    if _recording:
        raise RuntimeError("sfgs.importance.recording() is not re-entrant: another recording is open")
    cls = diff_gauss.GaussianRasterizer
    original = cls.forward

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3Ds_precomp=None):
        out = original(self, means3D, means2D, opacities, shs=shs, colors_precomp=colors_precomp, scales=scales,
                       rotations=rotations, cov3Ds_precomp=cov3Ds_precomp)
        stats.add(self.raster_settings, means3D=means3D, scales=scales, rotations=rotations, opacities=opacities, shs=shs,
                  colors_precomp=colors_precomp, pixel_mask=pixel_mask)
        return out

    _recording.append(original)
    cls.forward = forward
    try:
        yield stats
    finally:
        cls.forward = original
        _recording.clear()


def _model_count(model):
    xyz = getattr(model, "_xyz", None)
    return int((model.get_xyz if xyz is None else xyz).shape[0])


def prune(model, stats, **criteria):
    """model.prune_points(~stats.keep_mask(**criteria)) -- the reference's method (scene/gaussian_model.py:586; what
    sfgs.compact hooks). Returns the number of Gaussians removed; raises if the model's size changed since the statistics."""
    n = _model_count(model)
    if n != stats.num_gaussians:
        raise ValueError(f"the model has {n} Gaussians, the statistics were taken over {stats.num_gaussians}")
    keep = stats.keep_mask(**criteria)
    removed = int((~keep).sum().item())
    if removed:
        model.prune_points(~keep)
    return removed


def prune_table(rows, keep):
    """rows[keep] for the structured arrays of sfgs.ply (a fused PLY's vertex table, a merged scene): a new array."""
    if isinstance(keep, torch.Tensor):
        keep = keep.detach().cpu().numpy()
    keep = np.asarray(keep)
    if keep.dtype != np.bool_ or keep.ndim != 1:
        raise ValueError("keep must be a 1-D bool mask")
    if rows.ndim != 1 or rows.shape[0] != keep.shape[0]:
        raise ValueError(f"the table has {rows.shape[0] if rows.ndim else 0} rows, the mask {keep.shape[0]}")
    return rows[keep].copy()
