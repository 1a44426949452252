"""Float64 numpy oracle of sfgs.resample (include/sfgs.h, "Jittered ground truth"): the yardstick for the ERROR of a float32
evaluation -- the reference's (meshgrid, normalise, grid_sample un-normalises again) and the kernel's (x + ox directly) round
at different points, so neither is "the" answer. Not a restatement of torch: the formula, in float64.

    s = mask * src                               the float32 product the reference forms first (train.py:207) -- data, not error
    u = clamp(x + ox, 0, W - 1), v = clamp(y + oy, 0, H - 1)         NaN and -inf -> 0, +inf -> W - 1 / H - 1
    out[c, y, x] = bilinear interpolation of s[c] at (u, v)          neighbour index clamped (its weight is 0 there)
"""
import numpy as np


def clip64(t, hi):
    """min(hi, max(t, 0)) with max / min that drop a NaN (torch's device clip_coordinates): NaN, -inf -> 0; +inf -> hi."""
    with np.errstate(invalid="ignore"):
        t = np.where(t > 0.0, t, 0.0)
        return np.where(t < hi, t, float(hi))


def resample64(src, offset, mask=None):
    """src: float32 [C,H,W]; offset: float32 [H,W,2] (x, y); mask: None, (1,1,1) or [1,H,W] float32 -> float64 [C,H,W]."""
    src, offset = np.asarray(src, np.float32), np.asarray(offset, np.float32)
    C, H, W = src.shape
    assert offset.shape == (H, W, 2)
    s = src if mask is None else (np.asarray(mask, np.float32) * src).astype(np.float32)
    s = s.astype(np.float64)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u = clip64(xx + offset[..., 0].astype(np.float64), W - 1)
    v = clip64(yy + offset[..., 1].astype(np.float64), H - 1)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = u - x0, v - y0
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    return (s[:, y0, x0] * ((1 - fx) * (1 - fy)) + s[:, y0, x1] * (fx * (1 - fy)) +
            s[:, y1, x0] * ((1 - fx) * fy) + s[:, y1, x1] * (fx * fy))
