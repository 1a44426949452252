"""Test infrastructure (the product does not import this): the reference's colorize_depth_torch (render_video.py:129-170)
restated in numpy as a plain float32 sequence with EXACT order statistics -- what csrc/depthvis.hip has to reproduce bit for
bit -- and the seeded depth frames the depthvis tests and tests/golden/make_golden_depthvis.py share.

F = float32; every operation below is one IEEE float32 operation:
    disp = F(1) / depth on the valid pixels (depth > 0, and the mask), NaN elsewhere
    quantile q of the n sorted valid disparities v: vi = F(n - 1) * F(q), i = floor(vi), g = vi - i, a = v[i],
        b = v[min(i + 1, n - 1)], d = b - a, r = a + d * g, and r = b - d * (1 - g) when g >= 0.5; NaN when n == 0
        (how numpy 2.x evaluates nanquantile(..., method="linear") on a float32 array)
    x = 1 - (disp - lo) / (hi - lo)   (normalize off: x = 1 - disp)
    t = x * F(256); k = 255 if t == 256, 0 if t < 0, 255 if t >= 256, else trunc(t); NaN -> (0, 0, 0)
    uint8 pixel = lut[k]; float result = F(pixel) / F(255)"""
import numpy as np

F = np.float32
KINDS = ("smooth", "uniform", "constant", "zero", "tied", "sparse")


def disparity(depth, mask=None):
    depth = np.asarray(depth, dtype=F)
    valid = depth > 0
    if mask is not None:
        valid = valid & (np.asarray(mask) != 0)
    with np.errstate(divide="ignore", over="ignore"):
        disp = F(1) / np.where(valid, depth, F(1))
    return np.where(valid, disp, F(np.nan)).astype(F)


def quantile(v_sorted, q):
    """v_sorted: the valid disparities in ascending order (float32)."""
    n = v_sorted.size
    if n == 0:
        return F(np.nan)
    vi = F(n - 1) * F(q)
    i = int(np.floor(vi))
    g = vi - F(i)
    a, b = v_sorted[i], v_sorted[min(i + 1, n - 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        r = a + d * g
        if g >= F(0.5):
            r = b - d * (F(1) - g)
    return F(r)


def quantiles(disp):
    v = np.sort(disp[~np.isnan(disp)])
    return quantile(v, 0.01), quantile(v, 0.99)


def colour_index(x):
    """-> int64 index per element, -1 for NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * F(256)
        k = np.full(t.shape, -1, dtype=np.int64)
        inside = (t >= 0) & (t < 256)
        k[inside] = t[inside].astype(np.int64)
        k[t < 0] = 0
        k[t >= 256] = 255
    return k


def colorize(depth, lut, mask=None, normalize=True):
    """-> (uint8 [H,W,3], lo, hi); lo / hi are NaN-free only with normalize and a valid pixel. lut: uint8 [256,3]."""
    disp = disparity(depth, mask)
    lo = hi = F(np.nan)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if normalize:
            lo, hi = quantiles(disp)
            x = F(1) - (disp - lo) / (hi - lo)
        else:
            x = F(1) - disp
    assert x.dtype == F
    k = colour_index(x)
    rgb = np.asarray(lut, dtype=np.uint8)[np.clip(k, 0, 255)]
    rgb[k < 0] = 0
    return rgb, lo, hi


def to_float_chw(rgb8):
    """The reference's return value: uint8 / 255 in float32, [3,H,W]."""
    return np.ascontiguousarray((rgb8.astype(F) / F(255)).transpose(2, 0, 1))


def quantize_frame(image):
    """render_video.py:264 on a [3,H,W] float32 frame -> uint8 [H,W,3]; NaN -> 0."""
    img = np.asarray(image, dtype=F).transpose(1, 2, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (img * F(255) + F(0.5)).astype(F)
        t = np.where(np.isnan(t), F(0), t).clip(0, 255)
    return np.ascontiguousarray(t.astype(np.uint8))


def make_depth(kind, H, W, seed):
    """A seeded float32 [H,W] depth frame of one of KINDS (plus "special": smooth with NaN, +-inf, denormal and huge depths
    planted; "few": 40 valid pixels)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind in ("smooth", "special"):
        d = 60.0 + 25.0 * np.sin(xx / max(W, 2) * 5.0) + 15.0 * np.cos(yy / max(H, 2) * 3.0) + 0.5 * rng.standard_normal((H, W))
        d[rng.random((H, W)) < 0.05] = 0.0                 # holes: nothing rendered
        d[rng.random((H, W)) < 0.01] = -3.0
        if kind == "special":
            flat = d.reshape(-1)
            picks = rng.choice(flat.size, size=min(10, flat.size), replace=False)
            values = [np.nan, np.inf, -np.inf, 1e-42, 3e38, 1e-30, np.nan, np.inf, 2.5e-39, 1e30]
            for p, v in zip(picks, values):
                flat[p] = v
    elif kind == "uniform":
        d = rng.uniform(0.5, 200.0, (H, W))
    elif kind == "constant":
        d = np.full((H, W), 7.25)
    elif kind == "zero":
        d = np.zeros((H, W))
    elif kind == "tied":
        d = rng.integers(1, 6, (H, W)).astype(np.float64) * 2.5
    elif kind == "sparse":                                   # 0.1 % valid (at least one pixel)
        d = np.zeros((H, W))
        flat = d.reshape(-1)
        picks = rng.choice(flat.size, size=max(1, flat.size // 1000), replace=False)
        flat[picks] = rng.uniform(1.0, 100.0, picks.size)
    elif kind == "few":                                      # fewer than 64 valid pixels: less than one wave's worth
        d = np.zeros((H, W))
        flat = d.reshape(-1)
        picks = rng.choice(flat.size, size=min(40, flat.size), replace=False)
        flat[picks] = rng.uniform(1.0, 100.0, picks.size)
    else:
        raise ValueError(kind)
    with np.errstate(over="ignore"):
        return d.astype(F)


def make_mask(H, W, seed, keep=0.7):
    return np.random.default_rng(seed + 1000).random((H, W)) < keep
