"""The evaluation metrics of sfgs.metrics in float64 numpy: what the kernels and the reference's float32 statements are both
measured against ("oracle64"). Written from the definitions: mean |a - b|, mean (a - b)^2 per plane, 20 log10(1 / sqrt(mse)),
and SSIM with an 11 x 11 Gaussian window (sigma 1.5), zero padding, C1 = 0.01^2, C2 = 0.03^2."""
import numpy as np

ROW = ("l1", "psnr", "ssim", "mse", "psnr_c0", "psnr_c1", "psnr_c2", "psnr_c3")


def clamp01(x):
    """torch.clamp(x, 0, 1) on an array: NaN stays NaN."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))


def gaussian_window(size=11, sigma=1.5):
    k = np.arange(size, dtype=np.float64) - size // 2
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return g / g.sum()


def blur(x, w):
    """Separable 'same' correlation with zero padding over the last two axes."""
    r = len(w) // 2
    H, W = x.shape[-2:]
    p = np.zeros(x.shape[:-2] + (H + 2 * r, W + 2 * r), dtype=np.float64)
    p[..., r:r + H, r:r + W] = x
    h = sum(w[k] * p[..., :, k:k + W] for k in range(len(w)))
    return sum(w[k] * h[..., k:k + H, :] for k in range(len(w)))


def ssim_map(a, b):
    w = gaussian_window()
    mu1, mu2 = blur(a, w), blur(b, w)
    s1 = blur(a * a, w) - mu1 * mu1
    s2 = blur(b * b, w) - mu2 * mu2
    s12 = blur(a * b, w) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def plane_mse(a, b, clamp=False):
    """-> float64 [P]: mean (a - b)^2 of every plane (axis 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if clamp:
        a, b = clamp01(a), clamp01(b)
    d = (a - b).reshape(a.shape[0], -1)
    return (d * d).mean(axis=1)


def psnr_of_mse(m):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20.0 * np.log10(1.0 / np.sqrt(m))


def view_metrics(a, b, clamp=True, ssim=True):
    """-> float64 [8], in ROW's order, of two [P,H,W] arrays (P <= 4)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if clamp:
        a, b = clamp01(a), clamp01(b)
    P = a.shape[0]
    row = np.full(8, np.nan)
    mse_c = plane_mse(a, b)
    row[0] = np.abs(a - b).mean()
    row[4:4 + P] = psnr_of_mse(mse_c)
    row[1] = row[4:4 + P].mean()
    if ssim:
        with np.errstate(invalid="ignore"):
            row[2] = ssim_map(a, b).mean()
    row[3] = mse_c.mean()          # equal-sized planes: the mean over all elements
    return row


def summarise(per_view):
    """What Evaluator.result() reports from the [n,8] rows: means over the views and population stds."""
    per_view = np.asarray(per_view, dtype=np.float64).reshape(-1, 8)
    out = {"n": per_view.shape[0]}
    with np.errstate(invalid="ignore"):
        for k, name in ((0, "l1"), (1, "psnr"), (2, "ssim")):
            out[name] = float(per_view[:, k].mean())
            out[name + "_std"] = float(per_view[:, k].std())
    return out
