"""sfgs.metrics -- the evaluation pass of training_report (reference train.py:1058-1097) on HIP kernels (csrc/metrics.hip
through libsfgs.so): per view, the two clamps, `l1_loss(image, gt_image).mean().double()`, `psnr(image, gt_image).mean().double()`
(utils/image_utils.py:17-19) and, next to them, the SSIM of utils/loss_utils.py:33-63 in TWO launches, with no host read of
a device value.

    row = view_metrics(image, gt_image)          # device float64 [8]: l1, psnr, ssim, mse, psnr_c0 .. psnr_c3

    ev = Evaluator(len(cameras))                 # a device float64 [capacity, 8] table
    for viewpoint in cameras:
        ev.add(render_pkg["render"], viewpoint.original_image)      # two launches, no synchronisation
    r = ev.result()                              # ONE device-to-host copy: r["l1"], r["psnr"], r["ssim"], their _std, ...

`l1` and `mse` are means over all elements, `psnr_c` is 20 log10(1 / sqrt(mse_c)) of plane c in float64, `psnr` the mean of
the planes' values (what `psnr(...).mean()` is), `ssim` the mean of the SSIM map (NaN with ssim=False: then a streaming
kernel replaces the tiled one). Planes beyond C are NaN. An identical pair gives +inf, a NaN in a plane gives NaN, as the
reference's statements do.

psnr() and mse() are drop-ins for utils.image_utils.psnr and mse; install(train_module) rebinds exactly the name `psnr` in
the module that holds training_report, uninstall(train_module) restores it.

There is no torch fallback: without the HIP library every operator raises."""
import numpy as np
import torch

from . import _call
from . import _lib as L

__all__ = ["view_metrics", "Evaluator", "psnr", "mse", "install", "uninstall", "ROW"]

ROW = ("l1", "psnr", "ssim", "mse", "psnr_c0", "psnr_c1", "psnr_c2", "psnr_c3")
_L1, _PSNR, _SSIM, _MSE, _PLANE0 = 0, 1, 2, 3, 4


def _check_pair(image, gt_image):
    _call.check_tensor("image", image, "[C,H,W] with 1 <= C <= 4", lambda t: t.dim() == 3 and t.numel() > 0 and t.shape[0] <= 4)
    _call.check_tensor("gt_image", gt_image, f"{tuple(image.shape)} like image", lambda t: t.shape == image.shape)
    return tuple(int(v) for v in image.shape)


def _check_row(out):
    _call.check_tensor("out", out, "a contiguous [8]", lambda t: tuple(t.shape) == (8,) and t.is_contiguous(),
                       dtypes=(torch.float64,), none_ok=True)


def _run(a, b, P, H, W, flags, row):
    """One library call: the metrics of the contiguous pair a, b (P planes of H x W) into the 8 doubles of `row`."""
    lib = L.load()
    dev = a.device
    args = L.SfgsMetricsArgs(L.C.sizeof(L.SfgsMetricsArgs), P, H, W, a.data_ptr(), b.data_ptr(), int(flags), 0)
    with torch.cuda.device(dev):
        scratch = _call.scratch(lib.sfgs_metrics_scratch_bytes(L.C.byref(args)), dev, refused_if_zero=True)
        L.check(lib.sfgs_metrics_view(L.C.byref(args), L.ptr(row), L.ptr(scratch), scratch.numel(), _call.stream(dev)))
    return row


def _flags(clamp, ssim):
    return (L.METRICS_CLAMP if clamp else 0) | (L.METRICS_SSIM if ssim else 0)


def view_metrics(image, gt_image, clamp=True, ssim=True, out=None):
    """-> device float64 [8]: l1, psnr, ssim, mse, psnr_c0 .. psnr_c3 of clamp(image, 0, 1) against clamp(gt_image, 0, 1)
    (clamp=False: of the tensors as they are). image, gt_image: float32 [C,H,W] on the GPU, 1 <= C <= 4. Two launches, no
    synchronisation. out: a float64 [8] tensor on the same device to write into (it is returned)."""
    Cc, H, W = _check_pair(image, gt_image)
    _check_row(out)
    _call.check_gpu(image=image, gt_image=gt_image)
    _call.same_device(image.device, "image's device", out=out)
    row = torch.empty(8, dtype=torch.float64, device=image.device) if out is None else out
    return _run(image.detach().contiguous(), gt_image.detach().contiguous(), Cc, H, W, _flags(clamp, ssim), row)


class Evaluator:
    """The accumulators of one evaluation loop: a device float64 [capacity, 8] table, one row per view. The row counter
    lives on the host; nothing is read back before result()."""

    def __init__(self, capacity, device=None):
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer, got {capacity!r}")
        self.capacity = capacity
        self.device = None if device is None else torch.device(device)   # None: the first view's device
        if self.device is not None and self.device.type != "cuda":
            raise ValueError(f"device must be a GPU, got {self.device}")
        self.n = 0
        self._table = None   # allocated by the first add(): constructing an Evaluator touches no device

    def add(self, image, gt_image, clamp=True, ssim=True):
        """Write the next row: view_metrics(image, gt_image, clamp, ssim). Two launches, no synchronisation. Views may
        differ in size. ValueError when the table is full."""
        Cc, H, W = _check_pair(image, gt_image)
        if self.n >= self.capacity:
            raise ValueError(f"the Evaluator is full: capacity {self.capacity}")
        _call.check_gpu(image=image, gt_image=gt_image)
        if self._table is None:
            self._table = torch.empty((self.capacity, 8), dtype=torch.float64, device=self.device or image.device)
        _call.same_device(self._table.device, "the Evaluator's device", image=image)
        _run(image.detach().contiguous(), gt_image.detach().contiguous(), Cc, H, W, _flags(clamp, ssim), self._table[self.n])
        self.n += 1

    def result(self):
        """One device-to-host copy of the filled rows -> {"n", "l1", "psnr", "ssim" (means over the views: what
        training_report prints), "l1_std", "psnr_std", "ssim_std" (population std, np.std), "per_view" ([n,8] float64)}."""
        n = self.n
        per_view = np.empty((0, 8), np.float64) if n == 0 else self._table[:n].cpu().numpy()
        res = {"n": n, "per_view": per_view}
        with np.errstate(invalid="ignore"):   # inf - inf in the std of a set with an identical pair
            for k, name in ((_L1, "l1"), (_PSNR, "psnr"), (_SSIM, "ssim")):
                col = per_view[:, k]
                res[name] = float(col.mean()) if n else float("nan")
                res[name + "_std"] = float(col.std()) if n else float("nan")
        return res

    def reset(self):
        self.n = 0


def _stream_planes(name1, img1, name2, img2):
    """The checks of the two drop-ins -> (planes, elements per plane)."""
    _call.check_tensor(name1, img1, "a non-empty tensor of at least one dimension", lambda t: t.dim() >= 1 and t.numel() > 0)
    _call.check_tensor(name2, img2, f"{tuple(img1.shape)} like {name1}", lambda t: t.shape == img1.shape)
    if img1.shape[0] > 4:
        raise ValueError(f"{name1} must have at most 4 planes (shape[0]), got {tuple(img1.shape)}")
    _call.check_gpu(**{name1: img1, name2: img2})
    return int(img1.shape[0]), img1.numel() // int(img1.shape[0])


def _per_plane(img1, img2, flags):
    P, n = _stream_planes("img1", img1, "img2", img2)
    row = torch.empty(8, dtype=torch.float64, device=img1.device)
    _run(img1.detach().contiguous(), img2.detach().contiguous(), P, 1, n, flags, row)
    return row[_PLANE0:_PLANE0 + P].to(torch.float32).view(P, 1)


def psnr(img1, img2):
    """utils.image_utils.psnr: 20 log10(1 / sqrt(mse)) per plane (shape[0] <= 4 of them) -> float32 [shape[0], 1]. The
    streaming kernel, no clamp; the value is formed in float64 and rounded once."""
    return _per_plane(img1, img2, 0)


def mse(img1, img2):
    """utils.image_utils.mse: mean (img1 - img2)^2 per plane -> float32 [shape[0], 1]."""
    return _per_plane(img1, img2, L.METRICS_PLANE_MSE)


_hook = _call.NameHook(psnr=psnr)


def install(train_module):
    """Rebind `psnr` in the namespace of the module that holds training_report (it looks the name up in the module's
    globals when it calls it). A second install is a no-op; nothing else is patched."""
    _hook.install(train_module)


def uninstall(train_module):
    """Restore what install() replaced. Without an install: a no-op."""
    _hook.uninstall(train_module)
