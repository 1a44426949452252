#!/usr/bin/env python
"""Golden vectors of the evaluation pass: the reference's OWN utils.image_utils.psnr (and mse), utils.loss_utils.l1_loss and
ssim, driven by the statements of training_report (train.py:1064,1075,1090-1093): clamp both images to [0, 1],
`l1_loss(image, gt_image).mean().double()`, `psnr(image, gt_image).mean().double()`, accumulate over the views, divide.

Runs only in the authoring container (it imports /root/reference read-only; train.py itself cannot be imported, it
instantiates MoGe at import, so the loop body is restated around the imported functions). Everything runs on the CPU.

Cases: (3,45,65) with values outside [0, 1] on both operands (the clamp matters), (3,22,32) (exactly one 32 x 22 tile),
(1,23,33), an identical pair (PSNR +inf), a pair with one NaN pixel in channel 1, and a set of three views of different
sizes with its per-view values and the two means training_report prints. Recorded per case: the two inputs, l1, psnr
(float64, as the `.double()` leaves them), the per-plane psnr and mse (float32) and ssim (float32).
tests/test_metrics_host.py holds the float64 restatement to them, tests/test_gpu_metrics.py the kernels.

usage: python tests/golden/make_golden_metrics.py [--check]     (--check: regenerate and compare with the committed file)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "reference_metrics.npz")

CASES = {  # tag: (C, H, W, seed, kind)
    "clamp": (3, 45, 65, 21, "wide"),       # one past a 32 x 22 tile in both directions; values in about [-0.3, 1.3]
    "tile": (3, 22, 32, 22, "plain"),       # exactly one tile
    "gray": (1, 23, 33, 23, "plain"),
    "same": (3, 24, 40, 24, "same"),        # identical pair: mse = 0, PSNR = +inf
    "nan": (3, 30, 44, 25, "nan"),          # one NaN pixel in channel 1
}
VIEWS = ((3, 45, 65, 31), (3, 33, 70, 32), (3, 58, 36, 33))   # the three-view set


def make_pair(C, H, W, seed, kind):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(C, H, W, generator=g)
    image = gt + 0.1 * torch.randn(C, H, W, generator=g)
    if kind == "wide":
        gt = 1.6 * gt - 0.3
        image = 1.6 * image - 0.3
    elif kind == "same":
        image = gt.clone()
    elif kind == "nan":
        image[1, H // 2, W // 3] = float("nan")
    return image, gt


def report_view(fns, render, original_image):
    """The loop body of training_report for one view -> (l1, psnr) as it accumulates them, and the extras."""
    l1_loss, psnr, mse, ssim = fns
    image = torch.clamp(render, 0.0, 1.0)
    gt_image = torch.clamp(original_image, 0.0, 1.0)
    l1 = l1_loss(image, gt_image).mean().double()
    p = psnr(image, gt_image)
    return l1, p.mean().double(), p, mse(image, gt_image), ssim(image[None], gt_image[None])


def generate():
    sys.path.insert(0, REF)
    from utils.image_utils import mse, psnr
    from utils.loss_utils import l1_loss, ssim
    fns = (l1_loss, psnr, mse, ssim)
    out = {}

    def record(tag, image, gt):
        l1, p, p_c, m_c, s = report_view(fns, image, gt)
        out.update({f"{tag}_image": image.numpy().astype(np.float32), f"{tag}_gt_image": gt.numpy().astype(np.float32),
                    f"{tag}_l1": np.float64(l1.item()), f"{tag}_psnr": np.float64(p.item()),
                    f"{tag}_psnr_c": p_c.numpy().astype(np.float32).reshape(-1),
                    f"{tag}_mse_c": m_c.numpy().astype(np.float32).reshape(-1), f"{tag}_ssim": np.float32(s.item())})
        return l1, p

    for tag, (C, H, W, seed, kind) in CASES.items():
        record(tag, *make_pair(C, H, W, seed, kind))
    l1_test, psnr_test = 0.0, 0.0                       # train.py:1060-1061
    for i, (C, H, W, seed) in enumerate(VIEWS):
        l1, p = record(f"view{i}", *make_pair(C, H, W, seed, "wide" if i == 1 else "plain"))
        l1_test += l1
        psnr_test += p
    psnr_test /= len(VIEWS)
    l1_test /= len(VIEWS)
    out["views_l1_test"] = np.float64(l1_test.item())
    out["views_psnr_test"] = np.float64(psnr_test.item())
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert set(old.files) == set(out), set(old.files) ^ set(out)
        for k in out:
            np.testing.assert_array_equal(old[k], out[k], err_msg=k)
        print("reference_metrics.npz reproduced exactly")
        return
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
