#!/usr/bin/env python
"""Golden vectors of the training loss: the reference's OWN utils.loss_utils.l1_loss and ssim, driven by the statements
of train.py:205-234 (mask products, L1 + D-SSIM, the NaN / Inf scrub of the depth pair, the Pearson depth term).

Runs only in the authoring container (it imports /root/reference read-only). train.py itself cannot be imported (it
instantiates MoGe at import), so its loss statements are restated around the two imported functions; torchmetrics is
absent here, so pearson_corrcoef is spelled with torchmetrics' formula (_pearson_corrcoef_compute for one update), as
make_golden_r3.py does.

Two cases with a binary [1,H,W] mask and NaN / Inf planted in the depth pair; recorded: the inputs, the four scalars and
autograd's image.grad and depth.grad. tests/test_gpu_loss.py replays them into sfgs.loss.training_loss on the GPU.

usage: python tests/golden/make_golden_loss.py [--check]     (--check: regenerate and compare with the committed file)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "reference_loss.npz")

CASES = {  # tag: (C, H, W, lambda_dssim, lambda_depth, seed)
    "a": (3, 45, 65, 0.2, 0.5, 11),      # one past a 32 x 22 tile in both directions
    "b": (3, 22, 32, 0.25, 1.0, 12),     # exactly one tile
}


def pearson_corrcoef(preds, target):
    """torchmetrics.functional.regression.pearson_corrcoef for one update of [P,1] inputs."""
    preds, target = preds.squeeze(), target.squeeze()
    n = preds.shape[0]
    mx, my = preds.mean(), target.mean()
    var_x = ((preds - mx) * (preds - mx)).sum() / (n - 1)
    var_y = ((target - my) * (target - my)).sum() / (n - 1)
    corr_xy = ((preds - mx) * (target - my)).sum() / (n - 1)
    return torch.clamp(corr_xy / (var_x * var_y).sqrt(), -1.0, 1.0)


def depth_loss_func(gt_depth, depth):   # train.py:970-973
    return (1 - pearson_corrcoef(gt_depth, depth)).mean()


def train_loss(l1_loss, ssim, image, depth, original_image, original_depth, mask, lambda_dssim, lambda_depth):
    """train.py:205-234 (resample_gt_image and use_lpips_loss off); fused_ssim is the reference's ssim by contract."""
    gt_image = mask * original_image
    gt_depth = mask * original_depth
    image = mask * image
    depth = mask * depth
    Ll1 = l1_loss(image, gt_image)
    ssim_value = ssim(image, gt_image)
    loss = (1.0 - lambda_dssim) * Ll1 + lambda_dssim * (1.0 - ssim_value)
    depth_loss = 0.0
    gt_depth = gt_depth.reshape(-1, 1)
    depth = depth.reshape(-1, 1)
    nan_inf_mask = torch.isnan(depth) | torch.isinf(depth) | torch.isnan(gt_depth) | torch.isinf(gt_depth)
    depth[nan_inf_mask] = 0.0
    gt_depth[nan_inf_mask] = 0.0
    depth_loss += depth_loss_func(gt_depth, depth)
    loss += lambda_depth * depth_loss
    return loss, Ll1, ssim_value, depth_loss


def generate():
    sys.path.insert(0, REF)
    from utils.loss_utils import l1_loss, ssim
    out = {}
    for tag, (C, H, W, lam, lamd, seed) in CASES.items():
        g = torch.Generator().manual_seed(seed)
        gt_image = torch.rand(C, H, W, generator=g)
        image = (gt_image + 0.1 * torch.randn(C, H, W, generator=g)).clamp(0, 1)
        gt_depth = 400.0 + 20.0 * torch.randn(1, H, W, generator=g)
        depth = 0.9 * gt_depth + 6.0 * torch.randn(1, H, W, generator=g) + 7.0
        mask = (torch.rand(1, H, W, generator=g) < 0.75).float()
        depth.view(-1)[torch.rand(H * W, generator=g) < 0.03] = float("nan")
        depth.view(-1)[5] = float("inf")
        gt_depth.view(-1)[17] = float("-inf")
        gt_depth.view(-1)[H * W - 3] = float("nan")
        image.requires_grad_(True)
        depth.requires_grad_(True)
        loss, Ll1, ssim_value, depth_loss = train_loss(l1_loss, ssim, image, depth, gt_image, gt_depth, mask, lam, lamd)
        image_grad, = torch.autograd.grad((1.0 - lam) * Ll1 + lam * (1.0 - ssim_value), image, retain_graph=True)
        loss.backward()
        f32 = lambda t: t.detach().numpy().astype(np.float32)
        out.update({f"{tag}_image": f32(image), f"{tag}_gt_image": f32(gt_image), f"{tag}_depth": f32(depth),
                    f"{tag}_gt_depth": f32(gt_depth), f"{tag}_mask": f32(mask),
                    f"{tag}_lambda_dssim": np.float64(lam), f"{tag}_lambda_depth": np.float64(lamd),
                    f"{tag}_loss": f32(loss), f"{tag}_Ll1": f32(Ll1), f"{tag}_ssim": f32(ssim_value),
                    f"{tag}_depth_loss": f32(depth_loss),
                    f"{tag}_image_grad": f32(image_grad),            # of the photometric part of the loss
                    f"{tag}_depth_grad": f32(depth.grad)})
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert set(old.files) == set(out), set(old.files) ^ set(out)
        for k in out:
            np.testing.assert_array_equal(old[k], out[k], err_msg=k)
        print("reference_loss.npz reproduced exactly")
        return
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
