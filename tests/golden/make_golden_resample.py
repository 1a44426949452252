#!/usr/bin/env python
"""Golden vectors of the jittered ground truth: the reference's create_offset_gt (train.py:64-77) on mask * original_image
(train.py:207), around torch's OWN grid_sample on the CPU.

train.py cannot be imported (it instantiates MoGe at import), so, as make_golden_loss.py does, its statements are restated
here: lines 64-77 minus `.cuda()`, and line 207. Nothing of the reference tree is read.

Three cases; recorded: the inputs and the reference's float32 output.
    a: C = 3, 45 x 65, offsets U(-0.5, 0.5) (what train.py:190 draws), a binary [1,H,W] mask
    b: C = 1, 33 x 130, offsets U(-3, 3): all four borders clamp; no mask (Camera.original_mask of such a view: ones (1,1,1))
    c: C = 4, 2 x 2, offsets U(-0.5, 0.5), no mask: the smallest frame the reference's division by W - 1, H - 1 allows
The file comes to about 150 kB: uniform random floats do not compress (the three cases hold 37 k float32 values).
tests/test_resample_host.py compares them with the float64 oracle (tests/resample_np.py); tests/test_gpu_resample.py replays
them into sfgs.resample.resample_gt on the GPU.

usage: python tests/golden/make_golden_resample.py [--check]     (--check: regenerate and compare with the committed file)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_resample.npz")

CASES = {  # tag: (C, H, W, offset half-range, binary mask plane?, seed)
    "a": (3, 45, 65, 0.5, True, 31),
    "b": (1, 33, 130, 3.0, False, 32),
    "c": (4, 2, 2, 0.5, False, 33),
}


@torch.no_grad()
def create_offset_gt(image, offset):   # train.py:64-77, minus .cuda()
    height, width = image.shape[1:]
    meshgrid = np.meshgrid(range(width), range(height), indexing='xy')
    id_coords = np.stack(meshgrid, axis=0).astype(np.float32)
    id_coords = torch.from_numpy(id_coords)

    id_coords = id_coords.permute(1, 2, 0) + offset
    id_coords[..., 0] /= (width - 1)
    id_coords[..., 1] /= (height - 1)
    id_coords = id_coords * 2 - 1

    image = torch.nn.functional.grid_sample(image[None], id_coords[None], align_corners=True, padding_mode="border")[0]
    return image


def generate():
    out = {}
    for tag, (C, H, W, half, plane, seed) in CASES.items():
        g = torch.Generator().manual_seed(seed)
        original_image = torch.rand(C, H, W, generator=g)
        offset = (torch.rand(H, W, 2, generator=g) - 0.5) * (2.0 * half)
        mask = (torch.rand(1, H, W, generator=g) < 0.75).float() if plane else torch.ones(1, 1, 1)
        gt_image = mask * original_image                      # train.py:207 (the ones of a view without a mask change nothing)
        gt_image = create_offset_gt(gt_image, offset)         # train.py:215
        f32 = lambda t: t.detach().numpy().astype(np.float32)
        out.update({f"{tag}_image": f32(original_image), f"{tag}_offset": f32(offset), f"{tag}_out": f32(gt_image)})
        if plane:
            out[f"{tag}_mask"] = f32(mask)
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert set(old.files) == set(out), set(old.files) ^ set(out)
        for k in out:
            np.testing.assert_array_equal(old[k], out[k], err_msg=k)
        print("reference_resample.npz reproduced exactly")
        return
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
