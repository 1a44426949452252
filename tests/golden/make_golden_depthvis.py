#!/usr/bin/env python
"""Golden vectors of the depth colorisation: the reference's OWN colorize_depth_torch, imported from render_video.py and
run on CPU tensors (the function needs no GPU).

Runs only in the authoring container (it imports /root/reference read-only, and needs matplotlib). Third-party modules the
container lacks (plyfile, OpenEXR, Imath, mediapy) are stubbed the way tests/test_reference_imports.py does; diff_gauss,
simple_knn and fused_ssim are this repository's packages.

Recorded per case: depth [H,W], mask [H,W] (when the case has one), normalize, the float32 [3,H,W] result and the two
quantiles np.nanquantile gives on the reference's float32 disparity. Recorded once: the 256 x 3 uint8 table of "Spectral" as
the reference turns colormap output into bytes. The frames come from tests/depthvis_np.py (seeded). Cases: the six content
kinds with and without a mask at 37 x 53, a smooth frame at 135 x 240, NaN / +-inf / denormal depths planted, normalize
off, and the sizes 1 x 1 and 2 x 1.

usage: python tests/golden/make_golden_depthvis.py [--check]     (--check: regenerate and compare with the committed file)
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "reference_depthvis.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depthvis_np as dnp  # noqa: E402


def cases():
    """tag -> (kind, H, W, seed, with mask, normalize)"""
    out = {}
    for i, kind in enumerate(dnp.KINDS):
        for masked in (False, True):
            out[f"{kind}_{'m' if masked else 'n'}"] = (kind, 37, 53, 100 + i, masked, True)
    out["smooth_big_n"] = ("smooth", 135, 240, 201, False, True)
    out["smooth_big_m"] = ("smooth", 135, 240, 201, True, True)
    out["special_n"] = ("special", 37, 53, 301, False, True)
    out["special_m"] = ("special", 37, 53, 302, True, True)
    out["smooth_raw_n"] = ("smooth", 37, 53, 401, False, False)
    out["special_raw_m"] = ("special", 37, 53, 402, True, False)
    out["uniform_1x1_n"] = ("uniform", 1, 1, 501, False, True)
    out["uniform_2x1_n"] = ("uniform", 2, 1, 502, False, True)
    out["uniform_2x1_m"] = ("uniform", 2, 1, 503, True, True)
    return out


def import_reference_function():
    for name in ("plyfile", "OpenEXR", "Imath", "mediapy"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(ROOT, "skyfall-gs_amd"))
    sys.path.insert(0, REF)
    import render_video
    return render_video.colorize_depth_torch


def generate():
    colorize_depth_torch = import_reference_function()
    import matplotlib.pyplot as plt
    out = {"spectral_lut": (plt.get_cmap("Spectral")(np.arange(256)).clip(0, 1) * 255).astype(np.uint8)[:, :3]}
    for tag, (kind, H, W, seed, masked, normalize) in cases().items():
        depth = dnp.make_depth(kind, H, W, seed)
        mask = dnp.make_mask(H, W, seed) if masked else None
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")                  # all-NaN slices, divide by zero
            result = colorize_depth_torch(torch.from_numpy(depth)[None], None if mask is None else torch.from_numpy(mask)[None],
                                          normalize=normalize)
            # the two quantiles numpy gives on the float32 disparity the reference forms (:143-158)
            disp = dnp.disparity(depth, mask)
            lo, hi = np.nanquantile(disp, 0.01), np.nanquantile(disp, 0.99)
        assert result.dtype == torch.float32 and tuple(result.shape) == (3, H, W) and disp.dtype == np.float32
        out[f"{tag}_depth"] = depth
        if mask is not None:
            out[f"{tag}_mask"] = mask
        out[f"{tag}_normalize"] = np.bool_(normalize)
        out[f"{tag}_result"] = result.numpy()
        out[f"{tag}_quantiles"] = np.asarray([lo, hi], dtype=np.float32)
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert set(old.files) == set(out), set(old.files) ^ set(out)
        for k in out:
            np.testing.assert_array_equal(old[k], out[k], err_msg=k)
        print("reference_depthvis.npz reproduced exactly")
        return
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
