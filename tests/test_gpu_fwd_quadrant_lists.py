"""composite_fwd's per-quadrant entry lists (one list per DPP row = one 4x4 quadrant of the 8x8 tile, entries tested on
their x AND y extent): the lane-to-pixel map, the four ballots and the hit-mask word order are the only things that
differ from the row-pair strips, so the tests sit where those can go wrong -- ragged right / bottom tiles, lists of
several 64-entry batches with tiles that saturate, and splats on and next to the quadrant seams (x, y = 3 | 4 inside a
tile), each on the pixel grid and with a jittered sub-pixel tensor (the quadrant bounds widen by the tensor's bound).

Every case goes through diff_gauss like tests/test_gpu_raster.py (run_hip). The reference is the CPU oracle behind
tests/oracle_backend.py, driven through the same diff_gauss entry on CPU tensors, under tests/parity.py's bars. The
route-equality checks are HIP vs HIP and exact: the training forward against the no-grad forward (two instantiations of
the kernel, two list walks), gradients with the dead-entry prefill forced on and off (the backward reads the hit-mask
words the forward stored per PIXEL SLOT 8 y + x), and for the long lists the tile order forced on and off."""
import math

import numpy as np
import pytest
import torch

import oracle_backend
import parity
from sfgs.synth import scene, upstream_grads
from test_gpu_raster import run_hip

pytestmark = pytest.mark.gpu


def _ragged():
    """37x29: tiles 4 (x) and 3 (y) are cut after 5 columns / 5 rows -- the right quadrants hold one column, the bottom ones one row"""
    W, H = 37, 29
    _, g = scene(300, W, H, seed=31, zrange=(3., 6.), scale_range=(0.02, 0.4))
    return W, H, g, []


def _long_lists():
    """64x64, 3 000 splats of 1 .. 12 pixels: ~150 .. 400 entries per tile (several batches, both 32-entry halves); every
    fourth splat opaque, so that pixels -- and whole tiles -- saturate long before their list ends"""
    W, H = 64, 64
    _, g = scene(3000, W, H, seed=32, zrange=(3., 6.), scale_range=(0.05, 0.6))
    g["opacities"][::4] = 0.99
    return W, H, g, []


def _seams():
    """24x16 (3 x 2 tiles; quadrant seams between columns 3|4, 11|12, 19|20 and rows 3|4, 11|12), hand-placed splats"""
    W, H = 24, 16
    frame, _ = scene(1, W, H, seed=33)
    z = 5.0
    px_per_unit = W / (2.0 * frame["tanfovx"]) / z     # a scale of s world units is s * px_per_unit pixels of sigma

    def at(px, py):   # world position that projects to the pixel coordinate (px, py): pix = ((ndc + 1) W - 1) / 2
        return [((2 * px + 1) / W - 1) * frame["tanfovx"] * z, ((2 * py + 1) / H - 1) * frame["tanfovy"] * z, z]
    ident = [1., 0., 0., 0.]
    diag = [math.cos(math.pi / 8), 0., 0., math.sin(math.pi / 8)]      # 45 degrees about the view axis
    s = lambda sx, sy=None: [sx / px_per_unit, (sx if sy is None else sy) / px_per_unit, 0.01]
    rows = [  # position, scales (pixels of sigma), rotation, opacity
        (at(3.5, 3.5), s(0.8), ident, 0.7),      # exactly on the seam corner of tile (0, 0): all four quadrants
        (at(11.5, 6.0), s(0.5), ident, 0.8),     # on the vertical seam of tile (1, 0), inside the bottom quadrants
        (at(18.0, 11.5), s(0.5), ident, 0.8),    # on the horizontal seam of tile (2, 1)
        (at(3.0, 10.0), s(0.25), ident, 0.9),    # one pixel left of a vertical seam, too small to cross it ...
        (at(4.0, 13.0), s(0.25), ident, 0.9),    # ... and one pixel right of it
        (at(3.0, 14.0), s(1.2), ident, 0.6),     # the same two columns, large enough to cross
        (at(4.0, 9.0), s(1.2), ident, 0.6),
        (at(15.0, 3.0), s(0.25), ident, 0.9),    # one pixel above / below a horizontal seam
        (at(14.0, 4.0), s(0.25), ident, 0.9),
        (at(21.0, 3.0), s(1.2), ident, 0.6),
        (at(22.0, 4.0), s(1.2), ident, 0.6),
        (at(12.0, 8.0), s(4.0, 0.15), diag, 0.9),   # thin and diagonal through the common corner of four tiles: its
                                                    # bounding box covers quadrants that the ellipse itself misses
        (at(19.5, 11.5), s(0.6), ident, float("nan")),   # NaN opacity: infinite extents, kept by every list
        (at(12.0, 8.0), s(9.0), ident, 0.05),     # a faint one over the whole image, behind nothing in particular
    ]
    g = dict(means3D=torch.tensor([r[0] for r in rows], dtype=torch.float32),
             scales=torch.tensor([r[1] for r in rows], dtype=torch.float32),
             rotations=torch.tensor([r[2] for r in rows], dtype=torch.float32),
             opacities=torch.tensor([[r[3]] for r in rows], dtype=torch.float32),
             colors_precomp=torch.rand(len(rows), 3, generator=torch.Generator().manual_seed(34)), shs=None)
    g["means3D"][:, 2] += torch.linspace(0., 0.5, len(rows))   # distinct depths: one order
    return W, H, g, [12]    # row 12 is the NaN-opacity splat


CASES = {"ragged_37x29": _ragged, "long_lists_64x64": _long_lists, "seams_24x16": _seams}
_built = {}


def _case(name, jitter):
    """inputs and the oracle's results, computed once per (case, jitter) and never modified"""
    key = (name, jitter)
    if key in _built:
        return _built[key]
    W, H, g, poisoned = CASES[name]()
    frame, _ = scene(1, W, H, seed=35, jitter=jitter)     # the camera every case uses (+ the jittered sample points)
    if jitter:
        assert float(frame["subpix"].abs().max()) > 0.25   # bound > 0: the quadrant bounds really widen
    gc, gd = upstream_grads(W, H, 6)
    from diff_gauss import GaussianRasterizationSettings, GaussianRasterizer
    settings = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=frame["tanfovx"], tanfovy=frame["tanfovy"], kernel_size=frame["kernel_size"],
        subpixel_offset=frame["subpix"], bg=frame["bg"], scale_modifier=frame["scale_modifier"], viewmatrix=frame["view"],
        projmatrix=frame["proj"], sh_degree=frame["sh_degree"], campos=frame["campos"], prefiltered=False, debug=False)
    t = {k: (v.clone().requires_grad_(True) if v is not None else None) for k, v in g.items()}
    means2D = torch.zeros_like(t["means3D"], requires_grad=True)
    with oracle_backend.installed():
        color, depth, _, alpha, radii, _ = GaussianRasterizer(settings)(
            means3D=t["means3D"], means2D=means2D, shs=None, colors_precomp=t["colors_precomp"], opacities=t["opacities"],
            scales=t["scales"], rotations=t["rotations"], cov3Ds_precomp=None)
        gd = gd.clone()
        gd[torch.isnan(depth.detach())] = 0
        ((color * gc).sum() + (torch.nan_to_num(depth, nan=0.0) * gd).sum()).backward()
        R = oracle_backend.OracleBackend.last
    ref = dict(color=color.detach().numpy(), depth=depth.detach().numpy(), alpha=alpha.detach().numpy(),
               radii=radii.numpy(), grads={k: v.grad.numpy() for k, v in t.items() if v is not None},
               max_tile_list=int(R.max_tile_list))
    ref["grads"]["means2D"] = means2D.grad.numpy()
    _built[key] = (frame, g, gc, gd, ref, poisoned)
    return _built[key]


def _same_bits(a, b, keys, what):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("jitter", [False, True], ids=["grid", "jitter"])
@pytest.mark.parametrize("name", list(CASES))
def test_quadrant_lists_against_the_oracle_and_across_routes(name, jitter, sfgs_option):
    frame, g, gc, gd, ref, poisoned = _case(name, jitter)
    if name == "long_lists_64x64":
        assert ref["max_tile_list"] > 128, ref["max_tile_list"]      # several batches per tile
        a8 = ref["alpha"].reshape(8, 8, 8, 8).transpose(0, 2, 1, 3).reshape(64, 64)
        assert (a8.min(axis=1) > 0.98).any()                           # at least one tile whose every pixel is opaque
    out = run_hip(frame, g, gc, gd, debug=False)
    # 1. the oracle, parity.py's bars
    np.testing.assert_array_equal(out["radii"], ref["radii"])
    reps = [parity.assert_image_close(k, out[k], ref[k]) for k in ("color", "alpha", "depth")]
    keep = np.ones(len(ref["radii"]), bool)
    keep[poisoned] = False    # the NaN-opacity splat's OWN gradient is NaN (dL/dG = opacity x ...) in the oracle as well
    for k, G in ref["grads"].items():
        assert np.isfinite(G[keep]).all(), k
        reps.append(parity.assert_grad_close(k, out["grads"][k][keep], G[keep]))
    print(name, jitter, out["counters"], reps)
    assert np.abs(ref["grads"]["means3D"][keep]).max() > 0
    # 2. the training forward (hit masks, 32-entry halves) and the no-grad forward (64-entry walk): the same bits
    with torch.no_grad():
        plain = run_hip(frame, g, backward=False, debug=False)
    _same_bits({k: np.nan_to_num(out[k], nan=-1.0) for k in ("color", "depth", "alpha")},
               {k: np.nan_to_num(plain[k], nan=-1.0) for k in ("color", "depth", "alpha")}, ("color", "depth", "alpha"),
               "training vs no-grad forward")
    # 3. the backward over the forward's hit masks, dead entries zeroed one by one / skipped through the live flags
    grads = {}
    for mode in ("always", "never"):
        sfgs_option("prefill", mode)
        grads[mode] = run_hip(frame, g, gc, gd, debug=False)["grads"]
    sfgs_option("prefill", "auto")
    for k in grads["always"]:
        np.testing.assert_array_equal(grads["always"][k], grads["never"][k], err_msg=f"prefill always vs never: {k}")
        np.testing.assert_array_equal(grads["always"][k], out["grads"][k], err_msg=f"prefill always vs auto: {k}")
    # 4. long lists: tiles taken longest list first or in image order
    if name == "long_lists_64x64":
        outs = {}
        for mode in ("never", "always"):
            sfgs_option("tile_order", mode)
            outs[mode] = run_hip(frame, g, gc, gd, debug=False)
        for k in ("color", "depth", "alpha", "radii"):
            np.testing.assert_array_equal(np.nan_to_num(outs["never"][k], nan=-1.0), np.nan_to_num(outs["always"][k], nan=-1.0),
                                          err_msg=f"tile order: {k}")
        for k in outs["never"]["grads"]:
            np.testing.assert_array_equal(outs["never"]["grads"][k], outs["always"]["grads"][k], err_msg=f"tile order: {k}")
