"""Per-Gaussian, per-component bound on the rasterizer's backward against the CPU oracle (TEST INFRASTRUCTURE; DESIGN.md
section 8). parity.assert_grad_close judges a gradient tensor as a whole and cannot see a Gaussian whose gradient is small
next to the tensor's largest: this module judges every Gaussian in its OWN float32 error unit.

    |got - ref| <= K[case][tensor] * 2^-23 * unit            per Gaussian, per component

1. The pixel mask. One alpha >= 1/255 or T >= 1e-4 decision that falls the other way under another exponential changes
   the terms of every later entry of that pixel's list, so Gaussians cannot be masked; but every term a pixel adds to any
   gradient is linear in that pixel's upstream gradients. `pixel_mask` marks the pixels with a decision closer than
   DELTA = 2^-16 to its threshold (orc_pixel_margins) and `upstream` zeroes dL/dcolor, dL/ddepth and dL/dalpha there, for
   the oracle and for the implementation under test alike. A margin is relative to how far another float32 evaluation can
   move the tested value: the exponent of a thin, rotated splat is a cancelling sum (sum of |terms| = M in the hundreds,
   |power| < 5.5), so its exponential moves by a few 2^-24 M, not by "a few 1e-6": alpha margins are divided by max(1, M),
   T margins by the sum of alpha_j / (1 - alpha_j) max(1, M_j) over the factors of T. At most MASK_CAP of a case's pixels
   may be masked; a case above it gets another seed (sh1_ragged: 1.13 % at seed 7), never another cap.
2. The unit. orc_backward_ex exports, per Gaussian, the magnitude sums of the RAW per-pair terms (u dx, u dy, u dx^2, ...
   with u = G dL/dalpha as a magnitude: every subtraction inside it adds magnitudes, and G and w count max(1, M, the
   pixel's T factor of 1.) times). The product sums raw terms and applies opacity and conic once (raster_math.h:
   grad2d_from_sums), the oracle applies them per pair: `units` forms the magnitudes of the twelve 2D sums so that they
   bound both, and runs them through raster_chain_np.chain(magnitude=True).
3. K. Measured against references only, never against the implementation under test (`measure`): two calibration builds of
   the oracle (float32 sums in reverse order; every expf scaled by 1 +- 2 * 2^-23 max(1, M)) and the float64 chain against
   the oracle's float32 chain, each in units, under the pixel mask. K = 4 x the largest, rounded up to a power of two: the
   factor covers fused multiply-adds and the product's other association (raw sums, one scalar recurrence), which none of
   the three has. The third measurement is there because the two builds share the oracle's float32 chain instruction for
   instruction: without it the chain tensors' K would not know that a float32 chain rounds at all.

`python tests/grad_bounds.py` re-measures every case and prints the table below.
"""
import math

import numpy as np
import torch

from oracle import oracle as orc
from sfgs.synth import scene, upstream_grads

import camera_cases
import raster_chain_np

DELTA = 2.0 ** -16
MASK_CAP = 0.01
EPS = 2.0 ** -23
TENSORS = ("means3D", "means2D", "scales", "rotations", "opacities", "colors_precomp", "shs")

_PRECOMP_SMALL = dict(n=3000, W=200, H=120, kw=dict(zrange=(4., 8.), scale_range=(0.01, 0.2)))
_BIG_SPLATS = dict(n=400, W=256, H=192, kw=dict(zrange=(3., 6.), scale_range=(0.3, 2.0)))
CASES = {
    "precomp_small": _PRECOMP_SMALL,
    "sh1_ragged": dict(n=5000, W=130, H=77, seed=3, kw=dict(zrange=(2., 50.), scale_range=(0.01, 2.0), mode="sh", sh_degree=1)),
    "sh3_jitter": dict(n=4000, W=160, H=100, kw=dict(zrange=(250., 350.), scale_range=(0.2, 3.0), mode="sh", sh_degree=3,
                                                     jitter=True)),
    "big_splats": _BIG_SPLATS,
    "screen_filling": dict(n=60, W=640, H=400, kw=dict(zrange=(3., 6.), scale_range=(0.5, 3.0), opacity_range=(0.01, 0.05))),
    # every summation route of preprocess_bwd in one frame: <= 32 records, 33 .. 2 048, > 2 048 (chunk heads); translucent,
    # so that the small splats behind the large ones still receive a gradient
    "mixed_coop": dict(n=1200, W=512, H=384, kw=dict(zrange=(3., 60.), scale_range=(0.02, 3.0), opacity_range=(0.02, 0.3))),
    "lists_800": dict(n=900, W=24, H=24, kw=dict(zrange=(3., 6.), scale_range=(0.8, 1.5), opacity_range=(0.006, 0.03))),
    # loss = sum color gc + depth gd + alpha ga, and the same in raw depth mode
    "precomp_small_alpha": dict(_PRECOMP_SMALL, alpha=True),
    "precomp_small_alpha_raw": dict(_PRECOMP_SMALL, alpha=True, depth_mode=1),
    "big_splats_alpha": dict(_BIG_SPLATS, alpha=True),
    "big_splats_alpha_raw": dict(_BIG_SPLATS, alpha=True, depth_mode=1),
}
# general cameras (tests/camera_cases.py builds them: pose, off-centre principal point, splats beyond the Jacobian's guard
# band, depths down to the near cull); clamped_jacobian masks 1.07 % of its pixels at seed 3 and takes seed 4
for _name in ("clamped_jacobian", "near_plane", "pose_offcentre_sh3"):
    CASES[_name] = dict(camera=_name, n=camera_cases.CASES[_name]["n"], W=camera_cases.CASES[_name]["W"],
                        H=camera_cases.CASES[_name]["H"])

# case -> tensor -> (accf, jit, chain64, K): the measured maxima, in units, of the float32-sum build, the exp-jitter build
# and the float64 chain against the oracle (rounded up to three digits); K = 4 x the largest, rounded up to a power of two.
K_TABLE = {
    "precomp_small": {
        "means3D": (0.0632, 0.674, 0.0809, 4),
        "means2D": (0.0955, 0.683, 0.0283, 4),
        "scales": (0.0076, 0.0539, 0.0186, 0.25),
        "rotations": (0.00673, 0.0562, 0.00776, 0.25),
        "opacities": (0.061, 0.513, 0.0276, 4),
        "colors_precomp": (0.571, 1.88, 0.164, 8),
    },
    "sh1_ragged": {
        "means3D": (0.00391, 0.215, 0.00404, 1),
        "means2D": (0.0101, 0.344, 0.0042, 2),
        "scales": (0.000315, 0.0657, 0.000986, 0.5),
        "rotations": (0.000828, 0.0395, 0.000491, 0.25),
        "opacities": (0.00397, 0.757, 0.00416, 4),
        "shs": (0.0562, 1.99, 0.0525, 8),
    },
    "sh3_jitter": {
        "means3D": (0.0872, 9.58, 0.0917, 64),
        "means2D": (0.0621, 9.6, 0.0308, 64),
        "scales": (0.0208, 3.26, 0.048, 16),
        "rotations": (0.041, 2.31, 0.0439, 16),
        "opacities": (0.0695, 9.53, 0.0592, 64),
        "shs": (1.67, 4.49, 2.94, 32),
    },
    "big_splats": {
        "means3D": (0.00268, 0.0198, 0.0016, 0.125),
        "means2D": (0.0159, 0.0684, 0.00328, 0.5),
        "scales": (0.000801, 0.00703, 0.00151, 0.03125),
        "rotations": (0.00041, 0.0047, 0.000628, 0.03125),
        "opacities": (0.00353, 0.133, 0.0052, 1),
        "colors_precomp": (0.0379, 0.758, 0.00741, 4),
    },
    "screen_filling": {
        "means3D": (0.00284, 0.00826, 0.000678, 0.0625),
        "means2D": (0.326, 0.0563, 0.0389, 2),
        "scales": (0.000558, 0.000732, 0.000201, 0.00390625),
        "rotations": (0.000363, 0.00055, 0.00014, 0.00390625),
        "opacities": (0.00348, 0.0112, 0.000399, 0.0625),
        "colors_precomp": (0.0634, 0.0494, 0.00299, 0.5),
    },
    "mixed_coop": {
        "means3D": (0.139, 1.07, 0.151, 8),
        "means2D": (0.279, 1.15, 0.0943, 8),
        "scales": (0.0201, 0.21, 0.0212, 1),
        "rotations": (0.0226, 0.155, 0.0248, 1),
        "opacities": (0.142, 1.22, 0.0466, 8),
        "colors_precomp": (0.437, 2.39, 0.189, 16),
    },
    "lists_800": {
        "means3D": (0.0437, 0.0941, 0.0206, 0.5),
        "means2D": (0.19, 0.136, 0.0288, 1),
        "scales": (0.00354, 0.00915, 0.00717, 0.0625),
        "rotations": (0.00353, 0.00528, 0.00236, 0.03125),
        "opacities": (0.0365, 0.0816, 0.00863, 0.5),
        "colors_precomp": (0.543, 0.804, 0.108, 4),
    },
    "precomp_small_alpha": {
        "means3D": (0.0518, 0.661, 0.08, 4),
        "means2D": (0.0933, 0.668, 0.0303, 4),
        "scales": (0.0124, 0.0591, 0.0196, 0.25),
        "rotations": (0.00625, 0.0566, 0.0103, 0.25),
        "opacities": (0.0544, 0.516, 0.0257, 4),
        "colors_precomp": (0.571, 1.88, 0.164, 8),
    },
    "precomp_small_alpha_raw": {
        "means3D": (0.34, 1.52, 0.385, 8),
        "means2D": (0.422, 1.54, 0.111, 8),
        "scales": (0.0526, 0.182, 0.0629, 1),
        "rotations": (0.0234, 0.109, 0.0305, 0.5),
        "opacities": (0.304, 0.93, 0.111, 4),
        "colors_precomp": (0.571, 1.88, 0.164, 8),
    },
    "big_splats_alpha": {
        "means3D": (0.00351, 0.0246, 0.0026, 0.125),
        "means2D": (0.0123, 0.0794, 0.00348, 0.5),
        "scales": (0.00173, 0.019, 0.00142, 0.125),
        "rotations": (0.000835, 0.00861, 0.000703, 0.0625),
        "opacities": (0.00567, 0.159, 0.00224, 1),
        "colors_precomp": (0.0379, 0.758, 0.00741, 4),
    },
    "big_splats_alpha_raw": {
        "means3D": (0.0132, 0.0964, 0.0079, 0.5),
        "means2D": (0.0442, 0.201, 0.0135, 1),
        "scales": (0.00183, 0.0238, 0.00351, 0.125),
        "rotations": (0.00303, 0.024, 0.00224, 0.125),
        "opacities": (0.0165, 0.329, 0.0166, 2),
        "colors_precomp": (0.0379, 0.758, 0.00741, 4),
    },
    # general pose: the world coordinates (|p| ~ 14) cancel down to view-space ones in every product with the view and
    # projection matrices, so the unit of means3D is large next to its value and the readings, in units, are small
    "clamped_jacobian": {
        "means3D": (0.000199, 0.00261, 0.000463, 0.015625),
        "means2D": (0.0275, 0.0372, 0.00452, 0.25),
        "scales": (0.000261, 0.00161, 0.000192, 0.0078125),
        "rotations": (0.000338, 0.000386, 0.000142, 0.001953125),
        "opacities": (0.0179, 0.0354, 0.00117, 0.25),
        "colors_precomp": (0.0419, 0.804, 0.0268, 4),
    },
    "near_plane": {
        "means3D": (0.000139, 0.0026, 0.000408, 0.015625),
        "means2D": (0.0612, 0.833, 0.0137, 4),
        "scales": (0.0031, 0.0677, 0.00872, 0.5),
        "rotations": (0.00242, 0.0369, 0.00448, 0.25),
        "opacities": (0.0584, 1.78, 0.0204, 8),
        "colors_precomp": (0.135, 2.75, 0.0218, 16),
    },
    "pose_offcentre_sh3": {
        "means3D": (0.000391, 0.00313, 0.000353, 0.015625),
        "means2D": (0.0912, 0.361, 0.0162, 2),
        "scales": (0.00733, 0.0586, 0.0114, 0.25),
        "rotations": (0.00441, 0.0233, 0.00361, 0.125),
        "opacities": (0.0417, 0.317, 0.0315, 2),
        "shs": (0.662, 1.87, 0.673, 8),
    },
}


def k_of(case, tensor):
    return K_TABLE[case][tensor][3]


def choose_k(worst):
    return float(2.0 ** math.ceil(math.log2(max(4.0 * worst, 1e-30))))


def _round_up(v):
    """v rounded up to three significant digits (the table keeps maxima that its own K provably covers)"""
    if v <= 0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(v)) - 2)
    return float(f"{math.ceil(v / q - 1e-9) * q:.3g}")


def make_case(name):
    c = CASES[name]
    if "camera" in c:
        frame, g, _ = camera_cases.case(c["camera"])
    else:
        frame, g = scene(c["n"], c["W"], c["H"], seed=c.get("seed", 7), **c["kw"])
    frame["depth_mode"] = int(c.get("depth_mode", 0))
    return frame, g


def pixel_mask(R):
    """[H,W] bool: pixels with a compositing decision closer than DELTA to its threshold."""
    m = R.pixel_margins()
    return (np.minimum(m[..., 0], m[..., 1]) < DELTA) | (m[..., 2] < DELTA)


def upstream(name, R, mask):
    """(gc, gd, ga) of the case, zero at the masked pixels and, for the normalised depth, where the oracle's depth is NaN.
    ga is None unless the case has the alpha term."""
    c = CASES[name]
    W, H = c["W"], c["H"]
    gc, gd = upstream_grads(W, H, 0)
    gc, gd = gc.clone(), gd.clone()
    ga = None
    if c.get("alpha"):
        ga = torch.randn(1, H, W, generator=torch.Generator().manual_seed(2000)) / (W * H)
    keep = torch.from_numpy(~mask)
    gd[torch.from_numpy(np.isnan(R.depth))] = 0
    gc *= keep
    gd *= keep
    if ga is not None:
        ga *= keep
    return gc, gd, ga


def units(frame, g, R, sums):
    """dict tensor -> float64 array shaped like the gradient: the per-Gaussian, per-component error unit."""
    geom = R.geom().astype(np.float64)
    cA, cB, cC, op = np.abs(geom[:, 2]), np.abs(geom[:, 3]), np.abs(geom[:, 4]), np.abs(geom[:, 5])
    W, H = float(frame["W"]), float(frame["H"])
    m = sums[:, 12:]
    mags = np.zeros((sums.shape[0], 12))
    mags[:, 0] = op * 0.5 * W * (cA * m[:, 0] + cB * m[:, 1])
    mags[:, 1] = op * 0.5 * H * (cC * m[:, 1] + cB * m[:, 0])
    # absx = sum |gx_i|: |.| moves by what its argument moves by, and gx_i cancels INSIDE the pair (u = G dL/dalpha_i is a
    # difference): the unit of the x sum, not the sum's own value. (With "its own value" the exp-jitter build moved one
    # Gaussian of sh3_jitter, whose sum |u| is 6e5 times its sum u, by 9.1e5 units.)
    mags[:, 2:4] = mags[:, 0:2]
    mags[:, 4] = 0.5 * op * m[:, 2]
    mags[:, 5] = op * m[:, 3]
    mags[:, 6] = 0.5 * op * m[:, 4]
    mags[:, 7] = m[:, 5]
    mags[:, 8:11] = m[:, 6:9]
    mags[:, 11] = m[:, 9]
    return _chain(frame, g, R, sums[:, :12], mags, True)


def _chain(frame, g, R, sums, mags, magnitude):
    f = {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in frame.items() if v is not None}
    shs = None if g["shs"] is None else g["shs"].numpy()
    return raster_chain_np.chain(f, g["means3D"].numpy(), g["scales"].numpy(), g["rotations"].numpy(),
                                 g["opacities"].numpy(), shs, R.chain_state(), R.radii > 0, sums, mags, magnitude)


_REF = {}


def reference(name):
    """The oracle's side of a case, computed once per process and shared: frame, Gaussians, masked upstream gradients,
    gradients G, units, the float64 chain's gradients, mask share. Callers must not modify it."""
    if name in _REF:
        return _REF[name]
    frame, g = make_case(name)
    R = orc.OracleRender(frame, **g)
    mask = pixel_mask(R)
    gc, gd, ga = upstream(name, R, mask)
    G = R.backward(gc, gd, ga, export=True)
    sums = G.pop("_sums")
    ref = dict(name=name, frame=frame, g=g, R=R, mask=mask, share=float(mask.mean()), gc=gc, gd=gd, ga=ga, G=G, sums=sums,
               unit=units(frame, g, R, sums), chain64=_chain(frame, g, R, sums[:, :12], None, False))
    _REF[name] = ref
    return ref


_COUNTS = {}


def record_counts(name):
    """[N] int32: per Gaussian, the number of 8x8 tiles the product bins it into (host emulation, tests/hostcheck.py) = the
    number of gradient records the backward sums for it; decides its summation route in preprocess_bwd."""
    if name not in _COUNTS:
        import hostcheck
        frame, g = make_case(name)
        h = hostcheck.render(frame, g["means3D"], g["scales"], g["rotations"], g["opacities"], g["colors_precomp"], g["shs"])
        _COUNTS[name] = h["dup_counts"]
    return _COUNTS[name]


def has_gradient(name):
    """[N] bool: Gaussians with a non-zero reference gradient"""
    r = reference(name)
    return np.abs(r["G"]["means2D"]).max(axis=1) > 0


def route_of(count):
    return "none" if count == 0 else "lds (<= 32)" if count <= 32 else "wave stride (33 .. 2048)" if count <= 2048 else "chunk heads (> 2048)"


def in_units(got, ref, unit):
    """[N] float64: per Gaussian, the largest |got - ref| / (2^-23 unit) over its components (0 / 0 = 0, x / 0 = inf)."""
    N = ref.shape[0]
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).reshape(N, -1)
    u = (EPS * np.asarray(unit, np.float64)).reshape(N, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d == 0, 0.0, d / u)
    return e.max(axis=1) if e.shape[1] else np.zeros(N)


def variant_gradients(name, variant):
    r = reference(name)
    Rv = orc.OracleRender(r["frame"], variant=variant, **r["g"])
    return Rv.backward(r["gc"], r["gd"], r["ga"])


def measure(name):
    """tensor -> (accf, jit, chain64): the reference-only maxima that K is chosen from."""
    r = reference(name)
    cols = [variant_gradients(name, "accf"), variant_gradients(name, "jit"), r["chain64"]]
    return {k: tuple(float(in_units(c[k], r["G"][k], r["unit"][k]).max()) for c in cols) for k in r["G"]}


def detectable(name):
    """(detected, total): of the Gaussians with a non-zero reference gradient, how many would violate the bound in some
    tensor if their row were zero."""
    r = reference(name)
    N = r["R"].N
    nonzero = np.zeros(N, bool)
    seen = np.zeros(N, bool)
    for k, ref in r["G"].items():
        a = np.abs(ref.astype(np.float64)).reshape(N, -1)
        nonzero |= (a > 0).any(axis=1)
        seen |= (a > k_of(name, k) * EPS * r["unit"][k].reshape(N, -1)).any(axis=1)
    return int((seen & nonzero).sum()), int(nonzero.sum())


if __name__ == "__main__":
    import sys
    for case in (sys.argv[1:] or list(CASES)):
        ref_ = reference(case)
        m_ = ref_["R"].pixel_margins()
        print(f"# {case}: masked {ref_['share']:.4%} (alpha {np.mean(m_[..., 0] < DELTA):.4%}, T {np.mean(m_[..., 1] < DELTA):.4%}, "
              f"power {np.mean(m_[..., 2] < DELTA):.4%})")
        print(f'    "{case}": {{')
        for t_, v_ in measure(case).items():
            v_ = tuple(_round_up(x_) for x_ in v_)
            print(f'        "{t_}": ({v_[0]:g}, {v_[1]:g}, {v_[2]:g}, {choose_k(max(v_)):g}),')
        print("    },")
