"""Per-element bounds on the model-side kernels (prepass / act_math.h, eval_sh, Adam, densify_stats) against float64
references (TEST INFRASTRUCTURE; numpy and torch-CPU only, imports nothing of the product).

    |got - ref| <= K[op][tensor] * eps * unit            per element

1. The reference evaluates the reference project's statements (scene/gaussian_model.py:207-249, utils/sh_utils.py:57-112,
   torch/optim/adam.py::_multi_tensor_adam, scene/gaussian_model.py:744-749) in float64 from the inputs as they are (Adam:
   in long double, because a float64 tensor's chain is float64 itself).
2. The unit of an element follows the rule of tests/grad_bounds.py: the same expression with the magnitudes of all terms
   added, every subtraction counted as a sum of magnitudes. A product of positive terms is its own unit.
3. K is measured against references only, never against the HIP kernels: the largest error, in units, of a float32
   restatement (prepass: the closed forms rounded where torch's promotion rules round; eval_sh: the reference's evaluation
   order in torch float32; Adam: oracle/adam_np.adam_step) against the float64 reference, on the inputs the GPU tests use.
   K = 4 x that maximum, rounded up to a power of two: the 4 covers fused multiply-adds and the device's expf / exp / sqrt
   against libm, which no CPU restatement has.
eps is 2^-23 wherever a float32 intermediate enters (everything of the prepass, also its float64 opacity gradient: sq and
det1 are float32) and 2^-52 where the whole chain is float64 (Adam on a float64 tensor).

`python tests/model_ops_ref.py` re-measures K_TABLE and prints it.
"""
import math

import numpy as np
import torch

EPS32 = 2.0 ** -23
EPS64 = 2.0 ** -52
F32_TINY = float(np.finfo(np.float32).tiny)
NORM_EPS = float(np.float32(1e-12))     # F.normalize's clamp as a float32 tensor meets it
BLOCK_NS = (1, 255, 256, 257, 4099)     # around the 256-thread block, and one odd multi-block size
MEASURE_N = 8209
MEASURE_SEED, SECOND_SEED = 1, 2

# op -> tensor -> (measured maxima in units ..., K). prepass: the four (filter dtype, raw opacity dtype) routes in the
# order of SFGS_ACT_DISPATCH (f32/f32, f64/f32, f32/f64, f64/f64); eval_sh: unit directions, norms 0.1 .. 10;
# adam: adam_step in float32, the same statements in float64 (eps = 2^-52).
K_TABLE = {
    "prepass": {
        "scales": (1.67, 1.78, 1.67, 1.78, 8),
        "opacity": (3.57, 3.95, 2.99, 3.05, 16),
        "rotation": (1.34, 1.34, 1.34, 1.34, 8),
        "g_scaling": (3.45, 3.12, 3.24, 2.78, 16),
        "g_opacity": (2.86, 3.64, 2.49, 2.53, 16),
        "g_rotation": (3.41, 3.41, 3.41, 3.41, 16),
    },
    "eval_sh": {
        "out": (1.97, 3.53, 16),
        "g_sh": (2.27, 2.14, 16),
        "g_dirs": (2.13, 1.92, 16),
    },
    "adam": {
        "p": (3.82, 1.72, 16),
        "m": (1.46, 1.61, 8),
        "v": (2.15, 2.26, 16),
    },
}


def k_of(op, tensor):
    return K_TABLE[op][tensor][-1]


def choose_k(worst):
    return float(2.0 ** math.ceil(math.log2(max(4.0 * worst, 1e-30))))


def _round_up(v):
    """v rounded up to three significant digits (the table keeps maxima that its own K provably covers)"""
    if v <= 0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(v)) - 2)
    return float(f"{math.ceil(v / q - 1e-9) * q:.3g}")


def in_units(got, ref, unit, eps=EPS32):
    """elementwise |got - ref| / (eps unit) in float64 (0 / 0 = 0, x / 0 = inf, a non-finite difference = inf)"""
    got, ref = np.asarray(got).astype(np.float64), np.asarray(ref).astype(np.float64)
    d = np.abs(got - ref)
    u = eps * np.broadcast_to(np.asarray(unit).astype(np.float64), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d == 0, 0.0, d / u)
    return np.where(np.isfinite(d), e, np.inf)


def worst(got, ref, unit, eps=EPS32):
    e = in_units(got, ref, unit, eps)
    return float(e.max()) if e.size else 0.0


# ---- prepass (csrc/prepass.hip, csrc/act_math.h) ---------------------------------------------------------------------
ROUTES = ((np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64))


def quaternion_cases():
    """[M,4] float32: exact zero; norm 1e-13 (below F.normalize's clamp); norms 1e-3 .. 1e3; one component dominating."""
    rng = np.random.default_rng(11)
    rows = [np.zeros(4)]
    for _ in range(4):
        q = rng.normal(size=4)
        rows.append(q / np.linalg.norm(q) * 1e-13)
    for e in np.linspace(-3.0, 3.0, 25):
        q = rng.normal(size=4)
        rows.append(q / np.linalg.norm(q) * 10.0 ** e)
    for i in range(4):
        for big, small in ((1.0, 1e-4), (1e3, 1e-3), (1.0, 0.0)):
            q = rng.normal(size=4) * small
            q[i] = big if i % 2 == 0 else -big
            rows.append(q)
    return np.asarray(rows, np.float32)


def prepass_inputs(n, seed, ft=np.float64, ot=np.float32):
    """The wide-range inputs of the prepass tests: log-scales uniform in [-12, 4], log-filter uniform in [-8, 1], raw
    opacity ~ N(0, 4^2), quaternions of norm 1e-3 .. 1e3 (the rows of quaternion_cases() first, as far as n allows), and
    float32 upstream gradients ~ N(0, 1). The three generators are independent of the dtypes."""
    rng = np.random.default_rng(seed)
    scaling = rng.uniform(-12.0, 4.0, size=(n, 3)).astype(np.float32)
    filt = np.exp(rng.uniform(-8.0, 1.0, size=(n, 1))).astype(ft)
    opacity = (rng.normal(size=(n, 1)) * 4.0).astype(ot)
    q = rng.normal(size=(n, 4))
    q *= 10.0 ** rng.uniform(-3.0, 3.0, size=(n, 1)) / np.linalg.norm(q, axis=1, keepdims=True)
    rotation = q.astype(np.float32)
    special = quaternion_cases()[:n]
    rotation[:special.shape[0]] = special
    up = dict(g_scales=rng.normal(size=(n, 3)).astype(np.float32), g_opacity=rng.normal(size=(n, 1)).astype(np.float32),
              g_rotation=rng.normal(size=(n, 4)).astype(np.float32))
    return dict(scaling=scaling, opacity=opacity, rotation=rotation, filt=filt, **up)


def _prepass_terms64(scaling, opacity, filt):
    f8 = np.float64
    s = np.exp(scaling.astype(f8))
    sq = s * s
    f2 = np.square(filt.astype(f8)).reshape(-1, 1)
    t = sq + f2
    coef = np.sqrt(sq.prod(axis=1, keepdims=True) / t.prod(axis=1, keepdims=True))
    o = 1.0 / (1.0 + np.exp(-opacity.astype(f8).reshape(-1, 1)))
    return sq, f2, t, coef, o


def _zeros_like_up(a, shape):
    return np.zeros(shape, np.float64) if a is None else np.asarray(a).astype(np.float64)


def prepass_ref(scaling, opacity, rotation, filt, g_scales=None, g_opacity=None, g_rotation=None):
    """float64 reference and units. Returns (ref, unit): dicts with scales / opacity / rotation and, with respect to the
    RAW parameters, g_scaling / g_opacity / g_rotation for the loss sum(scales g_scales + opacity g_opacity + rotation
    g_rotation); an upstream gradient that is None is absent (zero)."""
    n = scaling.shape[0]
    sq, f2, t, coef, o = _prepass_terms64(scaling, opacity, filt)
    q = rotation.astype(np.float64)
    nrm = np.sqrt((q * q).sum(axis=1, keepdims=True))
    den = np.maximum(nrm, NORM_EPS)
    ref = dict(scales=np.sqrt(t), opacity=o * coef, rotation=q / den)
    unit = dict(scales=ref["scales"], opacity=ref["opacity"], rotation=np.abs(q) / den)
    gs, go, gr = _zeros_like_up(g_scales, (n, 3)), _zeros_like_up(g_opacity, (n, 1)), _zeros_like_up(g_rotation, (n, 4))
    ref["g_scaling"] = gs * sq / np.sqrt(t) + go * o * coef * f2 / t
    unit["g_scaling"] = np.abs(gs) * sq / np.sqrt(t) + np.abs(go) * o * coef * f2 / t
    ref["g_opacity"] = go * coef * o * (1.0 - o)
    unit["g_opacity"] = np.abs(go) * coef * o     # not times (1 - o): 1 - o is formed from a ROUNDED o, here and in torch
    h = q / den
    clamped = nrm <= NORM_EPS                     # d normalize = g / eps where the clamp is active
    ref["g_rotation"] = np.where(clamped, gr / den, (gr - h * (h * gr).sum(axis=1, keepdims=True)) / den)
    unit["g_rotation"] = np.where(clamped, np.abs(gr) / den,
                                  (np.abs(gr) + np.abs(h) * (np.abs(h) * np.abs(gr)).sum(axis=1, keepdims=True)) / den)
    return ref, unit


def prepass_f32(scaling, opacity, rotation, filt, g_scales=None, g_opacity=None, g_rotation=None):
    """The float32 restatement K is measured with: the closed forms, rounded where torch's promotion rules round
    (act_math.h: sq and det1 float32, t / det2 / coef in the filter's dtype, the sigmoid in the raw opacity's dtype, the
    gradients in double from those rounded terms and rounded once to the parameter's dtype)."""
    f4, f8 = np.float32, np.float64
    ft, ot = filt.dtype.type, opacity.dtype.type
    n = scaling.shape[0]
    s = np.exp(scaling.astype(f4))
    sq = (s * s).astype(f4)
    det1 = ((sq[:, 0] * sq[:, 1]).astype(f4) * sq[:, 2]).astype(f4).reshape(-1, 1)
    f = filt.reshape(-1, 1)
    f2 = (f * f).astype(ft)
    t = (sq.astype(ft) + f2).astype(ft)
    det2 = ((t[:, 0] * t[:, 1]).astype(ft) * t[:, 2]).astype(ft).reshape(-1, 1)
    coef = np.sqrt((det1.astype(ft) / det2).astype(ft)).astype(ft)
    raw_o = opacity.reshape(-1, 1)
    o = (ot(1) / (ot(1) + np.exp(-raw_o).astype(ot)).astype(ot)).astype(ot)
    out = dict(scales=np.sqrt(t).astype(ft).astype(f4))
    if ot is np.float64:
        out["opacity"] = (o * coef.astype(f8)).astype(f4)
    else:
        out["opacity"] = (o.astype(ft) * coef).astype(ft).astype(f4)
    q = rotation.astype(f4)
    nn = np.sqrt((q * q).sum(axis=1, keepdims=True, dtype=f4)).astype(f4)
    out["rotation"] = (q / np.maximum(nn, f4(1e-12))).astype(f4)
    gs, go, gr = _zeros_like_up(g_scales, (n, 3)), _zeros_like_up(g_opacity, (n, 1)), _zeros_like_up(g_rotation, (n, 4))
    c8, o8, t8 = coef.astype(f8), o.astype(f8), t.astype(f8)
    out["g_opacity"] = (go * c8 * o8 * (1.0 - o8)).astype(ot)
    out["g_scaling"] = (gs * sq.astype(f8) / np.sqrt(t8) + go * o8 * c8 * f2.astype(f8) / t8).astype(f4)
    g4 = gr.astype(f4)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (f4(1) / nn).astype(f4)
        h = (q * inv).astype(f4)
        dot = (h * g4).sum(axis=1, keepdims=True, dtype=f4)
        free = ((g4 - h * dot) * inv).astype(f4)
    out["g_rotation"] = np.where(nn > f4(1e-12), free, g4 * f4(1e12)).astype(f4)
    return out


PREPASS_TENSORS = ("scales", "opacity", "rotation", "g_scaling", "g_opacity", "g_rotation")


def measure_prepass(seed=MEASURE_SEED, n=MEASURE_N):
    """tensor -> the four routes' maxima, in units, of prepass_f32 against prepass_ref"""
    res = {k: [] for k in PREPASS_TENSORS}
    for ft, ot in ROUTES:
        x = prepass_inputs(n, seed, ft, ot)
        ref, unit = prepass_ref(**x)
        got = prepass_f32(**x)
        for k in PREPASS_TENSORS:
            res[k].append(worst(got[k], ref[k], unit[k]))
    return {k: tuple(v) for k, v in res.items()}


def det1_f32(scaling):
    """det1 as act_math.h forms it (float32): the prepass inputs must keep it a normal number"""
    s = np.exp(scaling.astype(np.float32))
    sq = s * s
    return (sq[:, 0] * sq[:, 1]) * sq[:, 2]


# ---- eval_sh (csrc/sh_eval.hip; the real SH basis up to degree 4 with the constants of utils/sh_utils.py) -------------
_C0 = 0.28209479177387814
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435)
_C4 = (2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431,
       -0.6690465435572892, 0.47308734787878004, -1.7701307697799304, 0.6258357354491761)
# basis k = constant * sum of (factor, x power, y power, z power): the polynomials of eval_sh multiplied out, so that the
# value, the partial derivatives and the magnitudes ("every term with a positive sign") come from one table
SH_POLY = (
    (_C0, ((1, 0, 0, 0),)),
    (-_C1, ((1, 0, 1, 0),)), (_C1, ((1, 0, 0, 1),)), (-_C1, ((1, 1, 0, 0),)),
    (_C2[0], ((1, 1, 1, 0),)), (_C2[1], ((1, 0, 1, 1),)), (_C2[2], ((2, 0, 0, 2), (-1, 2, 0, 0), (-1, 0, 2, 0))),
    (_C2[3], ((1, 1, 0, 1),)), (_C2[4], ((1, 2, 0, 0), (-1, 0, 2, 0))),
    (_C3[0], ((3, 2, 1, 0), (-1, 0, 3, 0))), (_C3[1], ((1, 1, 1, 1),)),
    (_C3[2], ((4, 0, 1, 2), (-1, 2, 1, 0), (-1, 0, 3, 0))), (_C3[3], ((2, 0, 0, 3), (-3, 2, 0, 1), (-3, 0, 2, 1))),
    (_C3[4], ((4, 1, 0, 2), (-1, 3, 0, 0), (-1, 1, 2, 0))), (_C3[5], ((1, 2, 0, 1), (-1, 0, 2, 1))),
    (_C3[6], ((1, 3, 0, 0), (-3, 1, 2, 0))),
    (_C4[0], ((1, 3, 1, 0), (-1, 1, 3, 0))), (_C4[1], ((3, 2, 1, 1), (-1, 0, 3, 1))),
    (_C4[2], ((7, 1, 1, 2), (-1, 1, 1, 0))), (_C4[3], ((7, 0, 1, 3), (-3, 0, 1, 1))),
    (_C4[4], ((35, 0, 0, 4), (-30, 0, 0, 2), (3, 0, 0, 0))), (_C4[5], ((7, 1, 0, 3), (-3, 1, 0, 1))),
    (_C4[6], ((7, 2, 0, 2), (-1, 2, 0, 0), (-7, 0, 2, 2), (1, 0, 2, 0))), (_C4[7], ((1, 3, 0, 1), (-3, 1, 2, 1))),
    (_C4[8], ((1, 4, 0, 0), (-6, 2, 2, 0), (1, 0, 4, 0))),
)


def _poly(terms, const, d, magnitude, wrt=None):
    x = np.abs(d) if magnitude else d
    acc = np.zeros(d.shape[0])
    for fac, *pw in terms:
        fac = float(fac)
        if wrt is not None:
            if pw[wrt] == 0:
                continue
            fac *= pw[wrt]
            pw = list(pw)
            pw[wrt] -= 1
        acc += (abs(fac) if magnitude else fac) * x[:, 0] ** pw[0] * x[:, 1] ** pw[1] * x[:, 2] ** pw[2]
    return (abs(const) if magnitude else const) * acc


def sh_basis(deg, dirs, magnitude=False):
    """(B [N,M], dB [N,M,3]) in float64, M = (deg+1)^2; magnitude=True: every term positive, on |x|, |y|, |z|"""
    d = np.asarray(dirs).astype(np.float64)
    m = (deg + 1) ** 2
    B = np.stack([_poly(t, c, d, magnitude) for c, t in SH_POLY[:m]], axis=1)
    dB = np.stack([np.stack([_poly(t, c, d, magnitude, w) for w in range(3)], axis=1) for c, t in SH_POLY[:m]], axis=1)
    return B, dB


def eval_sh_ref(deg, sh, dirs, g_out):
    """float64 reference and units of out [N,3], g_sh [N,3,K] (exact zeros in the unused coefficients), g_dirs [N,3]"""
    sh8, go = sh.astype(np.float64), g_out.astype(np.float64)
    m = (deg + 1) ** 2
    ref, unit = {}, {}
    for mag, dst in ((False, ref), (True, unit)):
        B, dB = sh_basis(deg, dirs, mag)
        s, g = (np.abs(sh8), np.abs(go)) if mag else (sh8, go)
        dst["out"] = np.einsum("nk,nck->nc", B, s[:, :, :m])
        dst["g_sh"] = np.zeros_like(sh8)
        dst["g_sh"][:, :, :m] = B[:, None, :] * g[:, :, None]
        dst["g_dirs"] = np.einsum("nkd,nck,nc->nd", dB, s[:, :, :m], g)
    return ref, unit


def eval_sh_f32(deg, sh, dirs):
    """The reference's eval_sh restated in torch (any float dtype; float32 on the CPU is what K is measured with): the
    factored polynomials, accumulated degree by degree in the reference's order. sh [N,3,K], dirs [N,3] -> [N,3]"""
    r = _C0 * sh[..., 0]
    if deg > 0:
        x, y, z = dirs[..., 0:1], dirs[..., 1:2], dirs[..., 2:3]
        r = r - _C1 * y * sh[..., 1] + _C1 * z * sh[..., 2] - _C1 * x * sh[..., 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        r = (r + _C2[0] * xy * sh[..., 4] + _C2[1] * yz * sh[..., 5] + _C2[2] * (2.0 * zz - xx - yy) * sh[..., 6]
             + _C2[3] * xz * sh[..., 7] + _C2[4] * (xx - yy) * sh[..., 8])
    if deg > 2:
        r = (r + _C3[0] * y * (3 * xx - yy) * sh[..., 9] + _C3[1] * xy * z * sh[..., 10]
             + _C3[2] * y * (4 * zz - xx - yy) * sh[..., 11] + _C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[..., 12]
             + _C3[4] * x * (4 * zz - xx - yy) * sh[..., 13] + _C3[5] * z * (xx - yy) * sh[..., 14]
             + _C3[6] * x * (xx - 3 * yy) * sh[..., 15])
    if deg > 3:
        r = (r + _C4[0] * xy * (xx - yy) * sh[..., 16] + _C4[1] * yz * (3 * xx - yy) * sh[..., 17]
             + _C4[2] * xy * (7 * zz - 1) * sh[..., 18] + _C4[3] * yz * (7 * zz - 3) * sh[..., 19]
             + _C4[4] * (zz * (35 * zz - 30) + 3) * sh[..., 20] + _C4[5] * xz * (7 * zz - 3) * sh[..., 21]
             + _C4[6] * (xx - yy) * (7 * zz - 1) * sh[..., 22] + _C4[7] * xz * (xx - 3 * yy) * sh[..., 23]
             + _C4[8] * (xx * (xx - 3 * yy) - yy * (3 * xx - yy)) * sh[..., 24])
    return r


def eval_sh_f32_all(deg, sh, dirs, g_out):
    """out, g_sh, g_dirs of eval_sh_f32 in float32 on the CPU (autograd for the two gradients)"""
    s = torch.tensor(sh, dtype=torch.float32, requires_grad=True)
    d = torch.tensor(dirs, dtype=torch.float32, requires_grad=True)
    out = eval_sh_f32(deg, s, d)
    (out * torch.tensor(g_out, dtype=torch.float32)).sum().backward()
    g_dirs = d.grad.numpy() if d.grad is not None else np.zeros_like(dirs)
    return dict(out=out.detach().numpy(), g_sh=s.grad.numpy(), g_dirs=g_dirs)


def sh_coeff_counts(deg):
    """stored coefficient counts K of the eval_sh tests: exactly (deg+1)^2, 16 and 25 where they suffice, one odd count"""
    m = (deg + 1) ** 2
    return sorted({m, m + 1} | {k for k in (16, 25) if k >= m})


def sh_inputs(n, k, seed, unit_dirs=True):
    rng = np.random.default_rng(seed)
    sh = rng.normal(size=(n, 3, k)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if not unit_dirs:
        d *= 10.0 ** rng.uniform(-1.0, 1.0, size=(n, 1))
    return dict(sh=sh, dirs=d.astype(np.float32), g_out=rng.normal(size=(n, 3)).astype(np.float32))


SH_TENSORS = ("out", "g_sh", "g_dirs")


def measure_sh(seed=MEASURE_SEED, n=4099):
    """tensor -> (unit directions, norms 0.1 .. 10): maxima over the degrees 0 .. 4 and their coefficient counts"""
    res = {k: [0.0, 0.0] for k in SH_TENSORS}
    for deg in range(5):
        for kk in sh_coeff_counts(deg):
            for j, unit_dirs in enumerate((True, False)):
                x = sh_inputs(n, kk, seed + 100 * deg + kk, unit_dirs)
                ref, unit = eval_sh_ref(deg, **x)
                got = eval_sh_f32_all(deg, **x)
                for k in SH_TENSORS:
                    res[k][j] = max(res[k][j], worst(got[k], ref[k], unit[k]))
    return {k: tuple(v) for k, v in res.items()}


# ---- Adam (csrc/adam.hip): one step of torch/optim/adam.py::_multi_tensor_adam ---------------------------------------
ADAM_STEPS = (1, 2, 10, 1000, 30000)


def adam_scalars(t, lr, beta1=0.9, beta2=0.999):
    """The host scalars as _multi_tensor_adam forms them, in double: (-lr / (1 - b1^t), sqrt(1 - b2^t))"""
    bc1 = 1 - beta1 ** t
    bc2 = 1 - beta2 ** t
    return (lr / bc1) * -1, bc2 ** 0.5


def adam_ref(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """One Adam step (t = the already incremented count) in long double from the inputs as they are. Returns (ref, unit)
    with p / m / v; nothing is modified."""
    L = np.longdouble
    p, g, m, v = (np.asarray(a).astype(L) for a in (p, g, m, v))
    step, bc2s = adam_scalars(t, lr, beta1, beta2)
    w1, w2, b2 = L(1 - beta1), L(1 - beta2), L(beta2)
    gm = np.abs(g)
    if weight_decay != 0:
        g = g + L(weight_decay) * p
        gm = gm + abs(L(weight_decay)) * np.abs(p)
    m1 = m + w1 * (g - m)
    m1u = np.abs(m) + w1 * (gm + np.abs(m))
    v1 = v * b2 + w2 * (g * g)
    v1u = np.abs(v) * b2 + w2 * (gm * gm)     # = v1 without weight decay; with it g' = g + wd p can cancel before it is squared
    d = np.sqrt(v1) / L(bc2s) + L(eps)
    p1 = p + L(step) * (m1 / d)
    p1u = np.abs(p) + abs(L(step)) * np.abs(m1) / d
    return dict(p=p1, m=m1, v=v1), dict(p=p1u, m=m1u, v=v1u)


def adam_f64(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """oracle/adam_np.adam_step's statements on float64 arrays (what torch runs on a float64 parameter)"""
    p, m, v = p.copy(), m.copy(), v.copy()
    if weight_decay != 0:
        g = g + weight_decay * p
    m += (1 - beta1) * (g - m)
    v *= beta2
    v += (1 - beta2) * (g * g)
    step, bc2s = adam_scalars(t, lr, beta1, beta2)
    p += step * (m / (np.sqrt(v) / bc2s + eps))
    return p, m, v


def adam_inputs(n, seed, dtype=np.float32, zeros=0):
    """random p, g, m and v > 0 over several orders of magnitude; the first `zeros` elements have g = m = v = 0 (a Gaussian
    no camera saw: with weight_decay = 0 its parameter must not move)"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=n)
    g = rng.normal(size=n) * 10.0 ** rng.uniform(-4.0, 0.0, size=n)
    m = rng.normal(size=n) * 10.0 ** rng.uniform(-4.0, 0.0, size=n)
    v = np.square(rng.normal(size=n) * 10.0 ** rng.uniform(-4.0, 0.0, size=n)) + 1e-12
    z = min(zeros, n)
    g[:z] = 0
    m[:z] = 0
    v[:z] = 0
    return tuple(a.astype(dtype) for a in (p, g, m, v))


def adam_hyper(i, t=None):
    """Hyper-parameters of tensor i of a multi-tensor case: every tensor its own lr, weight_decay (every third 0) and step"""
    return dict(lr=1e-4 * (1 + i) * 1.37 ** (i % 7), weight_decay=0.0 if i % 3 == 0 else 0.01 * (1 + i % 5),
                t=ADAM_STEPS[i % len(ADAM_STEPS)] if t is None else t, eps=1e-15)


ADAM_TENSORS = ("p", "m", "v")


def measure_adam(seed=MEASURE_SEED, n=4099):
    """tensor -> (adam_step in float32, the same statements in float64 at eps = 2^-52), over ADAM_STEPS x two hypers"""
    from oracle.adam_np import adam_step
    res = {k: [0.0, 0.0] for k in ADAM_TENSORS}
    for i, t in enumerate(ADAM_STEPS):
        for j in (1, 3):
            h = adam_hyper(j, t)
            p, g, m, v = adam_inputs(n, seed + 10 * i + j, np.float32, zeros=3 if h["weight_decay"] == 0 else 0)
            ref, unit = adam_ref(p, g, m, v, **h)
            got = adam_step(p.copy(), g, m.copy(), v.copy(), h["t"], h["lr"], eps=h["eps"], weight_decay=h["weight_decay"])
            for k, a in zip(ADAM_TENSORS, got):
                res[k][0] = max(res[k][0], _worst_ld(a, ref[k], unit[k], EPS32))
            p, g, m, v = adam_inputs(n, seed + 10 * i + j, np.float64, zeros=3 if h["weight_decay"] == 0 else 0)
            ref, unit = adam_ref(p, g, m, v, **h)
            got = adam_f64(p, g, m, v, h["t"], h["lr"], eps=h["eps"], weight_decay=h["weight_decay"])
            for k, a in zip(ADAM_TENSORS, got):
                res[k][1] = max(res[k][1], _worst_ld(a, ref[k], unit[k], EPS64))
    return {k: tuple(v) for k, v in res.items()}


def in_units_ld(got, ref, unit, eps):
    """in_units with the difference formed in long double (the float64 route's reference is finer than float64)"""
    L = np.longdouble
    d = np.abs(np.asarray(got).astype(L) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d == 0, L(0), d / (L(eps) * unit))
    return np.where(np.isfinite(d), e, np.inf).astype(np.float64)


def _worst_ld(got, ref, unit, eps):
    e = in_units_ld(got, ref, unit, eps)
    return float(e.max()) if e.size else 0.0


# ---- add_densification_stats (csrc/densify_stats.hip; scene/gaussian_model.py:744-749) -------------------------------
STATS = ("xyz_gradient_accum", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max", "denom")


def densify_stats_ref(bufs, grad, update_filter):
    """float64 result of one call: bufs name -> [N,1] (a missing xyz_gradient_accum_abs_max stays missing); rows with a false
    filter keep their value (the caller compares those bit for bit with what it preloaded)"""
    f = np.asarray(update_filter).astype(bool).reshape(-1)
    g = grad.astype(np.float64)
    out = {k: b.astype(np.float64).copy() for k, b in bufs.items()}
    n2 = np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2)[:, None]
    na = np.abs(g[:, 2:3])
    out["xyz_gradient_accum"][f] += n2[f]
    out["xyz_gradient_accum_abs"][f] += na[f]
    if "xyz_gradient_accum_abs_max" in out:
        out["xyz_gradient_accum_abs_max"][f] = np.maximum(out["xyz_gradient_accum_abs_max"][f], na[f])
    out["denom"][f] += 1
    return out


def ulp32(ref):
    """the float32 spacing at |ref|"""
    return np.spacing(np.abs(np.asarray(ref)).astype(np.float32)).astype(np.float64)


# ---- compute_3D_filter (csrc/filter3d.hip; reference: oracle/filter3d_np.py) -----------------------------------------
FILTER_OFFSET = 1.5e-9       # the threshold probes sit this far (relative) from their threshold: 1e-9 with room for rounding
FILTER_TESTS = ("depth", "left", "right", "top", "bottom")
SQRT02 = 0.2 ** 0.5


def camera(T=(0., 0., 0.), focal=800.0, W=640, H=480, cx=0.0, cy=0.0, R=None):
    return dict(R=np.eye(3) if R is None else np.asarray(R, np.float64), T=np.asarray(T, np.float64), cx=float(cx),
                cy=float(cy), image_width=W, image_height=H, focal_x=float(focal), focal_y=float(focal))


def filter3d_margins(xyz, cam):
    """[N,5] float64: the signed relative distance of every point from the five tests of compute_3D_filter (FILTER_TESTS),
    positive = passes, in the oracle's own statements"""
    p = np.asarray(xyz, np.float64) @ cam["R"] + cam["T"][None, :]
    W, H = cam["image_width"], cam["image_height"]
    z = np.maximum(p[:, 2], 0.001)
    x = p[:, 0] / z * cam["focal_x"] + (cam["cx"] / 2 * W + W / 2)
    y = p[:, 1] / z * cam["focal_y"] + (cam["cy"] / 2 * H + H / 2)
    return np.stack([(p[:, 2] - 0.2) / 0.2, (x + 0.15 * W) / (0.15 * W), (W * 1.15 - x) / (W * 1.15),
                     (y + 0.15 * H) / (0.15 * H), (1.15 * H - y) / (1.15 * H)], axis=1)


def filter3d_threshold_case(test, inside):
    """(xyz [2,3] float32, [camera], seen): a probe point FILTER_OFFSET inside or outside one threshold and an anchor at
    z = 50 that the camera certainly sees. float32 coordinates cannot carry 1e-9: the offset lives in the camera's float64
    T.z (depth) or principal point (screen margins); R is the identity, so the transform adds exact zeros."""
    sgn = 1.0 if inside else -1.0
    W, H, F = 640, 480, 500.0     # F <= 1.3 H keeps the anchor's pixel (the principal point) on the screen in every case
    anchor = [0.0, 0.0, 50.0]
    if test == "depth":
        probe, cam = [0.0, 0.0, 0.25], camera(T=(0., 0., 0.2 * (1 + sgn * FILTER_OFFSET) - 0.25), focal=F, W=W, H=H)
    else:
        horizontal = test in ("left", "right")
        size = W if horizontal else H
        low = test in ("left", "top")
        # probe at -1 / +1 along the axis, z = 1: pixel = -+F + c_ori; place c_ori so that the pixel is at the threshold
        target = -0.15 * size * (1 - sgn * FILTER_OFFSET) if low else 1.15 * size * (1 - sgn * FILTER_OFFSET)
        c_ori = target + F if low else target - F
        c = (c_ori - size / 2) * 2 / size
        a = -1.0 if low else 1.0
        probe = [a, 0.0, 1.0] if horizontal else [0.0, a, 1.0]
        # the anchor sits on the optical axis: its pixel is c_ori itself, which has to be on the screen
        cam = camera(focal=F, W=W, H=H, cx=c if horizontal else 0.0, cy=0.0 if horizontal else c)
    return np.asarray([probe, anchor], np.float32), [cam], bool(inside)


def filter3d_reduce_case(far_block_last, n=262_144 + 300, seed=5):
    """N = 262 444 points = 1 026 blocks of filter3d_min_depth_kernel, so filter3d_reduce_kernel's strided loop takes a second
    round (entries 1 024 and 1 025). Two cameras; every point is seen at a depth in [2, 10] except one at 30 in the last
    block (or block 0), and every 41st point lies behind both cameras and must take that largest seen distance."""
    rng = np.random.default_rng(seed)
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = rng.uniform(-0.2, 0.2, size=n)
    xyz[:, 1] = rng.uniform(-0.2, 0.2, size=n)
    xyz[:, 2] = rng.uniform(2.5, 10.0, size=n)
    xyz[::41, 2] = -5.0
    far = n - 7 if far_block_last else 5
    xyz[far] = (0.0, 0.0, 30.0)
    cams = [camera(T=(0.01, -0.02, 0.0), focal=700.0), camera(T=(-0.03, 0.0, -0.5), focal=800.0, W=800, H=600)]
    return xyz, cams, far


# ---- the table -----------------------------------------------------------------------------------------------------
MEASURES = (("prepass", measure_prepass), ("eval_sh", measure_sh), ("adam", measure_adam))


def measured_table(seed=MEASURE_SEED):
    tab = {}
    for op, fn in MEASURES:
        tab[op] = {}
        for k, v in fn(seed).items():
            v = tuple(_round_up(x) for x in v)
            tab[op][k] = v + (choose_k(max(v)),)
    return tab


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("K_TABLE = {")
    for op_, rows_ in measured_table().items():
        print(f'    "{op_}": {{')
        for t_, v_ in rows_.items():
            print(f'        "{t_}": ({", ".join(f"{x_:g}" for x_ in v_)}),')
        print("    },")
    print("}")
