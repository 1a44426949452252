"""Reference for the per-Gaussian blend-weight statistics (sfgs.importance; TEST INFRASTRUCTURE).

`walk` restates the compositing loop over the oracle's own geom() and tile_lists() in numpy, in FLOAT32 and in list order,
with the oracle's expression for the exponent: T <- T (1 - alpha), w = alpha T. It must be float32: a chain of hundreds of
small-alpha factors rounds at every step, and a float64 restatement is 169 error units away from the oracle's own red sum on
sh3_jitter where the float32 one is 1.1 away. It returns per Gaussian sum w, max w, hits and the error units
    sum u, max u,   u = w max(1, M, t_mag)
with M the sum of the magnitudes of the exponent's terms (orc_power_mag) and t_mag the pixel's sum of
alpha / (1 - alpha) max(1, M) over its blended splats -- how far another float32 exponential moves w (oracle/sfgs_oracle.c).
exp_jitter=n scales every exponential by 1 +- n 2^-23 max(1, M), the oracle's "jit" rule (same hash).

The bound (the project's rule, grad_bounds): per Gaussian |got - ref| <= K 2^-23 unit.
  sum: against the oracle's exported double-precision red sum (backward with dL/dcolor = the unmasked pixels on red,
       _sums[:, 8]) and its unit (_sums[:, 18]), plus hits 2^-32 for the product's truncation to 32 fractional bits;
  max: against the restatement's max w with unit max u.
K comes from references only: the oracle's accf and jit builds against the oracle (sum), the restatement with exp_jitter=2
against the plain one (sum and max); K = grad_bounds.choose_k(largest) = 4 x, rounded up to a power of two. The factor covers
FMA, v_exp_f32 and the product's association. The implementation under test is never an input.

`python tests/importance_np.py` re-measures every case and prints the table below.
"""
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "skyfall-gs_amd")):   # `python tests/importance_np.py` without pytest's conftest
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import oracle as orc  # noqa: E402

import grad_bounds  # noqa: E402

EPS = grad_bounds.EPS
CASES = ("precomp_small", "lists_800", "big_splats", "sh3_jitter", "sh1_ragged")
TILE = 16   # the oracle's tiles

# case -> (sum, max, K): the largest deviation between references, in units (rounded up to three digits), and K
K_TABLE = {
    "precomp_small": (1.5, 2.79, 16),
    "lists_800": (1.26, 3.41, 16),
    "big_splats": (0.495, 2.12, 16),
    "sh3_jitter": (4.03, 4.96, 32),
    "sh1_ragged": (1.98, 2.23, 16),
}


def k_of(case):
    return K_TABLE[case][2]


def _jitter_sign(px, py, k):
    """orc_expf's hash of (pixel, list position): +1 / -1"""
    with np.errstate(over="ignore"):
        h = (px.astype(np.uint32) * np.uint32(2654435761)) ^ (py.astype(np.uint32) * np.uint32(40503)) ^ \
            (np.uint32(k) * np.uint32(2246822519))
        h ^= h >> np.uint32(15)
        h *= np.uint32(2654435761)
        h ^= h >> np.uint32(13)
    return np.where((h & np.uint32(1)) != 0, np.float32(1.0), np.float32(-1.0))


def walk(R, subpix=None, pixel_keep=None, exp_jitter=0, dtype=np.float32):
    """R: an OracleRender. subpix: [H,W,2] float32 or None. pixel_keep: [H,W] bool, pixels whose pairs count (None: all;
    the others still composite). dtype: np.float64 only to reproduce the finding above (the chain must be float32).
    -> dict(sum, max, hits, unit_sum, unit_max), float64 / int64 [N]."""
    f32 = dtype
    geom = R.geom().astype(f32)
    starts, lst = R.tile_lists()
    H, W, N = R.H, R.W, R.N
    TX, TY = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    T = TX * TY
    lens = (starts[1:] - starts[:-1]).astype(np.int64)
    Lmax = int(lens.max()) if T else 0
    # pixels of every tile: [T, 256]
    ty, tx = np.divmod(np.arange(T), TX)
    oy, ox = np.divmod(np.arange(TILE * TILE), TILE)
    px = tx[:, None] * TILE + ox[None, :]
    py = ty[:, None] * TILE + oy[None, :]
    inside = (px < W) & (py < H)
    pxc, pyc = np.minimum(px, W - 1), np.minimum(py, H - 1)
    sx, sy = px.astype(f32), py.astype(f32)
    if subpix is not None:
        sp = np.asarray(subpix, np.float32).astype(f32)
        sx = sx + sp[pyc, pxc, 0]
        sy = sy + sp[pyc, pxc, 1]
    keep = inside if pixel_keep is None else inside & np.asarray(pixel_keep, bool)[pyc, pxc]
    Tr = np.ones((T, TILE * TILE), f32)
    live = inside.copy()
    t_mag = np.zeros((T, TILE * TILE), np.float64)
    steps = []
    for k in range(Lmax):
        rows = np.nonzero(lens > k)[0]
        if not live[rows].any():
            continue
        ids = lst[starts[rows] + k].astype(np.int64)
        g = geom[ids]
        mx, my, ca, cb, cc, op = (g[:, i:i + 1] for i in range(6))
        dx, dy = mx - sx[rows], my - sy[rows]
        power = f32(-0.5) * (ca * dx * dx + cc * dy * dy) - cb * dx * dy
        M = f32(0.5) * (np.abs(ca) * dx * dx + np.abs(cc) * dy * dy) + np.abs(cb * dx * dy)
        with np.errstate(over="ignore", invalid="ignore"):
            G = np.exp(power.astype(np.float64)).astype(f32)   # expf: the correctly rounded float32 exponential
        if exp_jitter:
            G = G * (f32(1.0) + _jitter_sign(px[rows], py[rows], k) * f32(exp_jitter) * f32(1.1920929e-7) * np.maximum(f32(1.0), M))
        with np.errstate(invalid="ignore"):
            alpha = np.minimum(f32(0.99), op * G)
            ok = live[rows] & ~(power > f32(0.0)) & ~(alpha < f32(1.0) / f32(255.0))
            test_T = Tr[rows] * (f32(1.0) - alpha)
            stop = ok & (test_T < f32(0.0001))
        acc = ok & ~stop
        w = np.where(acc, alpha * Tr[rows], f32(0.0)).astype(f32)
        Tr[rows] = np.where(acc, test_T, Tr[rows])
        live[rows] &= ~stop
        a64 = alpha.astype(np.float64)
        t_mag[rows] += np.where(acc, np.maximum(1.0, M.astype(np.float64)) * a64 / (1.0 - a64), 0.0)
        counted = acc & keep[rows]
        if counted.any():
            steps.append((rows, ids, np.where(counted, w, f32(0.0)), M, counted))
    out = dict(sum=np.zeros(N), max=np.zeros(N), hits=np.zeros(N, np.int64), unit_sum=np.zeros(N), unit_max=np.zeros(N))
    for rows, ids, w, M, counted in steps:
        w64 = w.astype(np.float64)
        u = w64 * np.maximum(np.maximum(1.0, M.astype(np.float64)), t_mag[rows])
        np.add.at(out["sum"], ids, w64.sum(axis=1))
        np.add.at(out["hits"], ids, counted.sum(axis=1))
        np.add.at(out["unit_sum"], ids, u.sum(axis=1))
        np.maximum.at(out["max"], ids, w64.max(axis=1))
        np.maximum.at(out["unit_max"], ids, u.max(axis=1))
    return out


def red_upstream(keep):
    """dL/dcolor [3,H,W] = 1 on red at the pixels of `keep`: the oracle's colour gradient on red is then sum_p w."""
    gc = np.zeros((3,) + keep.shape, np.float32)
    gc[0] = keep
    return torch.from_numpy(gc)


def oracle_sum(R, keep):
    """(sum [N], unit [N]) float64: the oracle's exported red sum and its error unit"""
    s = R.backward(red_upstream(keep), None, None, export=True)["_sums"]
    return s[:, 8].copy(), s[:, 18].copy()


_REF = {}


def reference(name):
    """Computed once per process and shared; callers must not modify it: frame, g, R, keep (the pixels that count:
    ~grad_bounds.pixel_mask), share (masked), walk (the restatement), osum / ounit (the oracle's sum and unit)."""
    if name not in _REF:
        frame, g = grad_bounds.make_case(name)
        R = orc.OracleRender(frame, **g)
        mask = grad_bounds.pixel_mask(R)
        keep = ~mask
        subpix = None if frame.get("subpix") is None else frame["subpix"].numpy()
        osum, ounit = oracle_sum(R, keep)
        _REF[name] = dict(name=name, frame=frame, g=g, R=R, keep=keep, share=float(mask.mean()), subpix=subpix,
                          walk=walk(R, subpix, keep), osum=osum, ounit=ounit)
    return _REF[name]


_JIT = {}


def walk_jitter(name, n=2):
    if (name, n) not in _JIT:
        r = reference(name)
        _JIT[(name, n)] = walk(r["R"], r["subpix"], r["keep"], exp_jitter=n)
    return _JIT[(name, n)]


def in_units(got, ref, unit):
    return grad_bounds.in_units(np.asarray(got)[:, None], np.asarray(ref)[:, None], np.asarray(unit)[:, None])


def measure(name):
    """(sum, max): the largest deviation between references, in units."""
    r = reference(name)
    devs = []
    for variant in ("accf", "jit"):
        Rv = orc.OracleRender(r["frame"], variant=variant, **r["g"])
        devs.append(float(in_units(oracle_sum(Rv, r["keep"])[0], r["osum"], r["ounit"]).max()))
    j = walk_jitter(name)
    devs.append(float(in_units(j["sum"], r["walk"]["sum"], r["ounit"]).max()))
    dmax = float(in_units(j["max"], r["walk"]["max"], r["walk"]["unit_max"]).max())
    return max(devs), dmax


def bounds(name):
    """(sum tolerance [N], max tolerance [N]) of the case's GPU comparison"""
    r = reference(name)
    K = k_of(name)
    return K * EPS * r["ounit"] + r["walk"]["hits"] * 2.0 ** -32, K * EPS * r["walk"]["unit_max"]


if __name__ == "__main__":
    import sys
    for case in (sys.argv[1:] or CASES):
        r_ = reference(case)
        w_ = r_["walk"]
        s_, m_ = measure(case)
        print(f"# {case}: masked {r_['share']:.4%}; restatement against the oracle's sum "
              f"{in_units(w_['sum'], r_['osum'], r_['ounit']).max():.3g} units; unit sums rel "
              f"{np.abs(w_['unit_sum'] - r_['ounit']).max() / max(r_['ounit'].max(), 1e-300):.3g}; never blended "
              f"{int((w_['hits'] == 0).sum())} of {r_['R'].N}; longest list {r_['R'].max_tile_list}")
        s_, m_ = grad_bounds._round_up(s_), grad_bounds._round_up(m_)
        print(f'    "{case}": ({s_:g}, {m_:g}, {grad_bounds.choose_k(max(s_, m_)):g}),')
