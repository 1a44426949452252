"""Float64 numpy restatement of the rasterizer's per-Gaussian backward chain (the second half of orc_backward in
oracle/sfgs_oracle.c; preprocess_backward_pr in the product's raster_math.h): from the twelve per-Gaussian 2D sums to the
gradients of means3D, means2D, scales, rotations, opacities and the colours. TEST INFRASTRUCTURE.

Every quantity is carried as a pair (v, m):
  v  the value, in float64;
  m  a running magnitude: what v becomes when every subtraction ADDS the magnitudes of its operands. m >= |v| always.
     Rules: (a +- b).m = a.m + b.m ; (a b).m = a.m b.m ; (1 / a).m = a.m / a.v^2 (an error of a moves 1 / a by that
     much over a.v^2) ; an exact input x has m = |x|.
A float32 evaluation of the same expression, in any order of association and with or without fused multiply-adds, differs
from v by a small multiple (about the depth of the expression) of 2^-24 m: m is the error unit of the result. Where the
chain cancels -- det = a c - b^2 of a thin splat, 1 / det^2 behind it -- m is orders of magnitude above |v|, and that is
exactly where two correct float32 implementations disagree.

chain(..., magnitude=False) returns the values: fed with the oracle's double sums it is an independent high-precision
reference of the chain. chain(..., magnitude=True) returns m: fed with the magnitude sums of the raw terms it is the
per-Gaussian, per-component error unit of every gradient tensor (tests/grad_bounds.py).

The forward state the chain reads (a0, b0, c0, the view-space mean, Sigma, coef, the clamp flags) is the oracle's float32
state, taken as exact inputs, and every DECISION (guard-band clamp, the coef guard) is taken in float32 exactly as the
oracle takes it: the chain differentiates the float32 forward that was actually run.
"""
import numpy as np

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)


class V:
    """value + running magnitude (module docstring)"""
    __slots__ = ("v", "m")
    __array_ufunc__ = None   # ndarray * V defers to V.__rmul__

    def __init__(self, v, m=None):
        self.v = np.asarray(v, np.float64)
        self.m = np.abs(self.v) if m is None else np.asarray(m, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.m + o.m)

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, self.m)

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, self.m * o.m)

    __rmul__ = __mul__

    def recip(self):
        return V(1.0 / self.v, self.m / (self.v * self.v))

    def __truediv__(self, o):
        return self * V.of(o).recip()

    def __rtruediv__(self, o):
        return V.of(o) * self.recip()

    def sqrt(self):
        r = np.sqrt(self.v)
        return V(r, np.maximum(r, 0.5 * self.m / np.maximum(r, 1e-300)))

    def where(self, mask, other):
        o = V.of(other)
        return V(np.where(mask, self.v, o.v), np.where(mask, self.m, o.m))


def _f32(x):
    return np.asarray(x, np.float32)


def chain(frame, means3D, scales, rotations, opacities, shs, state, visible, sums, mags=None, magnitude=False,
          clamp_mul=True):
    """frame: the dict of sfgs.camera.make_frame. means3D .. shs: the float32 inputs (shs [N,M,3] or None).
    state: OracleRender.chain_state(). visible: radii > 0. sums [N,12]: the per-Gaussian 2D sums in Acc2D / Grad2D order
    (gmx, gmy, absx, absy, gA, gB, gC, gop, gr, gg, gb, gdepth). mags [N,12]: their magnitudes (default |sums|).
    clamp_mul=False: the WRONG chain that lets a clamped Jacobian coordinate pass its gradient on (x_mul = y_mul = 1); the
    tests use it to show that they would notice that defect (tests/test_gpu_camera_model.py), nothing else may.
    Returns a dict of float64 arrays shaped like the oracle's gradients; invisible Gaussians get zeros."""
    N = int(np.asarray(means3D).shape[0])
    idx = np.nonzero(np.asarray(visible))[0]
    sums = np.asarray(sums, np.float64)
    mags = np.abs(sums) if mags is None else np.asarray(mags, np.float64)
    P = np.asarray(means3D, np.float64)[idx]
    S = np.asarray(scales, np.float64)[idx]
    Q = np.asarray(rotations, np.float64)[idx]
    st = np.asarray(state, np.float64)[idx]
    opac = V(np.asarray(opacities, np.float64).reshape(-1)[idx])
    W, H = int(frame["W"]), int(frame["H"])
    Vm = np.asarray(frame["view"], np.float64).reshape(-1)
    PM = np.asarray(frame["proj"], np.float64).reshape(-1)
    cam = np.asarray(frame["campos"], np.float64).reshape(-1)
    ks32 = np.float32(frame["kernel_size"])
    mod = float(np.float32(frame.get("scale_modifier", 1.0)))

    gmx, gmy, absx, absy, gA, gB, gC, gop, gr0, gr1, gr2, gdepth = (V(sums[idx, k], mags[idx, k]) for k in range(12))
    a0, b0, c0 = V(st[:, 0]), V(st[:, 1]), V(st[:, 2])
    tx, ty, tz = V(st[:, 3]), V(st[:, 4]), V(st[:, 5])
    coef = V(st[:, 12])
    out = {}

    # means2D: col 2 = sqrt(absx^2 + absy^2), which an error (ex, ey) of the two sums moves by at most hypot(ex, ey)
    m2abs = np.sqrt(absx.v * absx.v + absy.v * absy.v)
    out["means2D"] = [gmx, gmy, V(m2abs, np.maximum(m2abs, np.hypot(absx.m, absy.m)))]
    out["opacities"] = [gop * coef]
    gcoef = gop * opac

    # conic -> filtered covariance
    ks = V(float(ks32))
    a, b, c = a0 + ks, b0, c0 + ks
    det = a * c - b * b
    inv2 = (det * det).recip()
    ga = (-(c * c) * gA + b * c * gB - b * b * gC) * inv2
    gb = (2.0 * b * c * gA - (a * c + b * b) * gB + 2.0 * a * b * gC) * inv2
    gc = (-(b * b) * gA + a * b * gB - a * a * gC) * inv2
    # coef -> (a0, b0, c0); the guard is decided in float32 as the oracle decides it
    a0f, b0f, c0f = _f32(st[:, 0]), _f32(st[:, 1]), _f32(st[:, 2])
    af, cf = a0f + ks32, c0f + ks32
    det0f = a0f * c0f - b0f * b0f
    det1f = af * cf - b0f * b0f
    guard = (det0f > np.float32(1e-6)) & (det1f > np.float32(1e-6)) & (st[:, 12] > 0)
    det0 = a0 * c0 - b0 * b0
    safe_coef = coef.where(guard, 1.0)
    dcoef_dr = 0.5 / safe_coef
    den = det + 1e-6
    gdet0 = gcoef * dcoef_dr / den
    gdet1 = -(gcoef * dcoef_dr * det0) / (den * den)
    zero = V(np.zeros(len(idx)))
    ga = ga + (gdet0 * c0 + gdet1 * c).where(guard, zero)
    gb = gb + (gdet0 * (-2.0 * b0) + gdet1 * (-2.0 * b)).where(guard, zero)
    gc = gc + (gdet0 * a0 + gdet1 * a).where(guard, zero)

    # the rows of T = J W (guard band decided in float32)
    tanx32, tany32 = np.float32(frame["tanfovx"]), np.float32(frame["tanfovy"])
    limx32, limy32 = np.float32(1.3) * tanx32, np.float32(1.3) * tany32
    txf, tyf, tzf = _f32(st[:, 3]), _f32(st[:, 4]), _f32(st[:, 5])
    txtzf, tytzf = txf / tzf, tyf / tzf
    out_x = (txtzf < -limx32) | (txtzf > limx32)
    out_y = (tytzf < -limy32) | (tytzf > limy32)
    txtz, tytz = tx / tz, ty / tz
    ux = txtz.where(~out_x, V(np.where(txtzf < 0, -float(limx32), float(limx32)))) * tz
    uy = tytz.where(~out_y, V(np.where(tytzf < 0, -float(limy32), float(limy32)))) * tz
    fx = float(np.float32(W) / (np.float32(2.0) * tanx32))
    fy = float(np.float32(H) / (np.float32(2.0) * tany32))
    tz1 = tz.recip()
    tz2 = tz1 * tz1
    tz3 = tz2 * tz1
    J00, J02 = fx * tz1, -(fx * ux) * tz2
    J11, J12 = fy * tz1, -(fy * uy) * tz2
    T0 = [J00 * Vm[k * 4 + 0] + J02 * Vm[k * 4 + 2] for k in range(3)]
    T1 = [J11 * Vm[k * 4 + 1] + J12 * Vm[k * 4 + 2] for k in range(3)]
    c3 = [V(st[:, 6 + k]) for k in range(6)]
    S3 = [[c3[0], c3[1], c3[2]], [c3[1], c3[3], c3[4]], [c3[2], c3[4], c3[5]]]
    v0 = [S3[r][0] * T0[0] + S3[r][1] * T0[1] + S3[r][2] * T0[2] for r in range(3)]
    v1 = [S3[r][0] * T1[0] + S3[r][1] * T1[1] + S3[r][2] * T1[2] for r in range(3)]
    Gm = [[ga * T0[r] * T0[k] + gb * T0[r] * T1[k] + gc * T1[r] * T1[k] for k in range(3)] for r in range(3)]
    gT0 = [2.0 * ga * v0[k] + gb * v1[k] for k in range(3)]
    gT1 = [2.0 * gc * v1[k] + gb * v0[k] for k in range(3)]
    gJ00 = gT0[0] * Vm[0] + gT0[1] * Vm[4] + gT0[2] * Vm[8]
    gJ02 = gT0[0] * Vm[2] + gT0[1] * Vm[6] + gT0[2] * Vm[10]
    gJ11 = gT1[0] * Vm[1] + gT1[1] * Vm[5] + gT1[2] * Vm[9]
    gJ12 = gT1[0] * Vm[2] + gT1[1] * Vm[6] + gT1[2] * Vm[10]
    x_mul, y_mul = (~out_x).astype(np.float64), (~out_y).astype(np.float64)
    if not clamp_mul:
        x_mul, y_mul = np.ones_like(x_mul), np.ones_like(y_mul)
    gtx = x_mul * (-fx * tz2) * gJ02
    gty = y_mul * (-fy * tz2) * gJ12
    gtz = -fx * tz2 * gJ00 - fy * tz2 * gJ11 + (2.0 * fx * ux) * tz3 * gJ02 + (2.0 * fy * uy) * tz3 * gJ12
    gtz = gtz + gdepth
    gp = [gtx * Vm[k * 4 + 0] + gty * Vm[k * 4 + 1] + gtz * Vm[k * 4 + 2] for k in range(3)]
    # mean2D (NDC units) -> p through the perspective divide
    p = [V(P[:, k]) for k in range(3)]
    hx = PM[0] * p[0] + PM[4] * p[1] + PM[8] * p[2] + PM[12]
    hy = PM[1] * p[0] + PM[5] * p[1] + PM[9] * p[2] + PM[13]
    hw = PM[3] * p[0] + PM[7] * p[1] + PM[11] * p[2] + PM[15]
    pw = (hw + 0.0000001).recip()
    mul1, mul2 = hx * pw * pw, hy * pw * pw
    for k in range(3):
        gp[k] = gp[k] + (PM[k * 4 + 0] * pw - PM[k * 4 + 3] * mul1) * gmx + (PM[k * 4 + 1] * pw - PM[k * 4 + 3] * mul2) * gmy

    # Sigma = M M^T, M = R diag(mod s)
    qr, qx, qy, qz = (V(Q[:, k]) for k in range(4))
    R = [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qr * qz), 2.0 * (qx * qz + qr * qy)],
         [2.0 * (qx * qy + qr * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qr * qx)],
         [2.0 * (qx * qz - qr * qy), 2.0 * (qy * qz + qr * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]]
    Sv = [mod * V(S[:, j]) for j in range(3)]
    Mm = [[R[r][j] * Sv[j] for j in range(3)] for r in range(3)]
    gM = [[(Gm[r][0] + Gm[0][r]) * Mm[0][j] + (Gm[r][1] + Gm[1][r]) * Mm[1][j] + (Gm[r][2] + Gm[2][r]) * Mm[2][j]
           for j in range(3)] for r in range(3)]
    gs = [mod * (gM[0][j] * R[0][j] + gM[1][j] * R[1][j] + gM[2][j] * R[2][j]) for j in range(3)]
    gR = [gM[r][j] * Sv[j] for r in range(3) for j in range(3)]    # row-major [9]
    out["scales"] = gs
    out["rotations"] = [
        2.0 * (-qz * gR[1] + qy * gR[2] + qz * gR[3] - qx * gR[5] - qy * gR[6] + qx * gR[7]),
        2.0 * (qy * gR[1] + qz * gR[2] + qy * gR[3] - 2.0 * qx * gR[4] - qr * gR[5] + qz * gR[6] + qr * gR[7]
               - 2.0 * qx * gR[8]),
        2.0 * (-2.0 * qy * gR[0] + qx * gR[1] + qr * gR[2] + qx * gR[3] + qz * gR[5] - qr * gR[6] + qz * gR[7]
               - 2.0 * qy * gR[8]),
        2.0 * (-2.0 * qz * gR[0] - qr * gR[1] + qx * gR[2] + qr * gR[3] - 2.0 * qz * gR[4] + qy * gR[5] + qx * gR[6]
               + qy * gR[7])]

    grgb = [gr0, gr1, gr2]
    if shs is None:
        out["colors_precomp"] = grgb
    else:
        sh = np.asarray(shs, np.float64)[idx]            # [n, M, 3]
        M = sh.shape[1]
        deg = int(frame.get("sh_degree", 0))
        d = [p[k] - cam[k] for k in range(3)]
        ln = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]).sqrt()
        x, y, z = d[0] / ln, d[1] / ln, d[2] / ln
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        one = V(np.ones(len(idx)))
        basis = [SH_C0 * one]
        if deg > 0:
            basis += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
        if deg > 1:
            basis += [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
        if deg > 2:
            basis += [SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4.0 * zz - xx - yy),
                      SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), SH_C3[4] * x * (4.0 * zz - xx - yy),
                      SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3.0 * yy)]
        gsh = [[zero for _ in range(3)] for _ in range(M)]
        gdir = [zero, zero, zero]
        for ch in range(3):
            clamped = st[:, 13 + ch] != 0
            gr = grgb[ch].where(~clamped, zero)
            c_ = [V(sh[:, k, ch]) for k in range(M)]
            for k in range(len(basis)):
                gsh[k][ch] = basis[k] * gr
            dRdx = dRdy = dRdz = zero
            if deg > 0:
                dRdx, dRdy, dRdz = -SH_C1 * c_[3], -SH_C1 * c_[1], SH_C1 * c_[2]
            if deg > 1:
                dRdx = dRdx + SH_C2[0] * y * c_[4] + SH_C2[2] * 2.0 * -x * c_[6] + SH_C2[3] * z * c_[7] + SH_C2[4] * 2.0 * x * c_[8]
                dRdy = dRdy + SH_C2[0] * x * c_[4] + SH_C2[1] * z * c_[5] + SH_C2[2] * 2.0 * -y * c_[6] + SH_C2[4] * 2.0 * -y * c_[8]
                dRdz = dRdz + SH_C2[1] * y * c_[5] + SH_C2[2] * 4.0 * z * c_[6] + SH_C2[3] * x * c_[7]
            if deg > 2:
                dRdx = (dRdx + SH_C3[0] * c_[9] * 6.0 * xy + SH_C3[1] * c_[10] * yz + SH_C3[2] * c_[11] * -2.0 * xy
                        + SH_C3[3] * c_[12] * -6.0 * xz + SH_C3[4] * c_[13] * (-3.0 * xx + 4.0 * zz - yy)
                        + SH_C3[5] * c_[14] * 2.0 * xz + SH_C3[6] * c_[15] * 3.0 * (xx - yy))
                dRdy = (dRdy + SH_C3[0] * c_[9] * 3.0 * (xx - yy) + SH_C3[1] * c_[10] * xz
                        + SH_C3[2] * c_[11] * (-3.0 * yy + 4.0 * zz - xx) + SH_C3[3] * c_[12] * -6.0 * yz
                        + SH_C3[4] * c_[13] * -2.0 * xy + SH_C3[5] * c_[14] * -2.0 * yz + SH_C3[6] * c_[15] * -6.0 * xy)
                dRdz = (dRdz + SH_C3[1] * c_[10] * xy + SH_C3[2] * c_[11] * 8.0 * yz
                        + SH_C3[3] * c_[12] * 3.0 * (2.0 * zz - xx - yy) + SH_C3[4] * c_[13] * 8.0 * xz
                        + SH_C3[5] * c_[14] * (xx - yy))
            gdir = [gdir[0] + dRdx * gr, gdir[1] + dRdy * gr, gdir[2] + dRdz * gr]
        dot = x * gdir[0] + y * gdir[1] + z * gdir[2]
        gp = [gp[0] + (gdir[0] - x * dot) / ln, gp[1] + (gdir[1] - y * dot) / ln, gp[2] + (gdir[2] - z * dot) / ln]
        out["shs"] = gsh
    out["means3D"] = gp

    def dense(cols, shape):
        full = np.zeros((N,) + shape, np.float64)
        arr = np.stack([np.broadcast_to(c.m if magnitude else c.v, (len(idx),)) for c in cols], axis=1)
        full[idx] = arr.reshape((len(idx),) + shape)
        return full

    res = dict(means3D=dense(out["means3D"], (3,)), means2D=dense(out["means2D"], (3,)),
               scales=dense(out["scales"], (3,)), rotations=dense(out["rotations"], (4,)),
               opacities=dense(out["opacities"], (1,)))
    if shs is None:
        res["colors_precomp"] = dense(out["colors_precomp"], (3,))
    else:
        M = np.asarray(shs).shape[1]
        res["shs"] = dense([out["shs"][k][ch] for k in range(M) for ch in range(3)], (M, 3))
    return res
