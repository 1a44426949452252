"""sfgs.transform -- similarity transforms (rotation, uniform scale, translation) of trained Gaussian scenes on one HIP kernel
(csrc/transform.hip through libsfgs.so).

Why: the reference trains every satellite scene in a frame of its own. `readSatelliteInfo` (scene/dataset_readers.py:378-390,
cameras :397-457) rotates and shifts the points by the dataset's R / T (`xyz @ R.T - T`), scales them so that the 99th
percentile of their norms is 256 (another factor for every scene) and drops them so that the 1st percentile of z is 0. Two
tiles trained by the unchanged train.py therefore differ by a full similarity, and `sfgs.ply.merge_fused_plys(paths, offsets)`
-- a translation per file -- cannot put them into one frame. This module can:

    sim = Similarity.from_satellite_frame(R_fix, T_fix, scale, z_min)      # dataset frame -> the frame the model was trained in
    transform_model(model, sim.inverse())                                  # a trained scene back into the dataset frame
    merged = sfgs.ply.merge_fused_plys(paths, transforms=[a, b], out_path=...)

Moving a trained scene moves more than points: log-scales shift by log s, quaternions are multiplied by the rotation's,
filter_3D scales by s, and the view-dependent colour turns with the scene -- the SH coefficients of bands 1-3 are multiplied
by the real-SH rotation matrices of `sh_rotation` (in the basis order and signs of utils/sh_utils.py:57-112). DC colour and
opacity do not change. `transform_camera` moves a camera along, so that images stay what they were and depth scales by s.

Host side float64 (`Similarity`, `sh_rotation`, `satellite_normalisation`, `transform_camera` need neither GPU nor library);
the constants are rounded to float32 once and travel by value. There is no torch fallback: without the HIP library
`transform_gaussians` raises."""
import numpy as np
import torch

from . import _call
from . import _lib as L

__all__ = ["Similarity", "satellite_normalisation", "sh_rotation", "sh_basis", "rotation_quaternion", "kernel_constants",
           "transform_gaussians", "transform_model", "transform_camera"]

_ORTHO_TOL = 1e-9
_LAYOUTS = ("nk3", "n3k")


class Similarity:
    """x' = s R x + t with R a proper rotation (float64 [3,3]), s > 0, t float64 [3]."""

    def __init__(self, R, s=1.0, t=(0.0, 0.0, 0.0)):
        R = np.array(R, dtype=np.float64)
        t = np.array(t, dtype=np.float64).reshape(-1)
        s = float(s)
        if R.shape != (3, 3) or t.shape != (3,):
            raise ValueError(f"R must be [3,3] and t [3], got {R.shape} and {t.shape}")
        if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s)):
            raise ValueError("R, s and t must be finite")
        if np.abs(R @ R.T - np.eye(3)).max() > _ORTHO_TOL:
            raise ValueError(f"R is not orthonormal to {_ORTHO_TOL:g} (max |R R^T - I| = {np.abs(R @ R.T - np.eye(3)).max():.3g})")
        if np.linalg.det(R) < 0:
            raise ValueError("R is a reflection (det R < 0): not a proper similarity")
        if not s > 0:
            raise ValueError(f"s must be positive, got {s}")
        self.R, self.s, self.t = R, s, t

    @staticmethod
    def identity():
        return Similarity(np.eye(3))

    @staticmethod
    def from_matrix(M):
        """The 4 x 4 matrix [[s R, t], [0, 1]]."""
        M = np.array(M, dtype=np.float64)
        if M.shape != (4, 4) or not np.allclose(M[3], (0.0, 0.0, 0.0, 1.0), rtol=0, atol=1e-12):
            raise ValueError("a 4 x 4 matrix with last row (0, 0, 0, 1) expected")
        A = M[:3, :3]
        det = np.linalg.det(A)
        if not det > 0:
            raise ValueError("the linear part is singular or a reflection (det <= 0): not a proper similarity")
        s = float(np.cbrt(det))
        return Similarity(A / s, s, M[:3, 3])

    @staticmethod
    def from_satellite_frame(R_fix, T_fix, scale, z_min):
        """The map readSatelliteInfo applies to the points of a scene (scene/dataset_readers.py:381-390):
        x_m = scale (R_fix x - T_fix) - (0, 0, z_min). Its inverse() takes a trained scene back into the dataset's frame."""
        T_fix = np.asarray(T_fix, dtype=np.float64).reshape(3)
        return Similarity(R_fix, scale, -float(scale) * T_fix - np.array([0.0, 0.0, float(z_min)]))

    def matrix(self):
        M = np.eye(4)
        M[:3, :3] = self.s * self.R
        M[:3, 3] = self.t
        return M

    def inverse(self):
        return Similarity(self.R.T, 1.0 / self.s, -(self.R.T @ self.t) / self.s)

    def compose(self, other):
        """self after other: x -> self(other(x))."""
        return Similarity(self.R @ other.R, self.s * other.s, self.s * (self.R @ other.t) + self.t)

    def apply(self, points):
        """float64 [N,3] -> float64 [N,3] on the host."""
        return self.s * (np.asarray(points, dtype=np.float64) @ self.R.T) + self.t

    def __repr__(self):
        return f"Similarity(R={self.R.tolist()}, s={self.s!r}, t={self.t.tolist()})"


def satellite_normalisation(points, R_fix, T_fix):
    """-> (scale, z_min): the two percentiles of readSatelliteInfo (scene/dataset_readers.py:381-390), which the reference
    prints and does not store. points: [N,3] as read from points3D.txt; R_fix [3,3] and T_fix [3] from transforms_*.json."""
    xyz = np.asarray(points, dtype=np.float64)
    R = np.asarray(R_fix, dtype=np.float64)[:3, :3]
    T = np.asarray(T_fix, dtype=np.float64)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.shape[0] == 0:
        raise ValueError(f"points must be a non-empty [N,3], got {xyz.shape}")
    xyz = np.matmul(xyz, R.T) - T
    radius = np.percentile(np.linalg.norm(xyz, axis=1), 99)
    scale = 256 / radius
    xyz = xyz * scale
    z_min = np.percentile(xyz[:, 2], 1)
    return float(scale), float(z_min)


# ---- real spherical harmonics in eval_sh's basis ------------------------------------------------------------------------------
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435)


def sh_basis(dirs):
    """float64 [M,3] unit directions -> [M,15]: the factors of sh[..., 1] ... sh[..., 15] in eval_sh (utils/sh_utils.py:76-100),
    signs included."""
    d = np.asarray(dirs, dtype=np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([-_C1 * y, _C1 * z, -_C1 * x,
                     _C2[0] * xy, _C2[1] * yz, _C2[2] * (2.0 * zz - xx - yy), _C2[3] * xz, _C2[4] * (xx - yy),
                     _C3[0] * y * (3 * xx - yy), _C3[1] * xy * z, _C3[2] * y * (4 * zz - xx - yy),
                     _C3[3] * z * (2 * zz - 3 * xx - 3 * yy), _C3[4] * x * (4 * zz - xx - yy), _C3[5] * z * (xx - yy),
                     _C3[6] * x * (xx - 3 * yy)], axis=1)


_BANDS = ((0, 3), (3, 8), (8, 15))   # columns of sh_basis per band


def _fit_directions(count=64):
    """A fixed, well-spread direction set (golden-angle spiral): each band's basis has full column rank on it."""
    i = np.arange(count, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / count
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def sh_rotation(R, degree=3):
    """-> [D_1, ..., D_degree], float64 [(2 l + 1), (2 l + 1)]: the matrices with eval_sh(deg, D sh, R d) == eval_sh(deg, sh, d)
    for every unit d, i.e. basis_l(R d) = D_l basis_l(d). A band is closed under rotation, so the identity holds exactly for
    ONE matrix per band; it is found as the least-squares solution on a fixed direction set (residual at rounding level)."""
    R = np.asarray(R, dtype=np.float64)
    if R.shape != (3, 3):
        raise ValueError(f"R must be [3,3], got {R.shape}")
    if not 0 <= int(degree) <= 3:
        raise ValueError(f"degree must be 0 ... 3, got {degree}")
    d = _fit_directions()
    A, B = sh_basis(d), sh_basis(d @ R.T)
    out = []
    for a, b in _BANDS[:int(degree)]:
        X = np.linalg.lstsq(A[:, a:b], B[:, a:b], rcond=None)[0]   # A X = B, X = D^T
        X[np.abs(X) < 1e-14] = 0.0   # entries are bounded by 1 and carry ~1e-16 of noise: an exact zero (D(I) = I) stays one
        out.append(np.ascontiguousarray(X.T))
    return out


def rotation_quaternion(R):
    """float64 (w, x, y, z), w >= 0, of a proper rotation matrix (the largest of the four candidates as the pivot)."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cand = np.array([tr, R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]])
    k = int(np.argmax(cand))
    if k == 0:
        q = np.array([1.0 + tr, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1.0 + cand[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 + cand[2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + cand[3]])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def kernel_constants(sim):
    """The float32 constants the kernel receives, each rounded once from float64:
    dict(R [3,3], s, log_s, t [3], q [4], D1 [3,3], D2 [5,5], D3 [7,7])."""
    D = sh_rotation(sim.R, 3)
    f = np.float32
    return dict(R=sim.R.astype(f), s=f(sim.s), log_s=f(np.log(sim.s)), t=sim.t.astype(f),
                q=rotation_quaternion(sim.R).astype(f), D1=D[0].astype(f), D2=D[1].astype(f), D3=D[2].astype(f))


def transform_camera(R, T, sim):
    """CameraInfo's (R, T) -- R the camera-to-world rotation, T the world-to-camera translation -- of the same camera in the
    transformed world, chosen so that camera-space coordinates of transformed points are s times the old ones:
    W' = W R_sim^T, T' = s T - W' t with W = R^T. Images are unchanged, depth scales by s. -> (R', T'), float64."""
    if not isinstance(sim, Similarity):
        raise ValueError("sim must be a Similarity")
    W = np.asarray(R, dtype=np.float64).T
    W2 = W @ sim.R.T
    return np.ascontiguousarray(W2.T), sim.s * np.asarray(T, dtype=np.float64).reshape(3) - W2 @ sim.t


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _rest_coeffs(features_rest, rest_layout):
    k = 1 if rest_layout == "nk3" else 2
    return int(features_rest.shape[k])


def transform_gaussians(sim, xyz, scaling=None, rotation=None, features_rest=None, filter_3D=None, scaling_is_log=True,
                        rest_layout="nk3", inplace=False):
    """Apply `sim` to the tensors of N Gaussians in ONE launch. Device tensors, float32, contiguous when `inplace`:
        xyz [N,3] (or None)        s R x + t
        scaling [N,3]              scaling_is_log (the model's _scaling, a fused PLY's scale_*): + float32(log s); else: * s
        rotation [N,4]             (w, x, y, z) as given, not renormalised: q_R (x) q
        features_rest              [N,K-1,3] (rest_layout "nk3", the model's _features_rest) or [N,3,K-1] ("n3k", a fused PLY's
                                   f_rest_* columns), K-1 in {0, 3, 8, 15}: band l times D_l per channel
        filter_3D [N,1]            * s
    Every tensor is optional; DC colour and opacity do not change and are not passed.
    -> (xyz, scaling, rotation, features_rest, filter_3D): new tensors, or the arguments themselves when `inplace`; None stays None."""
    if not isinstance(sim, Similarity):
        raise ValueError("sim must be a Similarity")
    if rest_layout not in _LAYOUTS:
        raise ValueError(f"rest_layout must be 'nk3' or 'n3k', got {rest_layout!r}")
    named = dict(xyz=xyz, scaling=scaling, rotation=rotation, features_rest=features_rest, filter_3D=filter_3D)
    first = next((t for t in named.values() if isinstance(t, torch.Tensor)), None)
    if first is None:
        raise ValueError("at least one tensor is needed")
    N = int(first.shape[0]) if first.dim() > 0 else -1
    _call.check_tensor("xyz", xyz, f"[{N},3]", lambda t: tuple(t.shape) == (N, 3), none_ok=True)
    _call.check_tensor("scaling", scaling, f"[{N},3]", lambda t: tuple(t.shape) == (N, 3), none_ok=True)
    _call.check_tensor("rotation", rotation, f"[{N},4]", lambda t: tuple(t.shape) == (N, 4), none_ok=True)
    _call.check_tensor("filter_3D", filter_3D, f"[{N},1] or [{N}]", lambda t: tuple(t.shape) in ((N, 1), (N,)), none_ok=True)
    rest_text = f"[{N},K-1,3]" if rest_layout == "nk3" else f"[{N},3,K-1]"
    _call.check_tensor("features_rest", features_rest, rest_text + " with K-1 in (0, 3, 8, 15)",
                       lambda t: t.dim() == 3 and t.shape[0] == N and t.shape[2 if rest_layout == "nk3" else 1] == 3
                       and _rest_coeffs(t, rest_layout) in (0, 3, 8, 15), none_ok=True)
    if N >= 1 << 31:
        raise ValueError(f"at most 2^31 - 1 Gaussians per call, got {N}")
    if inplace:
        for name, t in named.items():
            if t is not None and not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous for an in-place transform")
    _call.check_gpu(**named)
    dev = first.device
    _call.same_device(dev, "the first tensor's device", **named)
    lib = L.load()
    src = {k: (None if t is None else t.detach().contiguous()) for k, t in named.items()}
    dst = {k: (None if t is None else (t if inplace else torch.empty_like(t))) for k, t in src.items()}
    kr = 0 if features_rest is None else _rest_coeffs(features_rest, rest_layout)
    c = kernel_constants(sim)
    args = L.SfgsSimilarityArgs()
    args.struct_size = L.C.sizeof(L.SfgsSimilarityArgs)
    args.flags = (L.SIM_SCALING_LOG if scaling_is_log else 0) | (L.SIM_REST_N3K if rest_layout == "n3k" else 0)
    args.n, args.sh_rest_coeffs = N, kr
    for field, key in (("xyz", "xyz"), ("scaling", "scaling"), ("rotation", "rotation"), ("sh_rest", "features_rest"),
                       ("filter3d", "filter_3D")):
        if src[key] is not None and not (key == "features_rest" and kr == 0):
            setattr(args, field + "_in", src[key].data_ptr())
            setattr(args, field + "_out", dst[key].data_ptr())
    for field in ("R", "t", "q", "D1", "D2", "D3"):
        flat = c[field].reshape(-1)
        setattr(args, field, type(getattr(args, field))(*[float(v) for v in flat]))
    args.s, args.log_s = float(c["s"]), float(c["log_s"])
    with torch.cuda.device(dev):
        L.check(lib.sfgs_similarity_transform(L.C.byref(args), _call.stream(dev)))
    if inplace:
        return tuple(named.values())
    return tuple(dst.values())


@torch.no_grad()
def transform_model(model, sim):
    """Move a GaussianModel-like object by `sim`, in place: _xyz, _scaling (log space), _rotation, _features_rest ([N,K-1,3]) and
    filter_3D where the model has one. _features_dc and _opacity do not change; `_embeddings` (the appearance MLP's
    per-Gaussian inputs) are left alone on purpose: they are not quantities of the frame. Adam's moments are NOT transformed,
    so a model that carries an optimizer is refused: transform before training_setup, or a model loaded for rendering."""
    if not isinstance(sim, Similarity):
        raise ValueError("sim must be a Similarity")
    if getattr(model, "optimizer", None) is not None:
        raise ValueError("the model carries an optimizer: its Adam moments would not be transformed")
    filt = getattr(model, "filter_3D", None)
    if not isinstance(filt, torch.Tensor) or filt.numel() == 0:
        filt = None
    # compute_3D_filter keeps float64 (scene/gaussian_model.py:255-308): that tensor takes one float64 product below, not the
    # float32 kernel
    filt64 = filt if filt is not None and filt.dtype == torch.float64 else None
    rest = model._features_rest.data
    transform_gaussians(sim, model._xyz.data, model._scaling.data, model._rotation.data,
                        rest if rest.shape[1] > 0 else None, None if filt64 is not None else filt, scaling_is_log=True,
                        rest_layout="nk3", inplace=True)
    if filt64 is not None:
        filt64.mul_(sim.s)
    return model
