"""Float64 numpy restatement of sfgs.transform's kernel (include/sfgs.h: sfgs_similarity_transform) and of transform_camera:
what tests/test_transform_host.py renders through the C oracle and what tests/test_gpu_transform.py holds the kernel to.

Every function takes the constants as a dict (R [3,3], s, log_s, t [3], q [4], D1, D2, D3) -- `constants(sim)` in float64,
`constants(sim, np.float32)` the values the kernel receives, rounded once and widened again -- and returns (value, abs_sum):
the float64 result and the sum of the absolute values of the terms that were added to form it, which is what a float32
error bound scales with."""
import numpy as np

BANDS = ((0, 3), (3, 8), (8, 15))
U = 2.0 ** -24
BOUND_FACTOR = 8 * U   # at most 7 products summed in index order, plus the final product / add


def quat_to_matrix(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def constants(sim, dtype=np.float64):
    """dtype=np.float32: every constant rounded to float32 once (what travels to the kernel), returned as float64."""
    from sfgs import transform as T
    D = T.sh_rotation(sim.R, 3)
    c = dict(R=sim.R, s=np.float64(sim.s), log_s=np.float64(np.log(sim.s)), t=sim.t, q=T.rotation_quaternion(sim.R),
             D1=D[0], D2=D[1], D3=D[2])
    return {k: np.asarray(v, np.float64).astype(dtype).astype(np.float64) for k, v in c.items()}


def xyz(c, x):
    x = np.asarray(x, np.float64)
    terms = c["s"] * c["R"][None, :, :] * x[:, None, :]          # [N, i, j] = s R_ij x_j
    return terms.sum(2) + c["t"], np.abs(terms).sum(2) + np.abs(c["t"])


def scaling(c, v, is_log):
    v = np.asarray(v, np.float64)
    if is_log:
        return v + c["log_s"], np.abs(v) + np.abs(c["log_s"])
    return v * c["s"], np.abs(v * c["s"])


def filter_3d(c, v):
    v = np.asarray(v, np.float64)
    return v * c["s"], np.abs(v * c["s"])


# q_R (x) q, Hamilton product on (w, x, y, z): out_i = sum_j sign[i][j] a[j] b[perm[i][j]]
_QPERM = np.array([[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]])
_QSIGN = np.array([[1, -1, -1, -1], [1, 1, 1, -1], [1, -1, 1, 1], [1, 1, -1, 1]], np.float64)


def rotation(c, q):
    q = np.asarray(q, np.float64)
    terms = _QSIGN[None] * c["q"][None, None, :] * q[:, _QPERM]   # [N, i, j]
    return terms.sum(2), np.abs(terms).sum(2)


def features_rest(c, f, layout):
    """f: [N,K-1,3] ("nk3") or [N,3,K-1] ("n3k"), K-1 in (0, 3, 8, 15) -> the same layout."""
    f = np.asarray(f, np.float64)
    v = f if layout == "n3k" else f.transpose(0, 2, 1)           # [N, 3, K-1]
    out, mag = np.zeros_like(v), np.zeros_like(v)
    for (a, b), D in zip(BANDS, (c["D1"], c["D2"], c["D3"])):
        if v.shape[2] < b:
            break
        terms = D[None, None, :, :] * v[:, :, None, a:b]          # [N, c, i, j] = D_ij v_j
        out[:, :, a:b] = terms.sum(3)
        mag[:, :, a:b] = np.abs(terms).sum(3)
    if layout == "n3k":
        return out, mag
    return out.transpose(0, 2, 1), mag.transpose(0, 2, 1)


def camera(R, T, sim):
    """CameraInfo's (R, T) in the transformed world: the world-to-camera map of x' = s R_s x + t that gives s times the old
    camera-space coordinates. p_cam = W x + T with W = R^T and x = R_s^T (x' - t) / s, times s."""
    W = np.asarray(R, np.float64).T
    W2 = W @ sim.R.T
    return W2.T, sim.s * np.asarray(T, np.float64) - W2 @ sim.t


def transform_scene(g, sim, dtype=np.float64):
    """A sfgs.synth scene dict (means3D, scales ACTIVATED, rotations, opacities, colors_precomp, shs [N,K,3] with DC first)
    moved by `sim` in float64 (constants in `dtype`) and rounded to float32 -> dict of float32 numpy arrays / None."""
    c = constants(sim, dtype)
    num = lambda t: None if t is None else np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t)
    out = {k: num(v) for k, v in g.items()}
    out["means3D"] = xyz(c, out["means3D"])[0].astype(np.float32)
    out["scales"] = scaling(c, out["scales"], False)[0].astype(np.float32)
    out["rotations"] = rotation(c, out["rotations"])[0].astype(np.float32)
    if out.get("shs") is not None:
        shs = out["shs"].astype(np.float64)
        shs[:, 1:] = features_rest(c, shs[:, 1:], "nk3")[0]
        out["shs"] = shs.astype(np.float32)
    return out


# ---- the render-invariance cases shared by the host test (C oracle) and the GPU test (HIP path) --------------------------------
RENDER_W, RENDER_H, RENDER_N = 96, 64, 3000
# The scene is sfgs.synth's default one (depth 250 ... 350, splats of 0.05 ... 0.6 world units: a few pixels each at 96 x 64,
# every one of the 3000 on screen): after s = 0.37 and t = (100, -50, 20) the positions are ~150 in size, a float32 ulp of
# 1.5e-5, which at a depth of ~110 and 83 pixels of focal length moves a splat by 1e-5 pixels -- inside the parity tolerance.
RENDER_FORMS = {"sh3": dict(mode="sh", sh_degree=3), "precomp_jitter": dict(mode="precomp", jitter=True),
                "sh2_pitch35": dict(mode="sh", sh_degree=2, pitch_deg=35)}


def render_similarity():
    from sfgs.transform import Similarity
    return Similarity(quat_to_matrix(np.random.default_rng(1).normal(size=4)), 0.37, (100.0, -50.0, 20.0))


def render_case(form):
    """-> (frame, scene dict, camera R, camera T) of sfgs.synth.scene(3000, 96, 64, seed=3, **RENDER_FORMS[form])."""
    import math
    from sfgs.synth import scene
    kw = RENDER_FORMS[form]
    frame, g = scene(RENDER_N, RENDER_W, RENDER_H, seed=3, **kw)
    R = np.eye(3)
    if kw.get("pitch_deg"):                                       # sfgs.synth.scene's camera
        a = math.radians(kw["pitch_deg"])
        R = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    return frame, g, R, np.zeros(3)


def moved_frame(frame, R, T, fovx_deg=60.0):
    """`frame` seen from the camera (R, T): everything but the three camera tensors is kept."""
    import math
    from sfgs.camera import fovy_from_fovx, make_frame
    fovx = math.radians(fovx_deg)
    new = make_frame(R, T, fovx, fovy_from_fovx(fovx, frame["W"], frame["H"]), frame["W"], frame["H"],
                     kernel_size=frame["kernel_size"], sh_degree=frame["sh_degree"], subpix=frame["subpix"])
    assert new["tanfovx"] == frame["tanfovx"] and new["tanfovy"] == frame["tanfovy"]
    return new
