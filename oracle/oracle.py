"""ctypes front-end of the CPU oracle (oracle/sfgs_oracle.c).  TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module; the
product path (skyfall-gs_amd/) never does. PARITY UNPINNED: see the header of sfgs_oracle.c.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_build", "liborc.so")
_lib = None
# calibration builds of the same source (oracle/Makefile: `make variants`); tests/grad_bounds.py measures against them
_VARIANT_PATHS = {"accf": os.path.join(_HERE, "_build", "liborc_accf.so"),
                  "jit": os.path.join(_HERE, "_build", "liborc_jit.so")}
_variant_libs = {}
EXPORT_WORDS = 22   # orc_backward_ex: 12 signed accumulators + 10 magnitude sums per Gaussian


def _stale(path):
    src = os.path.join(_HERE, "sfgs_oracle.c")
    return not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(src)


def build(force=False):
    if force or _stale(_LIB_PATH):
        subprocess.check_call(["make", "-C", _HERE, "-s", "-B"])
    return _LIB_PATH


def _declare(L):
    L.orc_forward.restype = C.c_void_p
    L.orc_forward.argtypes = [C.POINTER(OrcFrame), C.c_int32] + [C.c_void_p] * 10
    L.orc_backward.restype = C.c_int
    L.orc_backward.argtypes = [C.c_void_p, C.POINTER(OrcFrame)] + [C.c_void_p] * 17
    L.orc_backward_ex.restype = C.c_int
    L.orc_backward_ex.argtypes = [C.c_void_p, C.POINTER(OrcFrame)] + [C.c_void_p] * 18
    L.orc_free.argtypes = [C.c_void_p]
    L.orc_get_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.orc_pixel_margins.restype = None
    L.orc_pixel_margins.argtypes = [C.c_void_p, C.POINTER(OrcFrame), C.c_void_p]
    L.orc_get_chain_state.argtypes = [C.c_void_p, C.c_void_p]
    return L


def variant_lib(name):
    """One of the calibration builds ("accf": float32 sums in reverse order, "jit": every expf scaled by
    1 +- 2 * 2^-23 max(1, sum of |terms of its argument|)), built on
    first use. Never a reference: only OracleRender(..., variant=name) in the CPU calibration tests loads it."""
    if name not in _variant_libs:
        path = _VARIANT_PATHS[name]
        if _stale(path):
            subprocess.check_call(["make", "-C", _HERE, "-s", "-B", "variants"])
        _variant_libs[name] = _declare(C.CDLL(path))
    return _variant_libs[name]


class OrcFrame(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
                ("kernel_size", C.c_float), ("scale_modifier", C.c_float), ("sh_degree", C.c_int32),
                ("sh_coeffs", C.c_int32), ("depth_mode", C.c_int32), ("subpix", C.c_void_p),
                ("bg", C.c_void_p), ("view", C.c_void_p), ("proj", C.c_void_p), ("campos", C.c_void_p)]


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = _declare(C.CDLL(_LIB_PATH))
        _lib.orc_forward_rows.restype = C.c_void_p
        _lib.orc_forward_rows.argtypes = [C.POINTER(OrcFrame), C.c_int32] + [C.c_void_p] * 10 + [C.c_int32, C.c_int32]
        _lib.orc_get_tiles_touched.argtypes = [C.c_void_p, C.c_void_p]
        _lib.orc_get_n_contrib.argtypes = [C.c_void_p, C.c_void_p]
        _lib.orc_get_tile_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.orc_get_geom.argtypes = [C.c_void_p, C.c_void_p]
        _lib.orc_decision_margins.restype = None
        _lib.orc_decision_margins.argtypes = [C.c_void_p, C.POINTER(OrcFrame), C.c_void_p]
        _lib.orc_ssim.restype = C.c_double
        _lib.orc_ssim.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p]
        _lib.orc_knn_dist2.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        _lib.orc_test_cov3d.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        _lib.orc_test_quat_to_R.argtypes = [C.c_void_p, C.c_void_p]
        _lib.orc_test_sh.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.orc_test_project.argtypes = [C.POINTER(OrcFrame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def _f32(x):
    if x is None:
        return None
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class OracleRender:
    """One forward pass of the oracle; keeps the state the backward needs."""

    def __init__(self, frame, means3D, scales, rotations, opacities, colors_precomp=None, shs=None, tile_rows=None,
                 variant=None):
        """tile_rows = (row0, row1): render only those rows of 16x16 tiles (orc_forward_rows; forward-only checks of very
        large frames -- every Gaussian is still projected, `radii` is complete; the other pixels stay zero).
        variant: a calibration build (variant_lib) instead of the oracle proper; forward / backward only."""
        L = self._L = lib() if variant is None else variant_lib(variant)
        assert variant is None or tile_rows is None
        self.H, self.W = int(frame["H"]), int(frame["W"])
        self.N = int(means3D.shape[0])
        self._keep = dict(means3D=_f32(means3D), scales=_f32(scales), rotations=_f32(rotations),
                          opacities=_f32(opacities).reshape(-1), colors=_f32(colors_precomp), shs=_f32(shs),
                          subpix=_f32(frame.get("subpix")), bg=_f32(frame["bg"]), view=_f32(frame["view"]),
                          proj=_f32(frame["proj"]), campos=_f32(frame["campos"]))
        k = self._keep
        self.sh_coeffs = 0 if k["shs"] is None else int(k["shs"].shape[1])
        self.frame = OrcFrame(self.H, self.W, float(frame["tanfovx"]), float(frame["tanfovy"]),
                              float(frame["kernel_size"]), float(frame.get("scale_modifier", 1.0)),
                              int(frame.get("sh_degree", 0)), self.sh_coeffs, int(frame.get("depth_mode", 0)),
                              _ptr(k["subpix"]), _ptr(k["bg"]), _ptr(k["view"]), _ptr(k["proj"]),
                              _ptr(k["campos"]))
        P = self.H * self.W
        self.color = np.zeros((3, self.H, self.W), np.float32)
        self.depth = np.zeros((1, self.H, self.W), np.float32)
        self.alpha = np.zeros((1, self.H, self.W), np.float32)
        self.radii = np.zeros((self.N,), np.int32)
        args = (C.byref(self.frame), self.N, _ptr(k["means3D"]), _ptr(k["scales"]),
                _ptr(k["rotations"]), _ptr(k["opacities"]), _ptr(k["colors"]), _ptr(k["shs"]),
                _ptr(self.color), _ptr(self.depth), _ptr(self.alpha), _ptr(self.radii))
        self.tile_rows = tile_rows
        self._st = L.orc_forward(*args) if tile_rows is None else L.orc_forward_rows(*args, int(tile_rows[0]), int(tile_rows[1]))
        cnt = np.zeros(4, np.int64)
        L.orc_get_counts(self._st, _ptr(cnt))
        self.num_duplicates, self.num_visible, self.max_tile_list, self.num_tiles = [int(v) for v in cnt]
        assert P >= 0

    def tiles_touched(self):
        out = np.zeros(self.N, np.int32)
        lib().orc_get_tiles_touched(self._st, _ptr(out))
        return out

    def n_contrib(self):
        out = np.zeros((self.H, self.W), np.uint32)
        lib().orc_get_n_contrib(self._st, _ptr(out))
        return out

    def decision_margins(self):
        """(alpha, T, power): the smallest relative distance of any per-pixel compositing decision to its threshold
        (1/255, 1e-4, 0) -- see orc_decision_margins. A float32 implementation with another exponential may decide a pair
        closer than a few 1e-6 the other way."""
        out = np.zeros(3, np.float64)
        lib().orc_decision_margins(self._st, C.byref(self.frame), _ptr(out))
        return dict(alpha=float(out[0]), T=float(out[1]), power=float(out[2]))

    def tile_lists(self):
        starts = np.zeros(self.num_tiles + 1, np.int64)
        lst = np.zeros(max(self.num_duplicates, 1), np.uint32)
        lib().orc_get_tile_lists(self._st, _ptr(starts), _ptr(lst))
        return starts, lst[: self.num_duplicates]

    def geom(self):
        out = np.zeros((self.N, 12), np.float32)
        lib().orc_get_geom(self._st, _ptr(out))
        return out

    def pixel_margins(self):
        """[H,W,3] float64: per pixel, the smallest alpha margin, T margin and |power| of orc_decision_margins (1e30
        where the pixel never reaches the test) -- see orc_pixel_margins."""
        out = np.zeros((self.H, self.W, 3), np.float64)
        lib().orc_pixel_margins(self._st, C.byref(self.frame), _ptr(out))
        return out

    def chain_state(self):
        """[N,16] float64 of the float32 per-Gaussian state the backward chain reads: a0,b0,c0, tx,ty,tz, cov3d[6],
        coef, clamped[3]."""
        out = np.zeros((self.N, 16), np.float64)
        lib().orc_get_chain_state(self._st, _ptr(out))
        return out

    def backward(self, dL_dcolor=None, dL_ddepth=None, dL_dalpha=None, export=False):
        """export=True: also returns, under "_sums", the [N,22] float64 per-Gaussian sums of orc_backward_ex (the twelve
        signed accumulators, then the ten magnitude sums of the raw terms). The gradients are the same bits either way."""
        k = self._keep
        N = self.N
        g = dict(means3D=np.zeros((N, 3), np.float32), means2D=np.zeros((N, 3), np.float32),
                 scales=np.zeros((N, 3), np.float32), rotations=np.zeros((N, 4), np.float32),
                 opacities=np.zeros((N, 1), np.float32))
        gcol = np.zeros((N, 3), np.float32) if k["colors"] is not None else None
        gsh = np.zeros((N, self.sh_coeffs, 3), np.float32) if k["shs"] is not None else None
        dc, dd, da = _f32(dL_dcolor), _f32(dL_ddepth), _f32(dL_dalpha)
        sums = np.zeros((N, EXPORT_WORDS), np.float64) if export else None
        args = (self._st, C.byref(self.frame), _ptr(k["means3D"]), _ptr(k["scales"]),
                _ptr(k["rotations"]), _ptr(k["opacities"]), _ptr(k["colors"]), _ptr(k["shs"]),
                _ptr(self.alpha), _ptr(dc), _ptr(dd), _ptr(da), _ptr(g["means3D"]),
                _ptr(g["means2D"]), _ptr(g["scales"]), _ptr(g["rotations"]),
                _ptr(g["opacities"]), _ptr(gcol), _ptr(gsh))
        rc = self._L.orc_backward_ex(*args, _ptr(sums)) if export else self._L.orc_backward(*args)
        assert rc == 0
        if export:
            g["_sums"] = sums
        if gcol is not None:
            g["colors_precomp"] = gcol
        if gsh is not None:
            g["shs"] = gsh
        return g

    def close(self):
        if self._st:
            self._L.orc_free(self._st)
            self._st = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ssim(img1, img2, want_grad=False):
    a, b = _f32(img1), _f32(img2)
    assert a.ndim == 4 and a.shape == b.shape
    B, Cc, H, W = a.shape
    smap = np.zeros_like(a)
    grad = np.zeros_like(a) if want_grad else None
    val = lib().orc_ssim(_ptr(a), _ptr(b), B, Cc, H, W, _ptr(smap), _ptr(grad))
    return (val, smap, grad) if want_grad else (val, smap)


def knn_dist2(xyz):
    a = _f32(xyz)
    out = np.zeros(a.shape[0], np.float32)
    lib().orc_knn_dist2(_ptr(a), a.shape[0], _ptr(out))
    return out


# ---- helper hooks (checked against tests/golden, generated from the reference's own Python) -------------
def make_frame_struct(frame, sh_coeffs=0, keep=None):
    k = dict(subpix=_f32(frame.get("subpix")), bg=_f32(frame["bg"]), view=_f32(frame["view"]),
             proj=_f32(frame["proj"]), campos=_f32(frame["campos"]))
    if keep is not None:
        keep.append(k)
    return OrcFrame(int(frame["H"]), int(frame["W"]), float(frame["tanfovx"]), float(frame["tanfovy"]),
                    float(frame["kernel_size"]), float(frame.get("scale_modifier", 1.0)),
                    int(frame.get("sh_degree", 0)), sh_coeffs, int(frame.get("depth_mode", 0)), _ptr(k["subpix"]),
                    _ptr(k["bg"]), _ptr(k["view"]), _ptr(k["proj"]), _ptr(k["campos"]))


def cov3d(scales, modifier, quats):
    s, q = _f32(scales), _f32(quats)
    out = np.zeros((s.shape[0], 6), np.float32)
    for i in range(s.shape[0]):
        lib().orc_test_cov3d(_ptr(s[i]), float(modifier), _ptr(q[i]), _ptr(out[i]))
    return out


def quat_to_R(quats):
    q = _f32(quats)
    out = np.zeros((q.shape[0], 9), np.float32)
    for i in range(q.shape[0]):
        lib().orc_test_quat_to_R(_ptr(q[i]), _ptr(out[i]))
    return out.reshape(-1, 3, 3)


def sh_rgb(deg, sh_km3, dirs):
    """sh_km3 [N,M,3] (coefficient-major, as the rasterizer receives it), dirs [N,3] unit."""
    sh, d = _f32(sh_km3), _f32(dirs)
    out = np.zeros((sh.shape[0], 3), np.float32)
    for i in range(sh.shape[0]):
        lib().orc_test_sh(int(deg), int(sh.shape[1]), _ptr(sh[i]), _ptr(d[i]), _ptr(out[i]))
    return out


def project(frame, means3D, scales, quats):
    keep = []
    fr = make_frame_struct(frame, keep=keep)
    p, s, q = _f32(means3D), _f32(scales), _f32(quats)
    out = np.zeros((p.shape[0], 4), np.float32)
    for i in range(p.shape[0]):
        lib().orc_test_project(C.byref(fr), _ptr(p[i]), _ptr(s[i]), _ptr(q[i]), _ptr(out[i]))
    return out
