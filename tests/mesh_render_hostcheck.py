"""ctypes front-end of tests/host_check/mesh_render_check.cpp: the product's csrc/mesh_raster_math.h (the vertex record, the face
set-up, the edge functions and their tie-break, depth, key and attributes that csrc/mesh_raster.hip uses on the device) built
with g++ -ffp-contract=off and driven by plain sequential loops. Test infrastructure only; needs neither torch nor a GPU."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import consistency_np as cnp

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "host_check", "mesh_render_check.cpp")
_CSRC = os.path.join(_HERE, "..", "skyfall-gs_amd", "csrc")
_DEPS = [os.path.join(_CSRC, h) for h in ("mesh_raster_math.h", "mesh_math.h", "geo_unproject.h")]
_OUT = os.path.join(_HERE, "host_check", "_build", "libmeshrendercheck.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        newest = max(os.path.getmtime(p) for p in [_SRC] + _DEPS)
        if not os.path.exists(_OUT) or os.path.getmtime(_OUT) < newest:
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o", _OUT, _SRC])
        _lib = C.CDLL(_OUT)
        V, LL, D, I = C.c_void_p, C.c_longlong, C.c_double, C.c_int
        _lib.mrc_camera_sign.restype, _lib.mrc_camera_sign.argtypes = I, [V]
        _lib.mrc_project.restype = I
        _lib.mrc_project.argtypes = [V, V, D, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(D)]
        _lib.mrc_face.restype, _lib.mrc_face.argtypes = I, [V, I, I, C.POINTER(LL), C.POINTER(I)]
        _lib.mrc_covers.restype, _lib.mrc_covers.argtypes = I, [V, I, I, V, V]
        _lib.mrc_render.restype = I
        _lib.mrc_render.argtypes = [V, D, D, I, I, I, V, V, V, V, LL, LL, V, V, V, V, V, V]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p).value


def camera_words(k):
    """consistency_np.constants -> the sixteen doubles the check takes"""
    return np.ascontiguousarray(np.concatenate([k.M.reshape(-1), k.c, [k.cx_pix, k.cy_pix, k.focal_x, k.focal_y]]), dtype=np.float64)


def camera_sign(k):
    return lib().mrc_camera_sign(_p(camera_words(k)))


def project(k, p, near=0.0):
    """-> (usable, X, Y, z) of one float32 position"""
    cam, p = camera_words(k), np.ascontiguousarray(p, dtype=np.float32).reshape(3)
    X, Y, z = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
    ok = lib().mrc_project(_p(cam), _p(p), float(near), C.byref(X), C.byref(Y), C.byref(z))
    return bool(ok), X.value, Y.value, z.value


def face(xy, camera_sign=1, cull=False):
    """three snapped corners -> (outcome, A, sgn)"""
    xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(6)
    A, sgn = C.c_longlong(0), C.c_int(0)
    outcome = lib().mrc_face(_p(xy), int(camera_sign), int(bool(cull)), C.byref(A), C.byref(sgn))
    return outcome, A.value, sgn.value


def covers(xy, col, row):
    """-> (covered, E [3], owns_zero [3]) of a drawn face at a pixel"""
    xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(6)
    E, owns = np.zeros(3, np.int64), np.zeros(3, np.int32)
    rc = lib().mrc_covers(_p(xy), int(col), int(row), _p(E), _p(owns))
    assert rc >= 0, "the face is not drawn"
    return bool(rc), E, owns.astype(bool)


def render(V, F, Cc, camera, H, W, near=0.0, far=np.inf, normals=True, cull=None):
    """mesh_render_np.render's arguments -> a namespace with its fields (but setup)"""
    V = np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3)
    F = np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)
    Cc = None if Cc is None else np.ascontiguousarray(Cc, dtype=np.float32).reshape(-1, 3)
    vn = None if isinstance(normals, (bool, np.bool_)) else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    want_normal = vn is not None or bool(normals)
    cam = camera_words(cnp.constants(camera, H, W))
    depth, face_out, cover = np.zeros((1, H, W), np.float32), np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    normal = np.zeros((3, H, W), np.float32) if want_normal else None
    rgb = None if Cc is None else np.zeros((3, H, W), np.float32)
    counts = np.zeros(4, np.int64)
    status = lib().mrc_render(_p(cam), float(near), float(far), int(cull == "back"), H, W, _p(V), _p(Cc), _p(F), _p(vn), len(V), len(F),
                              _p(depth), _p(face_out), _p(normal), _p(rgb), _p(counts), _p(cover))
    return types.SimpleNamespace(depth=depth, face=face_out, normal=normal, rgb=rgb, counts=counts, status=status, cover=cover)
