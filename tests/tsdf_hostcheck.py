"""ctypes front-end of tests/host_check/tsdf_check.cpp: the product's csrc/tsdf_math.h (the per-voxel TSDF update and the per-cell
marching-tetrahedra triangulation that csrc/tsdf.hip runs on the device) built with g++ -ffp-contract=off and driven by plain
loops. Test infrastructure only; needs neither torch nor a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import consistency_np as cnp
from sfgs import _lib as L

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "host_check", "tsdf_check.cpp")
_DEPS = [os.path.join(_HERE, "..", "skyfall-gs_amd", "csrc", n) for n in ("tsdf_math.h", "geo_unproject.h")] + \
        [os.path.join(_HERE, "..", "include", "sfgs.h")]
_OUT = os.path.join(_HERE, "host_check", "_build", "libtsdfcheck.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        newest = max(os.path.getmtime(p) for p in [_SRC] + _DEPS)
        if not os.path.exists(_OUT) or os.path.getmtime(_OUT) < newest:
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o", _OUT, _SRC])
        _lib = C.CDLL(_OUT)
        _lib.tc_integrate.restype = C.c_int
        _lib.tc_integrate.argtypes = [C.POINTER(L.SfgsTsdfVolume), C.POINTER(L.SfgsTsdfView), C.c_int32, C.c_void_p]
        _lib.tc_extract.restype = C.c_longlong
        _lib.tc_extract.argtypes = [C.POINTER(L.SfgsTsdfVolume), C.c_void_p, C.c_void_p, C.c_longlong]
        for name in ("tc_tet_corner", "tc_winding_swap"):
            getattr(_lib, name).restype, getattr(_lib, name).argtypes = C.c_int, [C.c_int, C.c_int]
        _lib.tc_tet_triangles.restype, _lib.tc_tet_triangles.argtypes = C.c_int, [C.c_int]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p).value


def _volume(origin, voxel_size, trunc, max_weight, tsdf, weight, rgb):
    nz, ny, nx = tsdf.shape
    return L.SfgsTsdfVolume(C.sizeof(L.SfgsTsdfVolume), nx, ny, nz, (C.c_double * 3)(*origin), float(voxel_size), float(trunc),
                            float(max_weight), _p(tsdf), _p(weight), _p(rgb))


def integrate(state, vol, views, images=None):
    """tsdf_np.integrate's arguments -> `state` updated in place, and the int64 [5] outcome counts (behind, outside, unused,
    beyond the truncation, updated)."""
    keep, records = [], (L.SfgsTsdfView * len(views))()
    for n, v in enumerate(views):
        H, W = v.depth.shape
        k = cnp.constants(v.camera, H, W)
        depth = np.ascontiguousarray(v.depth, dtype=np.float32)
        mask = None if v.mask is None else np.ascontiguousarray(v.mask).astype(np.uint8)
        image = None if images is None else np.ascontiguousarray(images[n], dtype=np.float32)
        keep.append((depth, mask, image))
        records[n] = L.SfgsTsdfView(_p(depth), _p(mask), _p(image), H, W, (C.c_double * 9)(*k.M.reshape(-1)), (C.c_double * 3)(*k.c),
                                    k.cx_pix, k.cy_pix, k.focal_x, k.focal_y)
    outcomes = np.zeros(5, dtype=np.int64)
    v = _volume(vol.origin, vol.voxel_size, vol.trunc, vol.max_weight, state.tsdf, state.weight, state.rgb)
    assert lib().tc_integrate(C.byref(v), records, len(views), _p(outcomes)) == 0
    return outcomes


def extract(tsdf, weight, origin, voxel_size, rgb=None, capacity=None):
    """tsdf_np.extract's arguments -> (vertices float32 [n,3,3], colors or None, the count); capacity defaults to 12 per cell."""
    tsdf, weight = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.float32)
    rgb = None if rgb is None else np.ascontiguousarray(rgb, np.float32)
    nz, ny, nx = tsdf.shape
    if capacity is None:
        capacity = 12 * max(nx - 1, 0) * max(ny - 1, 0) * max(nz - 1, 0)
    vertices = np.zeros((max(capacity, 1), 3, 3), np.float32)
    colors = None if rgb is None else np.zeros((max(capacity, 1), 3, 3), np.float32)
    v = _volume(origin, voxel_size, 1.0, 1.0, tsdf, weight, rgb)
    n = lib().tc_extract(C.byref(v), _p(vertices), _p(colors), capacity)
    assert n >= 0, n
    return vertices[:min(n, capacity)], None if colors is None else colors[:min(n, capacity)], n
