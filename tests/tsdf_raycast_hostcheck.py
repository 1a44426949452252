"""ctypes front-end of tests/host_check/tsdf_raycast_check.cpp: the ray-cast of the product's csrc/tsdf_math.h (what
tsdf_raycast_kernel of csrc/tsdf.hip runs per pixel, with the uniform and the skipping march, and the empty-space table) built
with g++ -ffp-contract=off and driven by plain loops. Test infrastructure only; needs neither torch nor a GPU."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import consistency_np as cnp
from sfgs import _lib as L

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "host_check", "tsdf_raycast_check.cpp")
_DEPS = [os.path.join(_HERE, "..", "skyfall-gs_amd", "csrc", n) for n in ("tsdf_math.h", "geo_unproject.h")] + \
        [os.path.join(_HERE, "..", "include", "sfgs.h")]
_OUT = os.path.join(_HERE, "host_check", "_build", "libtsdfraycastcheck.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        newest = max(os.path.getmtime(p) for p in [_SRC] + _DEPS)
        if not os.path.exists(_OUT) or os.path.getmtime(_OUT) < newest:
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o", _OUT, _SRC])
        _lib = C.CDLL(_OUT)
        _lib.trc_raycast.restype = C.c_int
        _lib.trc_raycast.argtypes = [C.POINTER(L.SfgsTsdfVolume), C.POINTER(L.SfgsTsdfRay), C.c_void_p, C.c_void_p]
        _lib.trc_skip_build.restype = C.c_int
        _lib.trc_skip_build.argtypes = [C.POINTER(L.SfgsTsdfVolume), C.c_void_p, C.c_size_t]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p).value


def _volume(tsdf, weight, rgb, origin, voxel_size):
    nz, ny, nx = tsdf.shape
    return L.SfgsTsdfVolume(C.sizeof(L.SfgsTsdfVolume), nx, ny, nz, (C.c_double * 3)(*origin), float(voxel_size), 1.0, 1.0,
                            _p(tsdf), _p(weight), _p(rgb))


def skip_table(tsdf, weight):
    """-> uint8 [bz,by,bx], as tsdf_raycast_np.skip_table"""
    tsdf, weight = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.float32)
    nz, ny, nx = tsdf.shape
    bricks = [1 if n < 2 else (n + 6) // 8 for n in (nz, ny, nx)]
    table = np.full(bricks, 7, np.uint8)
    assert lib().trc_skip_build(C.byref(_volume(tsdf, weight, None, (0.0, 0.0, 0.0), 1.0)), _p(table), table.size) == 0
    return table


def raycast(tsdf, weight, rgb, origin, voxel_size, camera, H, W, step=None, near=0.0, far=np.inf, normals=True, skip=False):
    """tsdf_raycast_np.raycast's arguments -> namespace depth, normal, rgb, samples, jumps, longest, longest_run. skip: False for the uniform
    march, True for the skipping march over the table built here."""
    tsdf, weight = np.ascontiguousarray(tsdf, np.float32), np.ascontiguousarray(weight, np.float32)
    rgb = None if rgb is None else np.ascontiguousarray(rgb, np.float32)
    k = cnp.constants(camera, H, W)
    depth = np.full((1, H, W), -7.0, np.float32)
    normal = np.full((3, H, W), -7.0, np.float32) if normals else None
    colour = None if rgb is None else np.full((3, H, W), -7.0, np.float32)
    ray = L.SfgsTsdfRay(C.sizeof(L.SfgsTsdfRay), H, W, (C.c_double * 9)(*k.M.reshape(-1)), (C.c_double * 3)(*k.c), k.cx_pix, k.cy_pix,
                        k.focal_x, k.focal_y, float(near), float(far), float(voxel_size if step is None else step), _p(depth),
                        _p(normal), _p(colour))
    table = skip_table(tsdf, weight) if skip else None
    counters = np.zeros(4, np.int64)
    assert lib().trc_raycast(C.byref(_volume(tsdf, weight, rgb, origin, voxel_size)), C.byref(ray), _p(table), _p(counters)) == 0
    return types.SimpleNamespace(depth=depth, normal=normal, rgb=colour, samples=int(counters[0]), jumps=int(counters[1]),
                                 longest=int(counters[2]), longest_run=int(counters[3]))
