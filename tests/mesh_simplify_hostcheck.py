"""ctypes front-end of tests/host_check/mesh_simplify_check.cpp: the product's csrc/mesh_math.h (the cell of a vertex, the
fixed-point means, the sorted triple, the face normal and the normalisation that csrc/mesh.hip uses on the device) built with
g++ -ffp-contract=off and driven by plain sequential loops. Test infrastructure only; needs neither torch nor a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "host_check", "mesh_simplify_check.cpp")
_DEPS = [os.path.join(_HERE, "..", "skyfall-gs_amd", "csrc", "mesh_math.h")]
_OUT = os.path.join(_HERE, "host_check", "_build", "libmeshsimplifycheck.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        newest = max(os.path.getmtime(p) for p in [_SRC] + _DEPS)
        if not os.path.exists(_OUT) or os.path.getmtime(_OUT) < newest:
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o", _OUT, _SRC])
        _lib = C.CDLL(_OUT)
        V, LL = C.c_void_p, C.c_longlong
        _lib.msc_key_slots.restype, _lib.msc_key_slots.argtypes = C.c_ulonglong, [LL]
        _lib.msc_cell_axis.restype = C.c_int
        _lib.msc_cell_axis.argtypes = [C.c_float, C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_ulonglong)]
        _lib.msc_color_fix.restype, _lib.msc_color_fix.argtypes = C.c_ulonglong, [C.c_float]
        _lib.msc_decimate.restype = C.c_int
        _lib.msc_decimate.argtypes = [V, V, V, LL, LL, C.c_double, V, C.c_int, V, V, V, V, V]
        _lib.msc_vertex_faces.restype, _lib.msc_vertex_faces.argtypes = C.c_int, [V, LL, LL, V, V]
        _lib.msc_vertex_normals.restype, _lib.msc_vertex_normals.argtypes = None, [V, V, LL, LL, V, V, V]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p).value


def cell_axis(x, origin, cell):
    """-> (ok, i, p) of one coordinate"""
    i, p = C.c_int32(0), C.c_ulonglong(0)
    ok = lib().msc_cell_axis(float(np.float32(x)), float(origin), float(cell), C.byref(i), C.byref(p))
    return bool(ok), i.value, p.value


def decimate(V, F, Cc=None, cell=1.0, origin=(0.0, 0.0, 0.0), drop_duplicates=True):
    """mesh_simplify_np.decimate's arguments -> (V', F' int32, C' or None, vertex_map int32 [m], status)"""
    V = np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3)
    F = np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)
    Cc = None if Cc is None else np.ascontiguousarray(Cc, dtype=np.float32).reshape(-1, 3)
    m, n = len(V), len(F)
    org = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
    Vo = np.zeros((max(m, 1), 3), np.float32)
    Co = None if Cc is None else np.zeros((max(m, 1), 3), np.float32)
    Fo = np.zeros((max(n, 1), 3), np.int32)
    vmap = np.zeros(max(m, 1), np.int32)
    sizes = np.zeros(3, np.int64)
    rc = lib().msc_decimate(_p(V), _p(Cc), _p(F), m, n, float(cell), _p(org), int(bool(drop_duplicates)), _p(Vo), _p(Co), _p(Fo), _p(vmap),
                            _p(sizes))
    assert rc == 0, rc
    return Vo[:sizes[0]], Fo[:sizes[1]], None if Co is None else Co[:sizes[0]], vmap[:m], int(sizes[2])


def vertex_faces(F, m):
    F = np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)
    offsets, records = np.zeros(m + 1, np.int32), np.zeros(max(3 * len(F), 1), np.int32)
    assert lib().msc_vertex_faces(_p(F), len(F), m, _p(offsets), _p(records)) == 0
    return offsets, records[:3 * len(F)]


def vertex_normals(V, F, adjacency):
    V = np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3)
    F = np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)
    offsets, records = (np.ascontiguousarray(a, dtype=np.int32) for a in adjacency)
    out = np.zeros((max(len(V), 1), 3), np.float32)
    lib().msc_vertex_normals(_p(V), _p(F), len(V), len(F), _p(offsets), _p(records), _p(out))
    return out[:len(V)]
