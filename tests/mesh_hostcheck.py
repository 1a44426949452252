"""ctypes front-end of tests/host_check/mesh_check.cpp: the product's csrc/mesh_math.h (the vertex key, its hash, the table size
and the face rules that csrc/mesh.hip uses on the device) built with g++ -ffp-contract=off and driven by plain sequential loops.
Test infrastructure only; needs neither torch nor a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "host_check", "mesh_check.cpp")
_DEPS = [os.path.join(_HERE, "..", "skyfall-gs_amd", "csrc", "mesh_math.h")]
_OUT = os.path.join(_HERE, "host_check", "_build", "libmeshcheck.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        newest = max(os.path.getmtime(p) for p in [_SRC] + _DEPS)
        if not os.path.exists(_OUT) or os.path.getmtime(_OUT) < newest:
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o", _OUT, _SRC])
        _lib = C.CDLL(_OUT)
        _lib.mc_slots.restype, _lib.mc_slots.argtypes = C.c_ulonglong, [C.c_longlong]
        _lib.mc_hash.restype, _lib.mc_hash.argtypes = C.c_uint32, [C.c_uint32] * 3
        _lib.mc_degenerate.restype, _lib.mc_degenerate.argtypes = C.c_int, [C.c_int32] * 3
        _lib.mc_index_ok.restype, _lib.mc_index_ok.argtypes = C.c_int, [C.c_int32, C.c_longlong]
        _lib.mc_weld.restype = C.c_longlong
        _lib.mc_weld.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p).value


def weld(vertices, colors=None):
    """mesh_np.weld's arguments -> (V, F int32, colours or None, the table's slots, the slots looked at in all)"""
    soup = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3, 3)
    cols = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(-1, 3, 3)
    n = len(soup)
    V = np.zeros((max(3 * n, 1), 3), np.float32)
    Cc = None if cols is None else np.zeros((max(3 * n, 1), 3), np.float32)
    F = np.zeros((max(n, 1), 3), np.int32)
    probes = C.c_ulonglong(0)
    m = lib().mc_weld(_p(soup), _p(cols), n, _p(V), _p(Cc), _p(F), C.byref(probes))
    assert m >= 0, m
    return V[:m], F[:n], None if Cc is None else Cc[:m], int(lib().mc_slots(n)), int(probes.value)
