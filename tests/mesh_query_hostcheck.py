"""ctypes front-end of tests/host_check/mesh_query_check.cpp: the product's csrc/mesh_query_math.h (the cell function, the cells of
a face, the closest point of a triangle, the ring search's bounds, the sampler's area, mixer and positions that
csrc/mesh_query.hip uses on the device) built with g++ -ffp-contract=off and driven by plain sequential loops. Test
infrastructure only; needs neither torch nor a GPU."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "host_check", "mesh_query_check.cpp")
_CSRC = os.path.join(_HERE, "..", "skyfall-gs_amd", "csrc")
_DEPS = [os.path.join(_CSRC, h) for h in ("mesh_query_math.h", "mesh_math.h")]
_OUT = os.path.join(_HERE, "host_check", "_build", "libmeshquerycheck.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        newest = max(os.path.getmtime(p) for p in [_SRC] + _DEPS)
        if not os.path.exists(_OUT) or os.path.getmtime(_OUT) < newest:
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                                   "-o", _OUT, _SRC])
        _lib = C.CDLL(_OUT)
        V, LL, D, U = C.c_void_p, C.c_longlong, C.c_double, C.c_uint32
        _lib.mqc_cell.restype, _lib.mqc_cell.argtypes = D, [D, D, D]
        _lib.mqc_area.restype, _lib.mqc_area.argtypes = D, [V]
        _lib.mqc_mix3.restype, _lib.mqc_mix3.argtypes = U, [U, U, U]
        _lib.mqc_closest_faces.restype, _lib.mqc_closest_faces.argtypes = None, [V, V, V, LL, LL, V, V]
        _lib.mqc_grid.restype, _lib.mqc_grid.argtypes = None, [V, V, LL, LL, V, D, V, LL, V, V, LL, V, V]
        _lib.mqc_search.restype = None
        _lib.mqc_search.argtypes = [V, V, LL, LL, V, D, V, V, V, LL, V, LL, V, LL, D, V, V, V, V, V]
        _lib.mqc_sample.restype, _lib.mqc_sample.argtypes = None, [V, V, V, LL, LL, D, U, LL, V, V, V, V]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p).value


def _mesh(V, F):
    return np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)


def cell_of(x, origin, cell):
    return lib().mqc_cell(float(x), float(origin), float(cell))


def area(tri):
    return lib().mqc_area(_p(np.ascontiguousarray(tri, dtype=np.float32).reshape(9)))


def mix3(seed, face, counter):
    return lib().mqc_mix3(int(seed), int(face), int(counter))


def closest_faces(p, V, F):
    """one point against every face -> (d2 [n], q [n,3]); NaN rows for faces with an index out of range"""
    V, F = _mesh(V, F)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(3)
    d2, q = np.zeros(len(F)), np.zeros((len(F), 3))
    lib().mqc_closest_faces(_p(p), _p(V), _p(F), len(V), len(F), _p(d2), _p(q))
    return d2, q


def face_grid(V, F, cell, origin, dims, max_cells=4096, capacity=None):
    """-> namespace(cell, origin, dims, cell_start, pairs, large (ascending), skipped, status, need)"""
    V, F = _mesh(V, F)
    origin, dims = np.ascontiguousarray(origin, dtype=np.float64), np.ascontiguousarray(dims, dtype=np.int32)
    cells = int(np.prod(dims.astype(np.int64)))
    cell_start, large, state = np.zeros(cells + 1, np.int32), np.zeros(len(F), np.int32), np.zeros(4, np.int64)
    if capacity is None:
        lib().mqc_grid(_p(V), _p(F), len(V), len(F), _p(origin), float(cell), _p(dims), int(max_cells), _p(cell_start), None, 0, _p(large),
                       _p(state))
        capacity = int(state[0])
    pairs = np.full(capacity, -7, np.int32)
    lib().mqc_grid(_p(V), _p(F), len(V), len(F), _p(origin), float(cell), _p(dims), int(max_cells), _p(cell_start), _p(pairs), capacity,
                   _p(large), _p(state))
    return types.SimpleNamespace(cell=float(cell), origin=origin, dims=tuple(int(d) for d in dims), cell_start=cell_start, pairs=pairs,
                                 large=large[:state[1]].copy(), skipped=int(state[3]), status=int(state[2]), need=int(state[0]))


def search(grid, V, F, points, max_distance=np.inf):
    """-> (sqdist, face, point, counts [answered, without], rings)"""
    V, F = _mesh(V, F)
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    k = len(P)
    sq, fo, po = np.zeros(k), np.zeros(k, np.int32), np.zeros((k, 3), np.float32)
    counts, rings = np.zeros(2, np.int64), np.zeros(k, np.int32)
    dims = np.ascontiguousarray(grid.dims, dtype=np.int32)
    origin = np.ascontiguousarray(grid.origin, dtype=np.float64)
    cs, pr, lg = (np.ascontiguousarray(a, dtype=np.int32) for a in (grid.cell_start, grid.pairs, grid.large))
    lib().mqc_search(_p(V), _p(F), len(V), len(F), _p(origin), float(grid.cell), _p(dims), _p(cs), _p(pr), len(pr), _p(lg), len(lg), _p(P), k,
                     float(max_distance), _p(sq), _p(fo), _p(po), _p(counts), _p(rings))
    return sq, fo, po, counts, rings


def sample(V, F, Cc, density, seed=0, capacity=None):
    V, F = _mesh(V, F)
    Cc = None if Cc is None else np.ascontiguousarray(Cc, dtype=np.float32).reshape(-1, 3)
    state = np.zeros(4, np.int64)
    if capacity is None:
        lib().mqc_sample(_p(V), _p(Cc), _p(F), len(V), len(F), float(density), int(seed), 0, None, None, None, _p(state))
        capacity = int(state[0])
    points, face = np.zeros((capacity, 3), np.float32), np.zeros(capacity, np.int32)
    colors = None if Cc is None else np.zeros((capacity, 3), np.float32)
    lib().mqc_sample(_p(V), _p(Cc), _p(F), len(V), len(F), float(density), int(seed), capacity, _p(points), _p(face), _p(colors), _p(state))
    return types.SimpleNamespace(points=points, face=face, colors=colors, count=int(state[0]), status=int(state[2]))
