"""Host tests of sfgs.mesh: the numpy restatement tests/mesh_np.py against the committed host weld (tsdf_np.weld) and a plain
Python breadth-first search, its clean rules on the islands scene, the host build of csrc/mesh_math.h against the restatement
byte for byte, the PLY writer read back, and the library's refusals through ctypes. No GPU: every refusal is made before any GPU
work, and the writer is driven through CPU tensors."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import mesh_hostcheck as mhc
import mesh_np as mnp
import tsdf_np as tnp
from sfgs import _lib as L

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
E_ARG = -1
ENTRY_POINTS = ("sfgs_mesh_weld_scratch_bytes", "sfgs_mesh_weld", "sfgs_mesh_vet", "sfgs_mesh_components_scratch_bytes",
                "sfgs_mesh_components", "sfgs_mesh_clean_scratch_bytes", "sfgs_mesh_clean")
VOID12 = np.dtype((np.void, 12))


@functools.lru_cache(maxsize=None)
def islands():
    case = mnp.islands_volume()
    verts, cols = tnp.extract(case[0], case[1], case[3], case[4], case[2])
    V, F, Cc = mnp.weld(verts, cols)
    for a in (verts, cols, V, F, Cc):
        a.setflags(write=False)
    return verts, cols, V, F, Cc


def by_rank(F, m):
    label, triangles, vertices_in, count = mnp.components(F, m)
    roots = np.nonzero(label == np.arange(m))[0]
    return [(int(triangles[r]), int(vertices_in[r]), int(r)) for r in sorted(roots, key=lambda r: (-triangles[r], r))], count


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_weld_restatement_against_the_committed_host_weld():
    verts, cols, V, F, Cc = islands()
    assert len(verts) == 17338 and len(V) == 8704 and F.dtype == np.int32 and F.shape == (17338, 3)
    hostV, hostF = tnp.weld(verts)
    keys = np.ascontiguousarray(V).view(VOID12).reshape(-1)
    assert len(np.unique(keys)) == len(V)                                             # no vertex twice
    assert np.sort(keys).tobytes() == np.ascontiguousarray(hostV).view(VOID12).reshape(-1).tobytes()      # byte-sorted V is the host weld's
    assert V[F].tobytes() == verts.tobytes() and hostV[hostF].tobytes() == verts.tobytes()                # both index the same soup
    flat, cflat = verts.reshape(-1, 3), cols.reshape(-1, 3)
    first = np.full(len(V), len(flat))
    np.minimum.at(first, F.reshape(-1), np.arange(len(flat)))
    assert (np.diff(first) > 0).all()                                                 # numbered in order of first appearance
    assert Cc.tobytes() == cflat[first].tobytes() and V.tobytes() == flat[first].tobytes()
    assert mnp.weld(np.zeros((0, 3, 3), np.float32))[0].shape == (0, 3)


def test_components_restatement_against_a_breadth_first_search():
    _, _, V, F, _ = islands()
    ranked, count = by_rank(F, len(V))
    assert count == 8 and sorted(ranked) == mnp.bfs_components(F, len(V))
    assert ranked == [(7442, 3766, 405), (5044, 2524, 3629), (3128, 1566, 0), (1144, 574, 6944), (484, 220, 48), (48, 26, 8576),
                      (24, 14, 94), (24, 14, 8690)]
    assert int(mnp.degenerate(F).sum()) == 48
    # a vertex in no face is its own component; a degenerate face still joins and still counts
    F2 = np.array([[0, 1, 2], [4, 4, 5], [2, 2, 2]], np.int32)
    label, triangles, vertices_in, count = mnp.components(F2, 7)
    assert label.tolist() == [0, 0, 0, 3, 4, 4, 6] and count == 4
    assert triangles.tolist() == [2, 0, 0, 0, 1, 0, 0] and vertices_in.tolist() == [3, 0, 0, 1, 2, 0, 1]
    assert sorted(mnp.bfs_components(F2, 7)) == [(0, 1, 3), (0, 1, 6), (1, 2, 4), (2, 3, 0)]
    Vs, Fs = mnp.strip_mesh(2000)
    assert mnp.components(Fs, len(Vs))[3] == 1 and mnp.bfs_components(Fs, len(Vs)) == [(2000, 2002, 0)]


def test_clean_rules_tie_break_degenerates_and_identity():
    _, _, V, F, Cc = islands()
    label = mnp.components(F, len(V))[0]

    def labels_left(Fo, Vo):
        # the cleaned mesh's components, named by the INPUT label of their vertices (positions are unique: weld)
        pos = {bytes(r): k for k, r in enumerate(np.ascontiguousarray(V).view(VOID12).reshape(-1))}
        src = np.array([pos[bytes(r)] for r in np.ascontiguousarray(Vo).view(VOID12).reshape(-1)], dtype=np.int64)
        return sorted(set(label[src].tolist()))

    Vo, Fo, Co = mnp.clean(V, F, Cc, largest=100)
    assert Vo.tobytes() == V.tobytes() and Fo.tobytes() == F.tobytes() and Co.tobytes() == Cc.tobytes()   # keeps everything
    Vo, Fo, _ = mnp.clean(V, F, Cc, min_triangles=25)
    assert len(Fo) == 17338 - 48 and labels_left(Fo, Vo) == [0, 48, 405, 3629, 6944, 8576]
    Vo, Fo, _ = mnp.clean(V, F, Cc, largest=7)                                        # 24 against 24: the smaller label stays
    assert len(Fo) == 17338 - 24 and labels_left(Fo, Vo) == [0, 48, 94, 405, 3629, 6944, 8576]
    Vo, Fo, _ = mnp.clean(V, F, Cc, largest=1)
    assert (len(Fo), len(Vo)) == (7442, 3766) and labels_left(Fo, Vo) == [405]
    Vo, Fo, _ = mnp.clean(V, F, Cc, min_triangles=100, largest=7)
    assert labels_left(Fo, Vo) == [0, 48, 405, 3629, 6944]
    Vo, Fo, _ = mnp.clean(V, F, Cc, min_triangles=3000, largest=2)
    assert labels_left(Fo, Vo) == [405, 3629]
    Vo, Fo, Co = mnp.clean(V, F, Cc, drop_degenerate=True)
    assert len(Fo) == 17338 - 48 and not mnp.degenerate(Fo).any() and len(Vo) <= len(V)
    assert V[F[~mnp.degenerate(F)]].tobytes() == Vo[Fo].tobytes()                     # the same triangles, in the same order
    Vo, Fo, _ = mnp.clean(V, F, Cc, largest=0)
    assert len(Vo) == 0 and len(Fo) == 0
    # triangles counts degenerate faces too: a component of three degenerate faces passes min_triangles = 3 and is then emptied
    F2 = np.array([[0, 0, 1], [1, 1, 0], [0, 1, 1], [2, 3, 4]], np.int32)
    V2 = np.arange(15, dtype=np.float32).reshape(5, 3)
    Vo, Fo, _ = mnp.clean(V2, F2, None, min_triangles=3)
    assert Fo.tolist() == [[0, 0, 1], [1, 1, 0], [0, 1, 1]] and Vo.tobytes() == V2[:2].tobytes()
    Vo, Fo, _ = mnp.clean(V2, F2, None, min_triangles=3, drop_degenerate=True)
    assert len(Vo) == 0 and len(Fo) == 0


# ---- the host build of mesh_math.h -----------------------------------------------------------------------------------------------
def test_host_build_welds_byte_for_byte():
    verts, cols, V, F, Cc = islands()
    hV, hF, hC, slots, probes = mhc.weld(verts, cols)
    assert hV.tobytes() == V.tobytes() and hF.tobytes() == F.tobytes() and hC.tobytes() == Cc.tobytes()
    assert slots == 131072 >= 6 * len(verts) > slots // 2 and probes >= 3 * len(verts)
    print(f"islands: load factor {len(V) / slots:.4f}, mean probe length {probes / (3 * len(verts)):.4f}")
    # the hash spreads lattice positions: linear probing under a uniform hash at load a = 0.066 looks at (1 + 1 / (1 - a)^2) / 2 =
    # 1.07 slots per insertion and (1 + 1 / (1 - a)) / 2 = 1.04 per later match; 1.5 would mean clustering, not chance
    assert probes / (3 * len(verts)) < 1.5
    soup = mnp.special_soup()
    sV, sF, _ = mnp.weld(soup)
    hV, hF, _, _, _ = mhc.weld(soup)
    assert hV.tobytes() == sV.tobytes() and hF.tobytes() == sF.tobytes() and len(sV) == 11
    assert sF.tolist() == [[0, 1, 2], [3, 1, 4], [5, 6, 5], [7, 5, 0], [8, 9, 3], [6, 2, 10]]
    same = np.full((500, 3, 3), 1.25, np.float32)
    hV, hF, _, _, _ = mhc.weld(same)
    assert len(hV) == 1 and not hF.any()
    rng = np.random.default_rng(1)
    distinct = rng.random((700, 3, 3), dtype=np.float32)
    hV, hF, _, _, _ = mhc.weld(distinct)
    assert hV.tobytes() == distinct.tobytes() and hF.reshape(-1).tolist() == list(range(2100))
    assert mhc.weld(np.zeros((0, 3, 3), np.float32))[0].shape == (0, 3)
    lib = mhc.lib()
    assert [lib.mc_slots(n) for n in (0, 1, 10, 11, 1 << 29)] == [64, 64, 64, 128, 1 << 32]
    assert lib.mc_degenerate(1, 2, 3) == 0 and all(lib.mc_degenerate(*f) == 1 for f in ((1, 1, 2), (1, 2, 2), (1, 2, 1), (3, 3, 3)))
    assert lib.mc_index_ok(0, 1) == 1 and lib.mc_index_ok(-1, 5) == 0 and lib.mc_index_ok(5, 5) == 0 and lib.mc_index_ok(4, 5) == 1
    assert lib.mc_hash(0, 0, 0) != lib.mc_hash(0x80000000, 0, 0) != lib.mc_hash(0, 0x80000000, 0)


# ---- the writer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", (None, (500000.25, 4100000.5, -3.0)))
def test_save_ply_read_back(tmp_path, origin):
    from sfgs.mesh import Mesh
    _, _, V, F, Cc = islands()
    Cc = Cc.copy()
    Cc[3] = [np.nan, -0.5, 7.0]
    state = torch.tensor([len(V), len(F), 0, 0], dtype=torch.int64)
    spare = 5                                                                         # rows beyond the counts are not written out
    mesh = Mesh._made(torch.from_numpy(np.concatenate([V, np.full((spare, 3), 9, np.float32)])),
                      torch.from_numpy(np.concatenate([F, np.zeros((spare, 3), np.int32)])),
                      torch.from_numpy(np.concatenate([Cc, np.zeros((spare, 3), np.float32)])), state, "test")
    path = str(tmp_path / "sub" / "mesh.ply")
    mesh.save_ply(path, origin=origin)
    xyz, rgb, faces = mnp.read_ply(path)
    if origin is None:
        assert xyz.dtype == np.float32 and xyz.tobytes() == V.tobytes()
    else:
        assert xyz.dtype == np.float64 and xyz.tobytes() == (V.astype(np.float64) + np.array(origin)).tobytes()
    assert faces.tobytes() == F.tobytes() and rgb.tobytes() == mnp.ply_vertex_colors(Cc).tobytes()
    assert rgb[3].tolist() == [0, 0, 255]
    plain = Mesh._made(mesh.vertex_buffer, mesh.face_buffer, None, state, "test")
    plain.save_ply(path)
    xyz, rgb, faces = mnp.read_ply(path)
    assert rgb is None and xyz.tobytes() == V.tobytes() and faces.tobytes() == F.tobytes()
    with pytest.raises(ValueError):
        mesh.save_ply(path, origin=(1.0, 2.0))
    # a status left by the kernels surfaces at the one host read
    with pytest.raises(ValueError, match="face index"):
        Mesh._made(mesh.vertex_buffer, mesh.face_buffer, None, torch.tensor([len(V), len(F), 8, 0]), "test").vertices
    with pytest.raises(RuntimeError, match="trip bound"):
        Mesh._made(mesh.vertex_buffer, mesh.face_buffer, None, torch.tensor([len(V), len(F), 2, 0]), "test").faces


def test_wrong_arguments_raise_value_error_without_a_gpu():
    from sfgs import mesh as M
    soup = torch.zeros((4, 3, 3))
    for call in (lambda: M.weld(soup), lambda: M.weld(soup.double()), lambda: M.weld(soup[:, :2]), lambda: M.weld(soup.reshape(-1, 3)),
                 lambda: M.weld(soup, colors=soup[:3]), lambda: M.weld(soup, num_triangles=5), lambda: M.weld(soup, num_triangles=-1),
                 lambda: M.weld(soup, num_triangles=True), lambda: M.weld(None),
                 lambda: M.Mesh(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32)),
                 lambda: M.Mesh(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int64)),
                 lambda: M.Mesh(torch.zeros((3, 2)), torch.zeros((1, 3), dtype=torch.int32)),
                 lambda: M.Mesh(torch.zeros((0, 3)), torch.zeros((1, 3), dtype=torch.int32)),
                 lambda: M.Mesh(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32), colors=torch.zeros((2, 3)))):
        with pytest.raises(ValueError):
            call()
    mesh = M.Mesh._made(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32), None, torch.tensor([3, 1, 0, 0]), "test")
    for kw in ({"min_triangles": -1}, {"largest": 1.5}, {"largest": True}, {"drop_degenerate": 1}, {"components": object()}):
        with pytest.raises(ValueError):
            mesh.clean(**kw)


# ---- header, library, binding ----------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfgs.h"
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    declared_version = int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1))
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() == 28         # symbols were added, nothing else moved


def test_the_library_refuses_bad_arguments_before_any_gpu_work():
    lib = L.load()
    dummy = (C.c_double * 8)()
    p = C.cast(dummy, C.c_void_p).value                   # never dereferenced: every call below is refused first
    big = 1 << 40

    def refused(rc, what):
        assert rc == E_ARG, what
        assert lib.sfgs_last_error(), what

    assert lib.sfgs_mesh_weld_scratch_bytes(-1) == 0 and lib.sfgs_mesh_weld_scratch_bytes((1 << 29) + 1) == 0
    assert lib.sfgs_mesh_weld_scratch_bytes(0) > 0
    n = 1000
    slots = 8192                                                                      # the power of two >= 6 n
    assert lib.sfgs_mesh_weld_scratch_bytes(n) >= slots * 4 + 3 * n * 4 + 3 * n + lib.sfgs_compact_scratch_bytes(3 * n)
    assert lib.sfgs_mesh_weld_scratch_bytes(1 << 29) >= (1 << 32) * 4
    for bad, what in (((p, None, -1, p, None, p, p, 0, p, big, None), "n < 0"),
                      ((p, None, (1 << 29) + 1, p, None, p, p, 0, p, big, None), "n > 2^29"),
                      ((p, None, 5, p, None, p, None, 0, p, big, None), "NULL state"),
                      ((None, None, 5, p, None, p, p, 0, p, big, None), "NULL soup"),
                      ((p, None, 5, None, None, p, p, 0, p, big, None), "NULL vertices"),
                      ((p, None, 5, p, None, None, p, 0, p, big, None), "NULL faces"),
                      ((p, None, 5, p, None, p, p, 0, None, big, None), "NULL scratch"),
                      ((p, p, 5, p, None, p, p, 0, p, big, None), "colours in, none out"),
                      ((p, None, 5, p, p, p, p, 0, p, big, None), "colours out, none in"),
                      ((p, None, 5, p, None, p, p, 2, p, big, None), "unknown flag"),
                      ((p, None, 5, p, None, p, p, 0, p, 100, None), "scratch too small")):
        refused(lib.sfgs_mesh_weld(*bad), what)
    assert b"scratch too small" in lib.sfgs_last_error()
    for bad, what in (((p, -1, 5, p, None), "n < 0"), ((p, 5, -1, p, None), "m < 0"), ((p, 5, 1 << 31, p, None), "m > int32"),
                      ((p, 5, 5, None, None), "NULL state"), ((None, 5, 5, p, None), "NULL faces")):
        refused(lib.sfgs_mesh_vet(*bad), what)
    assert lib.sfgs_mesh_components_scratch_bytes(-1) == 0 and lib.sfgs_mesh_components_scratch_bytes(1 << 31) == 0
    assert lib.sfgs_mesh_components_scratch_bytes(1000) >= 4000
    for bad, what in (((p, -1, 5, p, p, p, p, p, big, None), "n < 0"), ((p, 5, -1, p, p, p, p, p, big, None), "m < 0"),
                      ((p, 5, 0, p, p, p, p, p, big, None), "faces over no vertex"), ((p, 5, 5, None, p, p, p, p, big, None), "NULL labels"),
                      ((p, 5, 5, p, None, p, p, p, big, None), "NULL triangles"), ((p, 5, 5, p, p, None, p, p, big, None), "NULL vertices_in"),
                      ((p, 5, 5, p, p, p, None, p, big, None), "NULL state"), ((p, 5, 5, p, p, p, p, None, big, None), "NULL scratch"),
                      ((None, 5, 5, p, p, p, p, p, big, None), "NULL faces"), ((p, 5, 5, p, p, p, p, p, 8, None), "scratch too small")):
        refused(lib.sfgs_mesh_components(*bad), what)
    assert lib.sfgs_mesh_clean_scratch_bytes(-1, 5) == 0 and lib.sfgs_mesh_clean_scratch_bytes(5, (1 << 29) + 1) == 0
    assert lib.sfgs_mesh_clean_scratch_bytes(1000, 2000) >= 3000 + lib.sfgs_compact_scratch_bytes(1000) + lib.sfgs_compact_scratch_bytes(2000)
    ok = [p, None, p, 5, 5, p, p, 0, p, None, p, p, p, big, None]

    def clean_with(**kw):
        names = ("vertices", "colors", "faces", "m", "n", "labels", "keep_root", "drop", "vertices_out", "colors_out", "faces_out",
                 "state", "scratch", "scratch_bytes", "stream")
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.sfgs_mesh_clean(*a)

    for kw in ({"m": -1}, {"n": -1}, {"m": 0}, {"n": (1 << 29) + 1}, {"vertices": None}, {"faces": None}, {"labels": None},
               {"keep_root": None}, {"vertices_out": None}, {"faces_out": None}, {"state": None}, {"scratch": None}, {"colors": p},
               {"colors_out": p}, {"drop": 2}, {"scratch_bytes": 16}):
        refused(clean_with(**kw), kw)
