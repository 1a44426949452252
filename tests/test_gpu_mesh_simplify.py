"""GPU tests of Mesh.decimate / vertex_faces / vertex_normals / save_ply(normals=) (csrc/mesh.hip). The reference is the numpy
restatement tests/mesh_simplify_np.py (held to the host build of the product's header and to independent spellings by
tests/test_mesh_simplify_host.py). Nothing here reads the reference tree.

Bounds. Every comparison is assert-equal on the BYTES: positions and colours are integer means resolved by a fixed float64
expression, faces and adjacency are integers, and the normals are float64 sums taken in a fixed order -- there is nothing to
tolerate, and no row or count is left out.

Chunk boundaries of the implementation, and which scene crosses them:
  * every kernel runs workgroups of 256 threads: all scenes span many workgroups and their sizes (8 704 / 17 338, 9 000 / 5 000,
    76 846 / 152 114, 5 002 / 5 000) are no multiples of 256;
  * the three compaction plans of a decimation (first-appearance ranks over m vertex rows, kept clusters over m rows, kept faces
    over n rows) and the adjacency's count scan rank 4 096 rows per workgroup and scan 1 024 workgroups per round with a carry,
    i.e. 4 194 304 rows: the height field of 2 050 x 2 048 vertices (4 198 400 rows, 8 388 606 faces) puts cluster
    representatives, kept faces and vertex counts behind that carry, and is checked against a closed form;
  * the adjacency sorts a segment by insertion up to 32 records and by heapsort beyond: islands reaches valence 63 (both paths),
    the fan's hub 5 000."""
import functools

import numpy as np
import pytest
import torch

import mesh_np as mnp
import mesh_simplify_np as snp
import tsdf_np as tnp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # a copy: the shared scenes are read-only


def same(t, want, what, dtype=torch.float32):
    assert t.device == torch.device(DEV) and t.dtype == dtype, what
    got = t.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == np.ascontiguousarray(want).tobytes(), what


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (volume case, soup, soup colours, V, F, C) through the restatement, once"""
    case = {"islands": mnp.islands_volume, "wavy": lambda: tnp.wavy_volume((72, 64, 64), colors=True)}[name]()
    verts, cols = tnp.extract(case[0], case[1], case[3], case[4], case[2])
    return (case,) + frozen(verts, cols, *mnp.weld(verts, cols))


@functools.lru_cache(maxsize=None)
def device_mesh(name):
    """TsdfVolume.load -> extract -> mesh()"""
    from sfgs.tsdf import TsdfVolume
    case, verts = scene(name)[:2]
    tsdf, weight, rgb, origin, voxel = case
    nz, ny, nx = tsdf.shape
    v = TsdfVolume(origin, (nx, ny, nz), voxel, trunc=1.0, colors=True, device=DEV)
    v.load(dev(tsdf), dev(weight), dev(rgb))
    return v.extract(len(verts)).mesh()


@functools.lru_cache(maxsize=None)
def reference(name, cell, origin, colours=True, drop_duplicates=True):
    _, _, _, V, F, C = scene(name)
    out = snp.decimate(V, F, C if colours else None, cell, origin, drop_duplicates)
    frozen(*out[:4])
    return out


def check_mesh(mesh, V, F, C, what):
    assert (int(mesh.num_vertices), int(mesh.num_faces)) == (len(V), len(F)), what
    same(mesh.vertices, V, f"vertices, {what}")
    same(mesh.faces, F, f"faces, {what}", torch.int32)
    if C is None:
        assert mesh.colors is None
    else:
        same(mesh.colors, C, f"colours, {what}")


def check_decimate(mesh, V, F, C, what, **kw):
    Vo, Fo, Co, vmap, info = snp.decimate(V, F, C, kw["cell"], kw.get("origin", (0.0, 0.0, 0.0)), kw.get("drop_duplicates", True))
    out, got_map = mesh.decimate(return_map=True, **kw)
    check_mesh(out, Vo, Fo, Co, f"decimate {kw}, {what}")
    same(got_map, vmap, f"vertex map, {kw}, {what}", torch.int32)
    assert out.vertex_buffer.shape[0] == len(V) and out.face_buffer.shape[0] == len(F)           # allocated at the input's sizes
    return out, (Vo, Fo, Co, vmap, info)


# ---- 1. islands: TsdfVolume.load -> extract -> mesh() -> decimate --------------------------------------------------------------------
@pytest.mark.parametrize("cell,origin", snp.ISLAND_CASES)
@pytest.mark.parametrize("colours", (True, False))
@pytest.mark.parametrize("drop_duplicates", (True, False))
def test_islands_decimate(cell, origin, colours, drop_duplicates):
    from sfgs.mesh import Mesh
    _, _, _, V, F, C = scene("islands")
    mesh = device_mesh("islands")
    if not colours:
        mesh = Mesh._made(mesh.vertex_buffer, mesh.face_buffer, None, mesh._state, "weld")
    Vo, Fo, Co, vmap, info = reference("islands", cell, origin, colours, drop_duplicates)
    assert info["duplicates"] > 0 and info["single"] > 0 and info["collapsed"] > 0
    out, got_map = mesh.decimate(cell, origin=origin, drop_duplicates=drop_duplicates, return_map=True)
    for s in (out.num_vertices, out.num_faces):
        assert s.device == torch.device(DEV) and s.dtype == torch.int64 and s.dim() == 0
    check_mesh(out, Vo, Fo, Co, (cell, origin, colours, drop_duplicates))
    same(got_map, vmap, "vertex map", torch.int32)
    assert tuple(out.vertex_buffer.shape) == (len(V), 3) and tuple(out.face_buffer.shape) == (len(F), 3)     # the input's sizes
    assert (out.color_buffer is None) == (not colours) and (out.color_buffer is None or out.color_buffer.shape == (len(V), 3))
    plain = mesh.decimate(cell, origin, drop_duplicates)                               # positional, no map: the same mesh
    assert torch.equal(plain.vertices, out.vertices) and torch.equal(plain.faces, out.faces)


# ---- 2. limits -----------------------------------------------------------------------------------------------------------------------
def test_islands_limits():
    mesh = device_mesh("islands")
    empty, vmap = mesh.decimate(64.0, return_map=True)
    assert tuple(empty.vertices.shape) == (0, 3) and tuple(empty.faces.shape) == (0, 3) and tuple(empty.colors.shape) == (0, 3)
    assert bool((vmap == -1).all())
    ident = mesh.decimate(1e-4)
    want = mesh.clean(drop_degenerate=True)
    assert int(ident.num_faces) == 17338 - 48
    assert torch.equal(ident.vertices, want.vertices) and torch.equal(ident.faces, want.faces) and torch.equal(ident.colors, want.colors)
    again = empty.decimate(1.0)                                                        # an empty mesh decimates to an empty mesh
    assert (int(again.num_vertices), int(again.num_faces)) == (0, 0)
    assert tuple(empty.vertex_normals().shape) == (0, 3) and empty.vertex_faces().offsets.tolist() == [0]


# ---- 3. decimate, then continue --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,origin", snp.ISLAND_CASES[:2])
def test_decimate_then_components_and_clean(cell, origin):
    Vo, Fo, Co, _, _ = reference("islands", cell, origin)
    out = device_mesh("islands").decimate(cell, origin)
    cc = out.components()
    labels, triangles, vertices_in, count = mnp.components(Fo, len(Vo))
    same(cc.labels, labels, "labels", torch.int32)
    same(cc.triangles, triangles, "triangles", torch.int32)
    same(cc.vertices_in, vertices_in, "vertices_in", torch.int32)
    assert cc.check() == count
    check_mesh(out.clean(largest=1), *mnp.clean(Vo, Fo, Co, largest=1), "decimate, clean(largest=1)")
    check_mesh(out.clean(largest=1, components=cc).decimate(2 * cell, origin),
               *snp.decimate(*mnp.clean(Vo, Fo, Co, largest=1), 2 * cell, origin)[:3], "decimate, clean, decimate")


# ---- 4. contention: three clusters take every sum ------------------------------------------------------------------------------------
def test_three_blobs_of_3000_vertices():
    from sfgs.mesh import Mesh
    rng = np.random.default_rng(21)
    centres = np.array([[0.5, 0.5, 0.5], [4.5, 0.5, 0.5], [0.5, 4.5, -3.5]])
    V = (centres[:, None, :] + rng.uniform(-0.49, 0.49, (3, 3000, 3))).reshape(-1, 3).astype(np.float32)
    C = rng.uniform(-0.2, 1.2, V.shape).astype(np.float32)
    corners = np.stack([rng.integers(0, 3000, 5000) + 3000 * b for b in range(3)], axis=-1)
    F = np.take_along_axis(corners, np.argsort(rng.random((5000, 3)), axis=1), axis=1).astype(np.int32)   # any corner order
    mesh = Mesh(dev(V), dev(F), dev(C))
    out, (Vo, Fo, Co, vmap, info) = check_decimate(mesh, V, F, C, "blobs", cell=1.0)
    assert (len(Vo), len(Fo), info["clusters"], info["duplicates"]) == (3, 1, 3, 4999) and Fo.tolist() == [(F[0] // 3000).tolist()]
    out, (Vo2, Fo2, _, _, _) = check_decimate(mesh, V, F, C, "blobs", cell=1.0, drop_duplicates=False)
    assert len(Fo2) == 5000 and Fo2.tobytes() == (F // 3000).astype(np.int32).tobytes()              # every face, its own winding
    assert Vo2.tobytes() == Vo.tobytes()
    # the positions are the integer means: within cell 2^-30 + an ulp of the float64 mean, and not one member's bytes
    mean = V.astype(np.float64).reshape(3, 3000, 3).mean(axis=1)
    assert (np.abs(Vo.astype(np.float64) - mean) <= 2.0 ** -30 + np.spacing(np.abs(Vo))).all()


# ---- 5. scale, against a closed form ---------------------------------------------------------------------------------------------------
def test_height_field_across_the_scan_carries():
    from sfgs.mesh import Mesh
    nx, ny = 2050, 2048
    V, F = snp.height_field(nx, ny)
    m, n = len(V), len(F)
    assert m > 1024 * 4096 and n > 1024 * 4096                                        # every plan's scan takes a second round
    mesh = Mesh(torch.from_numpy(V).to(DEV), torch.from_numpy(F).to(DEV))
    out, vmap = mesh.decimate(2.0, origin=(-0.5, -0.5, -0.5), return_map=True)
    cx, cy = nx // 2, ny // 2
    X, Y = np.meshgrid(np.arange(cx, dtype=np.int64), np.arange(cy, dtype=np.int64), indexing="xy")
    wantV = np.stack([2 * X + 0.5, 2 * Y + 0.5, (X + Y) % 3], axis=-1).reshape(-1, 3).astype(np.float32)     # the coarse grid, row-major
    QX, QY = np.meshgrid(np.arange(cx - 1, dtype=np.int64), np.arange(cy - 1, dtype=np.int64), indexing="xy")
    k00 = (QY * cx + QX).reshape(-1)                                                  # the quads at odd-odd corners survive
    wantF = np.stack([np.stack([k00, k00 + 1, k00 + cx], axis=-1), np.stack([k00 + 1, k00 + cx + 1, k00 + cx], axis=-1)], axis=1)
    wantF = wantF.reshape(-1, 3).astype(np.int32)
    x, y = np.arange(m, dtype=np.int64) % nx, np.arange(m, dtype=np.int64) // nx
    assert (int(out.num_vertices), int(out.num_faces)) == (cx * cy, 2 * (cx - 1) * (cy - 1))
    same(out.vertices, wantV, "coarse grid")
    same(out.faces, wantF, "coarse faces", torch.int32)
    same(vmap, ((y // 2) * cx + x // 2).astype(np.int32), "vertex map", torch.int32)
    first = 2 * (np.arange(cx * cy) // cx) * nx + 2 * (np.arange(cx * cy) % cx)       # the clusters' representatives
    assert (first < 1024 * 4096).any() and (first >= 1024 * 4096).any()               # on both sides of the carry
    # the adjacency of the fine grid: counts behind the count scan's carry; the records by what defines them
    adj = mesh.vertex_faces()
    offsets, records = adj
    flat = F.reshape(-1)
    counts = np.bincount(flat, minlength=m)
    want_offsets = np.zeros(m + 1, np.int64)
    want_offsets[1:] = np.cumsum(counts)
    same(offsets, want_offsets.astype(np.int32), "offsets", torch.int32)
    rec = records.cpu().numpy()
    assert rec.shape == (3 * n,) and (flat[rec] == np.repeat(np.arange(m, dtype=np.int32), counts)).all()  # each in its vertex's segment
    inner = np.ones(3 * n, bool)
    inner[want_offsets[:-1][counts > 0]] = False
    assert (np.diff(rec.astype(np.int64), prepend=-1)[inner] > 0).all()                # ascending inside every segment
    assert adj.check() == 0


# ---- 6. adjacency ------------------------------------------------------------------------------------------------------------------------
def test_adjacency_islands_strip_and_fan():
    from sfgs.mesh import Mesh, VertexFaces
    _, _, _, V, F, _ = scene("islands")
    adj = device_mesh("islands").vertex_faces()
    want = snp.vertex_faces(F, len(V))
    assert isinstance(adj, VertexFaces) and isinstance(adj, tuple) and len(adj) == 2 and int(np.diff(want[0]).max()) == 63
    offsets, records = adj
    same(offsets, want[0], "islands offsets", torch.int32)
    same(records, want[1], "islands records", torch.int32)
    assert adj.check() == 0
    Vs, Fs = mnp.strip_mesh()
    adj = Mesh(dev(Vs), dev(Fs)).vertex_faces()
    want = snp.vertex_faces(Fs, len(Vs))
    same(adj.offsets, want[0], "strip offsets", torch.int32)
    same(adj.records, want[1], "strip records", torch.int32)
    Vf, Ff = snp.fan_mesh(5000)
    want = snp.vertex_faces(Ff, len(Vf))
    assert want[0][1] == 5000                                                          # the hub: heapsort
    fan = Mesh(dev(Vf), dev(Ff))
    adj = fan.vertex_faces()
    same(adj.offsets, want[0], "fan offsets", torch.int32)
    same(adj.records, want[1], "fan records", torch.int32)
    assert adj.check() == 0 and adj._state.tolist() == [len(Vf), len(Ff), 0, 0]
    same(fan.vertex_normals(adj), snp.vertex_normals(Vf, Ff), "fan normals")


# ---- 7. normals --------------------------------------------------------------------------------------------------------------------------
def test_normals_islands_decimated_and_wavy():
    _, _, _, V, F, _ = scene("islands")
    mesh = device_mesh("islands")
    want = snp.vertex_normals(V, F)
    adj = mesh.vertex_faces()
    same(mesh.vertex_normals(), want, "islands normals")
    same(mesh.vertex_normals(adjacency=adj), want, "islands normals, adjacency handed in")
    assert adj.check() == 0
    cell, origin = snp.ISLAND_CASES[0]
    Vo, Fo = reference("islands", cell, origin)[:2]
    small = mesh.decimate(cell, origin)
    same(small.vertex_normals(), snp.vertex_normals(Vo, Fo), "decimated normals")
    same(small.vertex_normals(small.vertex_faces()), snp.vertex_normals(Vo, Fo), "decimated normals, adjacency handed in")
    _, _, _, Vw, Fw, _ = scene("wavy")
    assert (len(Vw), len(Fw)) == (76846, 152114)
    wavy = device_mesh("wavy")
    same(wavy.vertex_normals(), snp.vertex_normals(Vw, Fw), "wavy normals")
    with pytest.raises(ValueError):
        mesh.vertex_normals(adjacency=small.vertex_faces())                           # made for another mesh


def test_normals_of_a_repeated_index_and_an_isolated_vertex():
    from sfgs.mesh import Mesh
    V = np.random.default_rng(2).random((6, 3), dtype=np.float32)
    F = np.array([[0, 0, 1], [1, 2, 4], [2, 5, 4]], np.int32)
    mesh = Mesh(dev(V), dev(F))
    adj = mesh.vertex_faces()
    assert adj.offsets.tolist() == [0, 2, 4, 6, 6, 8, 9] and adj.records.tolist() == [0, 1, 2, 3, 4, 6, 5, 8, 7]   # 0 twice in face 0
    got = mesh.vertex_normals(adj)
    same(got, snp.vertex_normals(V, F), "tiny normals")
    n = got.cpu().numpy()
    assert n[3].tobytes() == bytes(12) and n[0].tobytes() == bytes(12)                # isolated; only the (v, v, w) face: +0.0 each
    assert n[1].tobytes() == Mesh(dev(V), dev(F[1:])).vertex_normals().cpu().numpy()[1].tobytes() and np.abs(n[1]).sum() > 0


# ---- 8. bad input ------------------------------------------------------------------------------------------------------------------------
def test_bad_vertices_and_indices_surface_and_nothing_is_indexed():
    from sfgs.mesh import Mesh
    V, F = mnp.strip_mesh(3000)
    for bad_value, cell in ((np.nan, 1.0), (np.inf, 1.0), (1e30, 1.0), (3e9, 1.0), (5.0, 1e-9)):
        Vb = V.copy()
        Vb[F[1234, 1], 2] = bad_value
        mesh = Mesh(dev(Vb), dev(F))
        out, vmap = mesh.decimate(cell, return_map=True)
        for use in (lambda: out.vertices, lambda: out.faces, lambda: out.components(), lambda: out.vertex_normals()):
            with pytest.raises(ValueError, match="vertex"):
                use()
        # the kernels themselves leave the vertex out, drop its faces and say so: the restatement's bytes
        Vo, Fo, _, want_map, info = snp.decimate(Vb, F, None, cell)
        kept_v, kept_f, status, _ = out._state.tolist()
        assert (kept_v, kept_f, status) == (len(Vo), len(Fo), 16) and info["bad"] >= 1 and info["status"] == 16
        same(out.vertex_buffer[:kept_v], Vo, "vertices without the bad vertex")
        same(out.face_buffer[:kept_f], Fo, "faces without the bad vertex", torch.int32)
        same(vmap, want_map, "map without the bad vertex", torch.int32)
        assert want_map[F[1234, 1]] == -1
    for bad in (len(V), -1, 2 ** 31 - 1):
        Fb = F.copy()
        Fb[77, 2] = bad
        mesh = Mesh(dev(V), dev(Fb))
        for use in (lambda: mesh.decimate(1.0), lambda: mesh.vertex_faces(), lambda: mesh.vertex_normals()):
            with pytest.raises(ValueError, match="face index"):
                use()
    good = Mesh(dev(V), dev(F))                                                       # a following call on a good mesh still works
    check_decimate(good, V, F, None, "strip after the bad ones", cell=3.0)
    same(good.vertex_normals(), snp.vertex_normals(V, F), "strip normals")


def test_the_kernels_skip_a_bad_face_index():
    from sfgs import _call
    from sfgs import _lib as L
    V, F = mnp.strip_mesh(3000)
    Fb = F.copy()
    Fb[77, 2] = len(V)
    Fb[78, 0] = -5
    m, n = len(V), len(Fb)
    lib, device = L.load(), torch.device(DEV)
    Vd, Fd = dev(V), dev(Fb)
    Vo_, Fo_ = torch.full((m + 8, 3), -7.0, device=DEV), torch.full((n + 8, 3), -7, dtype=torch.int32, device=DEV)
    vmap, state = torch.full((m + 8,), -7, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    scratch = _call.scratch(lib.sfgs_mesh_decimate_scratch_bytes(m, n, 0), device, refused_if_zero=True)
    L.check(lib.sfgs_mesh_decimate(L.ptr(Vd), None, L.ptr(Fd), m, n, 3.0, 0.0, 0.0, 0.0, 1, L.ptr(Vo_), None, L.ptr(Fo_), L.ptr(vmap),
                                   L.ptr(state), L.ptr(scratch), scratch.numel(), _call.stream(device)))
    Vo, Fo, _, want_map, info = snp.decimate(V, Fb, None, 3.0)
    assert info["status"] == 8 and state.tolist() == [len(Vo), len(Fo), 8, 0]
    same(Vo_[:len(Vo)], Vo, "vertices without the bad faces")
    same(Fo_[:len(Fo)], Fo, "faces without the bad faces", torch.int32)
    same(vmap[:m], want_map, "map without the bad faces", torch.int32)
    assert bool((Vo_[m:] == -7).all()) and bool((Fo_[n:] == -7).all()) and bool((vmap[m:] == -7).all())   # nothing beyond the sizes
    offsets, records = torch.full((m + 9,), -7, dtype=torch.int32, device=DEV), torch.full((3 * n + 8,), -7, dtype=torch.int32, device=DEV)
    scratch = _call.scratch(lib.sfgs_mesh_vertex_faces_scratch_bytes(m), device, refused_if_zero=True)
    L.check(lib.sfgs_mesh_vertex_faces(L.ptr(Fd), n, m, L.ptr(offsets), L.ptr(records), L.ptr(state), L.ptr(scratch), scratch.numel(),
                                       _call.stream(device)))
    flat = Fb.reshape(-1)
    ok = np.nonzero((flat >= 0) & (flat < m))[0]
    want_records = ok[np.argsort(flat[ok], kind="stable")].astype(np.int32)            # the two bad corners are left out
    want_offsets = np.concatenate([[0], np.cumsum(np.bincount(flat[ok], minlength=m))]).astype(np.int32)
    assert state.tolist() == [m, n, 8, 0]
    same(offsets[:m + 1], want_offsets, "offsets without the bad corners", torch.int32)
    same(records[:3 * n - 2], want_records, "records without the bad corners", torch.int32)
    assert bool((offsets[m + 1:] == -7).all()) and bool((records[3 * n - 2:] == -7).all())


# ---- 9. determinism and plumbing -----------------------------------------------------------------------------------------------------
def run_all(mesh):
    cell, origin = snp.ISLAND_CASES[1]
    out, vmap = mesh.decimate(cell, origin, return_map=True)
    adj = mesh.vertex_faces()
    normals = mesh.vertex_normals(adj)
    return out, vmap, adj, normals


def test_two_runs_give_the_same_bytes():
    mesh = device_mesh("islands")
    runs = []
    for _ in range(2):
        out, vmap, adj, normals = run_all(mesh)
        runs.append([t.cpu().numpy().tobytes() for t in (out.vertices, out.faces, out.colors, out._state[:3], vmap, adj.offsets, adj.records,
                                                         adj._state, normals)])
    assert runs[0] == runs[1]


def test_non_default_stream():
    _, _, _, V, F, C = scene("islands")
    mesh = device_mesh("islands")
    mesh.vertices                                                                      # the one host read, before the side stream
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(DEV) == side and side.cuda_stream != 0
        out, vmap, adj, normals = run_all(mesh)
    side.synchronize()
    cell, origin = snp.ISLAND_CASES[1]
    Vo, Fo, Co, want_map, _ = reference("islands", cell, origin)
    check_mesh(out, Vo, Fo, Co, "side stream")
    same(vmap, want_map, "vertex map on a side stream", torch.int32)
    want = snp.vertex_faces(F, len(V))
    same(adj.offsets, want[0], "offsets on a side stream", torch.int32)
    same(adj.records, want[1], "records on a side stream", torch.int32)
    same(normals, snp.vertex_normals(V, F), "normals on a side stream")


# ---- 10. PLY -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", (None, (500000.25, 4100000.5, -3.0)))
@pytest.mark.parametrize("colours", (True, False))
def test_save_ply_with_normals(tmp_path, origin, colours):
    from sfgs.mesh import Mesh
    cell, where = snp.ISLAND_CASES[0]
    Vo, Fo, Co = reference("islands", cell, where)[:3]
    small = device_mesh("islands").decimate(cell, where)
    if not colours:
        small = Mesh._made(small.vertex_buffer, small.face_buffer, None, small._state, "decimate")
    normals = small.vertex_normals()
    path, old = str(tmp_path / "normals.ply"), str(tmp_path / "plain.ply")
    small.save_ply(path, origin=origin, normals=normals)
    xyz, got, rgb, faces, names = snp.read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz"] + (["red", "green", "blue"] if colours else [])
    assert got.tobytes() == snp.vertex_normals(Vo, Fo).tobytes() and faces.tobytes() == Fo.tobytes()
    assert xyz.tobytes() == (Vo if origin is None else Vo.astype(np.float64) + np.array(origin)).tobytes()
    assert (rgb is None) == (not colours) and (rgb is None or rgb.tobytes() == mnp.ply_vertex_colors(Co).tobytes())
    small.save_ply(old, origin=origin)                                                 # without normals: today's bytes
    xyz2, rgb2, faces2 = mnp.read_ply(old)
    assert xyz2.tobytes() == xyz.tobytes() and faces2.tobytes() == Fo.tobytes() and (rgb2 is None) == (not colours)
    small.save_ply(path, origin=origin, normals=None)
    assert open(old, "rb").read() == open(path, "rb").read()
    for bad in (normals.cpu(), normals[:-1], normals.double()):
        with pytest.raises(ValueError):
            small.save_ply(path, normals=bad)
