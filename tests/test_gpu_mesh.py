"""GPU tests of sfgs.mesh (csrc/mesh.hip): soup -> welded indexed mesh -> component labels and counts -> cleaned mesh. The
reference is the numpy restatement tests/mesh_np.py (held to the committed host weld, to a plain breadth-first search and to
the host build of the product's header by tests/test_mesh_host.py). Nothing here reads the reference tree.

Bounds. Every comparison is assert-equal on the BYTES: the results are integers and copied rows, so there is nothing to tolerate
and no row or count is left out.

Chunk boundaries of the implementation, and which scene crosses them:
  * every mesh kernel runs workgroups of 256 threads, four waves: all scenes but n = 1 span many workgroups, and their sizes
    (17 338, 152 114, 5 000, 20 000, 200 000 faces; 8 704, 76 846 vertices) are no multiples of 256 or 64;
  * the per-wave / per-workgroup count sums take one path when a wave's lanes share a label (wavy, the strip, the all-equal
    soup: ONE root takes every count) and another when they do not (islands at the seams, the distinct soup: 64 labels a wave);
  * the flag scan (the row compaction's plan) ranks 4 096 rows per workgroup -- crossed by everything from islands up -- and scans
    1 024 workgroups per round with a carry, i.e. 4 194 304 rows. The wavy soup has 456 342 rows and stays below that, so the
    carry is taken by a synthetic soup of 1 420 000 triangles (4 260 000 rows) over 300 000 random vertices, a sixth of
    which first appear in the last 20 000 triangles, behind the carry."""
import functools

import numpy as np
import pytest
import torch

import mesh_np as mnp
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
    """-> (volume case or None, soup, soup colours or None, V, F, C) through the restatement, once"""
    case = {"islands": mnp.islands_volume, "wavy": lambda: tnp.wavy_volume((72, 64, 64), colors=True)}[name]()
    verts, cols = tnp.extract(case[0], case[1], case[3], case[4], case[2])
    return (case,) + frozen(verts, cols, *mnp.weld(verts, cols))


@functools.lru_cache(maxsize=None)
def reference_components(name):
    _, _, _, V, F, _ = scene(name)
    return frozen(*mnp.components(F, len(V))[:3]) + (mnp.components(F, len(V))[3],)


def soup_of(case, capacity):
    from sfgs.tsdf import TsdfVolume
    tsdf, weight, rgb, origin, voxel = case
    nz, ny, nx = tsdf.shape
    v = TsdfVolume(origin, (nx, ny, nz), voxel, trunc=1.0, colors=rgb is not None, device=DEV)
    v.load(dev(tsdf), dev(weight), None if rgb is None else dev(rgb))
    return v.extract(capacity)


def check_mesh(mesh, V, F, C, what):
    for s in (mesh.num_vertices, mesh.num_faces):
        assert s.device == torch.device(DEV) and s.dtype == torch.int64 and s.dim() == 0
    assert (int(mesh.num_vertices), int(mesh.num_faces)) == (len(V), len(F)), what
    same(mesh.vertices, V, f"vertices, {what}")
    same(mesh.faces, F, f"faces, {what}", torch.int32)
    if C is None:
        assert mesh.colors is None
    else:
        same(mesh.colors, C, f"colours, {what}")


def check_components(cc, want, what):
    labels, triangles, vertices_in, count = want
    same(cc.labels, labels, f"labels, {what}", torch.int32)
    same(cc.triangles, triangles, f"triangles, {what}", torch.int32)
    same(cc.vertices_in, vertices_in, f"vertices_in, {what}", torch.int32)
    assert cc.count.device == torch.device(DEV) and cc.count.dtype == torch.int64 and cc.count.dim() == 0
    assert int(cc.count) == count == cc.check(), what


def check_clean(mesh, V, F, C, what, **kw):
    Vo, Fo, Co = mnp.clean(V, F, C, **kw)
    out = mesh.clean(**kw)
    check_mesh(out, Vo, Fo, Co, f"clean {kw}, {what}")
    assert out.vertex_buffer.shape[0] == len(V) and out.face_buffer.shape[0] == len(F)           # allocated at the input's sizes
    return out, (Vo, Fo, Co)


# ---- 1. islands: TsdfVolume.load -> extract -> mesh --------------------------------------------------------------------------------
def test_islands_weld_and_components():
    case, verts, cols, V, F, C = scene("islands")
    want = reference_components("islands")
    roots = np.nonzero(want[0] == np.arange(len(V)))[0]
    assert want[3] == 8 and sorted(want[1][roots].tolist())[:2] == [24, 24]          # guards on the fixture: 8 components, the tie
    assert (len(verts), len(V), int(mnp.degenerate(F).sum())) == (17338, 8704, 48)
    soup = soup_of(case, len(verts) + 50)                                             # spare capacity: rows the weld must not read
    mesh = soup.mesh()
    check_mesh(mesh, V, F, C, "islands")
    assert mesh.vertex_buffer.shape[0] == 3 * len(verts)
    check_components(mesh.components(), want, "islands")
    # without colours: the same vertices and faces
    from sfgs.mesh import weld
    check_mesh(weld(soup.vertices), V, F, None, "islands, no colours")
    # relation to the host weld: byte-sorted V is TriangleSoup.weld()'s V
    hostV, _ = soup.weld()
    keys = mesh.vertices.cpu().numpy().view(np.dtype((np.void, 12))).reshape(-1)
    assert np.sort(keys).tobytes() == np.ascontiguousarray(hostV).tobytes()


CLEAN_CASES = ({"min_triangles": 25}, {"largest": 7}, {"largest": 1}, {"largest": 100}, {"min_triangles": 100, "largest": 7},
               {"min_triangles": 3000, "largest": 2}, {"drop_degenerate": True}, {"drop_degenerate": True, "min_triangles": 25},
               {"drop_degenerate": True, "largest": 7}, {"drop_degenerate": True, "min_triangles": 30, "largest": 3}, {"largest": 0},
               {"min_triangles": 0})


@functools.lru_cache(maxsize=None)
def islands_mesh():
    case, verts, cols, V, F, C = scene("islands")
    return soup_of(case, len(verts)).mesh()


@pytest.mark.parametrize("kw", CLEAN_CASES, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_islands_clean(kw):
    _, _, _, V, F, C = scene("islands")
    mesh = islands_mesh()
    out, (Vo, Fo, Co) = check_clean(mesh, V, F, C, "islands", **kw)
    if kw == {"min_triangles": 25}:
        assert len(Fo) == len(F) - 48                                                 # the two components of 24 triangles
    if kw == {"largest": 7}:                                                          # label 94 stays, 8690 goes, by the tie-break
        assert V[94].tobytes() in {bytes(r) for r in Vo.view(np.dtype((np.void, 12))).reshape(-1)}
        assert V[8690].tobytes() not in {bytes(r) for r in Vo.view(np.dtype((np.void, 12))).reshape(-1)}
    if kw in ({"largest": 100}, {"min_triangles": 0}):                                # keeps everything: the input's bytes
        assert torch.equal(out.vertices, mesh.vertices) and torch.equal(out.faces, mesh.faces) and torch.equal(out.colors, mesh.colors)
    if kw == {"largest": 0}:
        assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3)
    # a clean with the components handed in is the same clean; a cleaned mesh cleans and labels again
    again = mesh.clean(components=mesh.components(), **kw)
    check_mesh(again, Vo, Fo, Co, f"clean with components, {kw}")
    check_components(out.components(), mnp.components(Fo, len(Vo)), f"components of the cleaned mesh, {kw}")


# ---- 2. wavy: one component takes every count ----------------------------------------------------------------------------------------
def test_wavy_one_component():
    case, verts, cols, V, F, C = scene("wavy")
    assert (len(verts), 3 * len(verts), len(V)) == (152114, 456342, 76846)
    want = reference_components("wavy")
    assert want[3] == 1 and want[1][0] == len(F) and want[2][0] == len(V)
    mesh = soup_of(case, len(verts)).mesh()
    check_mesh(mesh, V, F, C, "wavy")
    check_components(mesh.components(), want, "wavy")
    check_clean(mesh, V, F, C, "wavy", min_triangles=64, largest=1)
    check_clean(mesh, V, F, C, "wavy", drop_degenerate=True)
    check_clean(mesh, V, F, C, "wavy", min_triangles=len(F) + 1)


# ---- 3. synthetic soups through sfgs.mesh.weld -------------------------------------------------------------------------------------
def weld_and_check(soup, cols, what, full=True):
    from sfgs.mesh import weld
    V, F, C = mnp.weld(soup, cols)
    mesh = weld(dev(soup), None if cols is None else dev(cols))
    check_mesh(mesh, V, F, C, what)
    if full:
        check_components(mesh.components(), mnp.components(F, len(V)), what)
    return mesh, (V, F, C)


def test_one_triangle_and_no_triangle():
    from sfgs.mesh import weld
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    mesh, (V, F, C) = weld_and_check(tri, tri * 0.5, "n = 1")
    assert F.tolist() == [[0, 1, 2]]
    check_clean(mesh, V, F, C, "n = 1", largest=1, drop_degenerate=True)
    empty = weld(torch.zeros((0, 3, 3), device=DEV))
    assert (int(empty.num_vertices), int(empty.num_faces)) == (0, 0) and tuple(empty.vertices.shape) == (0, 3)
    assert int(empty.components().count) == 0 and tuple(empty.clean(largest=1).faces.shape) == (0, 3)
    # num_triangles: only the first rows are welded, the rest is never read
    padded = np.concatenate([tri, np.full((3, 3, 3), np.nan, np.float32)])
    check_mesh(weld(dev(padded), num_triangles=1), V, F, None, "num_triangles = 1")


def test_all_vertices_equal():
    soup = np.full((5000, 3, 3), 0.375, np.float32)
    mesh, (V, F, C) = weld_and_check(soup, None, "15 000 equal vertices")
    assert len(V) == 1 and not F.any()
    cc = mesh.components()
    assert int(cc.count) == 1 and cc.triangles.tolist() == [5000] and cc.vertices_in.tolist() == [1]
    out, _ = check_clean(mesh, V, F, C, "15 000 equal vertices", drop_degenerate=True)
    assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3)
    check_clean(mesh, V, F, C, "15 000 equal vertices", min_triangles=5000, largest=1)


def test_all_vertices_distinct():
    rng = np.random.default_rng(11)
    soup = rng.random((20000, 3, 3), dtype=np.float32)
    assert len(np.unique(soup.reshape(-1, 3), axis=0)) == 60000
    mesh, (V, F, C) = weld_and_check(soup, rng.random((20000, 3, 3), dtype=np.float32), "60 000 distinct vertices")
    assert V.tobytes() == soup.tobytes() and F.reshape(-1).tolist() == list(range(60000))
    assert int(mesh.components().count) == 20000
    check_clean(mesh, V, F, C, "60 000 distinct vertices", largest=777)             # 20 000 ties: the 777 smallest labels
    check_clean(mesh, V, F, C, "60 000 distinct vertices", min_triangles=2)


def test_signed_zeros_and_nan_payloads():
    soup = mnp.special_soup()
    mesh, (V, F, C) = weld_and_check(soup, np.arange(54, dtype=np.float32).reshape(6, 3, 3), "zeros and NaNs")
    assert len(V) == 11 and F.tolist() == [[0, 1, 2], [3, 1, 4], [5, 6, 5], [7, 5, 0], [8, 9, 3], [6, 2, 10]]
    check_clean(mesh, V, F, C, "zeros and NaNs", drop_degenerate=True)


def test_scan_carry_on_a_soup_of_4_2_million_rows():
    rng = np.random.default_rng(7)
    V0 = rng.random((300_000, 3), dtype=np.float32)
    index = rng.integers(0, 250_000, (1_420_000, 3))
    index[1_400_000:] = rng.integers(0, len(V0), (20_000, 3))                         # vertices that first appear behind row 4 200 000
    soup = V0[index]
    assert soup.shape[0] * 3 > 1024 * 4096                                            # the plan's scan takes a second round
    mesh, (V, F, C) = weld_and_check(soup, None, "4.2 M rows", full=False)
    first = np.full(len(V), 3 * len(soup))
    np.minimum.at(first, F.reshape(-1), np.arange(3 * len(soup)))
    assert (first < 1024 * 4096).any() and (first >= 1024 * 4096).any()               # representatives on both sides of the carry


def test_strip_of_200000_faces_shuffled():
    from sfgs.mesh import Mesh
    V, F = mnp.strip_mesh()
    frozen(V, F)
    mesh = Mesh(dev(V), dev(F))
    check_mesh(mesh, V, F, None, "strip")
    want = mnp.components(F, len(V))
    assert want[3] == 1 and want[1][0] == 200000 and want[2][0] == 200002
    check_components(mesh.components(), want, "strip")
    check_clean(mesh, V, F, None, "strip", largest=1)


def test_isolated_vertex_and_caller_colours():
    from sfgs.mesh import Mesh
    F = np.array([[0, 1, 2], [2, 1, 4], [6, 7, 6], [7, 7, 7]], np.int32)
    V = np.arange(27, dtype=np.float32).reshape(9, 3)
    C = V[::-1] / 27
    mesh = Mesh(dev(V), dev(F), dev(C))
    want = mnp.components(F, 9)
    assert want[0].tolist() == [0, 0, 0, 3, 0, 5, 6, 6, 8] and want[3] == 5 and want[1].tolist() == [2, 0, 0, 0, 0, 0, 2, 0, 0]
    check_components(mesh.components(), want, "isolated vertices")
    out, (Vo, Fo, Co) = check_clean(mesh, V, F, C, "isolated vertices", largest=100)      # unreferenced vertices go
    assert len(Vo) == 6 and Fo.tolist() == [[0, 1, 2], [2, 1, 3], [4, 5, 4], [5, 5, 5]]
    check_clean(mesh, V, F, C, "isolated vertices", largest=1)                           # 2 against 2: label 0 stays
    check_clean(mesh, V, F, C, "isolated vertices", drop_degenerate=True, min_triangles=2)


def test_out_of_range_index_surfaces_and_nothing_is_indexed():
    from sfgs import _call
    from sfgs import _lib as L
    from sfgs.mesh import Mesh
    V, F = mnp.strip_mesh(3000)
    for bad in (len(V), -1, 2 ** 31 - 1):
        Fb = F.copy()
        Fb[1234, 1] = bad
        mesh = Mesh(dev(V), dev(Fb))
        for use in (lambda: mesh.vertices, lambda: mesh.components(), lambda: mesh.clean(largest=1)):
            with pytest.raises(ValueError, match="face index"):
                use()
    # the kernels themselves skip the face and say so: the labels are those of the mesh without it
    lib = L.load()
    m, n = len(V), len(Fb)
    faces = dev(Fb)
    labels, triangles, vertices_in = (torch.full((m + 64,), -7, dtype=torch.int32, device=DEV) for _ in range(3))
    state = torch.zeros(4, dtype=torch.int64, device=DEV)
    scratch = _call.scratch(lib.sfgs_mesh_components_scratch_bytes(m), torch.device(DEV), refused_if_zero=True)
    L.check(lib.sfgs_mesh_components(L.ptr(faces), n, m, L.ptr(labels), L.ptr(triangles), L.ptr(vertices_in), L.ptr(state), L.ptr(scratch),
                                     scratch.numel(), _call.stream(torch.device(DEV))))
    want = mnp.components(np.delete(Fb, 1234, axis=0), m)
    assert state.tolist() == [want[3], 0, 8, 0]
    same(labels[:m], want[0], "labels without the bad face", torch.int32)
    same(triangles[:m], want[1], "triangles without the bad face", torch.int32)
    same(vertices_in[:m], want[2], "vertices_in without the bad face", torch.int32)
    assert all(bool((t[m:] == -7).all()) for t in (labels, triangles, vertices_in))


# ---- 4. determinism and plumbing ---------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes():
    _, verts, cols, V, F, C = scene("islands")
    from sfgs.mesh import weld
    s, c = dev(verts), dev(cols)
    runs = []
    for _ in range(2):
        mesh = weld(s, c)
        cc = mesh.components()
        out = mesh.clean(min_triangles=25, largest=5, drop_degenerate=True, components=cc)
        runs.append([t.cpu().numpy().tobytes() for t in (mesh.vertices, mesh.faces, mesh.colors, cc.labels, cc.triangles, cc.vertices_in,
                                                         cc._state[:3], out.vertices, out.faces, out.colors)])
    assert runs[0] == runs[1]


def test_non_default_stream():
    case, verts, cols, V, F, C = scene("islands")
    s, c = dev(verts), dev(cols)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(DEV) == side and side.cuda_stream != 0
        from sfgs.mesh import weld
        mesh = weld(s, c)
        cc = mesh.components()
        out = mesh.clean(largest=3)
    side.synchronize()
    check_mesh(mesh, V, F, C, "side stream")
    check_components(cc, reference_components("islands"), "side stream")
    check_mesh(out, *mnp.clean(V, F, C, largest=3), "clean on a side stream")


def test_a_soup_beyond_its_capacity_raises():
    case, verts, _, _, _, _ = scene("islands")
    soup = soup_of(case, 1000)
    with pytest.raises(ValueError, match=f"capacity of {len(verts)} would have sufficed"):
        soup.mesh()


@pytest.mark.parametrize("origin", (None, (500000.25, 4100000.5, -3.0)))
def test_save_ply_read_back(tmp_path, origin):
    _, _, _, V, F, C = scene("islands")
    mesh = islands_mesh()
    path = str(tmp_path / "islands.ply")
    mesh.save_ply(path, origin=origin)
    xyz, rgb, faces = mnp.read_ply(path)
    if origin is None:
        assert xyz.dtype == np.float32 and xyz.tobytes() == V.tobytes()
    else:
        assert xyz.dtype == np.float64 and xyz.tobytes() == (V.astype(np.float64) + np.array(origin)).tobytes()
    assert faces.tobytes() == F.tobytes() and rgb.tobytes() == mnp.ply_vertex_colors(C).tobytes()
    mesh.clean(largest=1).save_ply(path)
    xyz, rgb, faces = mnp.read_ply(path)
    Vo, Fo, Co = mnp.clean(V, F, C, largest=1)
    assert xyz.tobytes() == Vo.tobytes() and faces.tobytes() == Fo.tobytes() and rgb.tobytes() == mnp.ply_vertex_colors(Co).tobytes()


def test_wrong_arguments_raise_value_error():
    from sfgs.mesh import Mesh, weld
    soup = torch.zeros((4, 3, 3), device=DEV)
    mesh = weld(soup)
    other = Mesh(torch.zeros((5, 3), device=DEV), torch.zeros((2, 3), dtype=torch.int32, device=DEV))
    for call in (lambda: weld(soup.cpu()), lambda: weld(soup.double()), lambda: weld(soup[:, :, :2]), lambda: weld(soup, colors=soup[:2]),
                 lambda: weld(soup, colors=soup.cpu()), lambda: weld(soup.transpose(1, 2)), lambda: weld(soup, num_triangles=5),
                 lambda: Mesh(soup[0], torch.zeros((1, 3), dtype=torch.int64, device=DEV)),
                 lambda: Mesh(soup[0], torch.zeros((1, 3), dtype=torch.int32)),
                 lambda: Mesh(soup[0], torch.zeros((1, 3), dtype=torch.int32, device=DEV), colors=soup[1].cpu()),
                 lambda: mesh.clean(min_triangles=-1), lambda: mesh.clean(largest=2.5), lambda: mesh.clean(drop_degenerate=None),
                 lambda: mesh.clean(components=other.components()), lambda: mesh.save_ply("/tmp/never.ply", origin=(1.0,))):
        with pytest.raises(ValueError):
            call()
