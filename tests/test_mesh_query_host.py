"""Host tests of the mesh queries (Mesh.face_grid, Mesh.closest, Mesh.sample): the host build of csrc/mesh_query_math.h against the
numpy restatement tests/mesh_query_np.py byte for byte, the closest point against independent spellings, the ring search against
brute force (the proof of the stop rule, run on the CPU), the sampler's statistics, and the refusals of the library. No GPU: every
refusal is made before any GPU work.

The tolerances here are derived, not measured.
  LATTICE. d2 is the squared distance to the closest point of the closed triangle, so it is at most the squared distance to ANY
  point of it, up to the float64 rounding of both sides: a relative 16 x 2^-52 of the larger (about ten rounded operations each)
  plus an absolute (64 x 2^-52 s)^2 with s = the largest |coordinate| involved, for the cancellation in p - q.
  SPHERE. The mesh of tsdf_np.sphere_volume interpolates the zero crossing of a sampled distance field along the edges of its
  tetrahedra: a vertex lies on a voxel edge where the linearly interpolated field is zero. Along an edge of length at most
  sqrt(3) voxel the field |x - c| - R deviates from its linear interpolant by at most L^2 / (8 R) (second derivative at most
  1 / R near the surface), and a face's interior lies inside the sphere of its vertices by at most the sagitta L^2 / (8 R) of a
  chord of length L again. |sqrt(d2) - | |p - c| - R| | is held to twice that with L = sqrt(3) voxel, plus the float32 rounding of
  the stored field and vertices (2^-20 of the coordinates' magnitude).
  SAMPLE ON ITS FACE. A sample is float32(a + u1 (b - a) + u2 (c - a)) of a point of the triangle computed in float64: each
  coordinate moves by at most half an ulp of float32, 2^-24 of its magnitude, hence d2 <= 3 (max |coordinate| 2^-24)^2, times 1.01
  for the float64 roundings before the last one.
  COUNT. The total is a sum of n independent roundings of variance at most 1/4: its standard deviation is at most sqrt(n) / 2,
  and 2 sqrt(n) is four of them."""
import ctypes as C

import numpy as np
import pytest

import mesh_query_hostcheck as hc
import mesh_query_np as mq
import mesh_render_np as mrn
import tsdf_np as tnp
from sfgs import _lib as L

E_ARG = -1
SCENES = list(mq.scenes())


def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)


def grid_np(name, **kw):
    V, F, _, g, _ = mq.scenes()[name]
    return mq.face_grid(V, F, g["cell"], g["origin"], g["dims"], **kw)


# ---- the header against numpy ------------------------------------------------------------------------------------------------------
def test_the_cell_function_is_the_restatements_and_monotone():
    rng = np.random.default_rng(0)
    xs = np.sort(np.concatenate([rng.normal(0, 50, 500), np.float32(rng.normal(0, 1e-3, 100)).astype(np.float64),
                                 [0.0, -0.0, 1.5, 3.0, -4.5, 1e30, -1e30, np.inf, -np.inf]]))
    for origin, cell in ((0.0, 1.5), (-3.25, 0.1), (7.0, 1e-3), (1e6, 3.0)):
        got = np.array([hc.cell_of(x, origin, cell) for x in xs])
        same_bytes(got, mq.cell_of(xs, origin, cell), f"cell, origin {origin}, cell {cell}")
        assert (np.diff(got) >= 0).all() or np.isnan(np.diff(got)).any()       # inf - inf at the two ends only
        assert (np.diff(got[1:-1]) >= 0).all()
    assert np.isnan(hc.cell_of(np.nan, 0.0, 1.0))


@pytest.mark.parametrize("name", SCENES)
def test_the_headers_closest_point_equals_numpys(name):
    V, F, _, _, P = mq.scenes()[name]
    Vd, Fi = V.astype(np.float64), np.asarray(F).reshape(-1, 3)
    ok = ((Fi >= 0) & (Fi < len(V))).all(axis=1)
    assert ok.all()
    for p in P[:24]:
        d2, q = hc.closest_faces(p, V, F)
        rd2, rq = mq.tri_closest(p.astype(np.float64), Vd[Fi[:, 0]], Vd[Fi[:, 1]], Vd[Fi[:, 2]])
        # a NaN never wins and is written nowhere: its sign and payload are not part of the contract
        assert (np.isnan(d2) == np.isnan(rd2)).all() and (np.isnan(q) == np.isnan(rq)).all()
        same_bytes(np.nan_to_num(d2, nan=-1.0), np.nan_to_num(rd2, nan=-1.0), f"d2, {name}")
        same_bytes(np.nan_to_num(q, nan=-1.0), np.nan_to_num(rq, nan=-1.0), f"q, {name}")


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("max_cells", (0, mq.MAX_CELLS_DEFAULT, 1 << 30))
def test_the_headers_grid_equals_numpys(name, max_cells):
    V, F, _, g, _ = mq.scenes()[name]
    ref = grid_np(name, max_cells=max_cells)
    got = hc.face_grid(V, F, ref.cell, ref.origin, ref.dims, max_cells=max_cells)
    same_bytes(got.cell_start, ref.cell_start, f"cell_start, {name}")
    same_bytes(got.pairs, ref.pairs, f"pairs, {name}")
    same_bytes(got.large, ref.large, f"large, {name}")
    assert (got.skipped, got.status, got.need) == (ref.skipped, 0, len(ref.pairs))
    if max_cells == 0:
        assert len(ref.pairs) == 0 and len(ref.large) == len(F) - ref.skipped
    if max_cells == 1 << 30:
        assert len(ref.large) == 0


def test_the_shared_scenes_are_the_cases_they_are_meant_to_be():
    g = grid_np("fan")
    assert np.diff(g.cell_start).max() == 5000                                  # thousands of faces in one cell
    g = grid_np("quad in a fine grid")
    assert len(g.large) == 2 and len(g.pairs) == 0                              # both faces on the large list at the default
    g = grid_np("special soup")
    assert g.skipped == 3                                                        # the faces with a NaN vertex
    V, F, _ = mrn.islands_mesh()
    assert (len(F), len(V)) == (17338, 8704)
    g = grid_np("islands, a given grid smaller than the mesh")
    ok, lo, hi = mq.face_ranges(V, F, g.cell, g.origin, g.dims)
    raw = mq.cell_of(V.astype(np.float64)[:, 0], g.origin[0], g.cell)
    assert raw.min() < 0 and raw.max() > g.dims[0] - 1                           # clamped ranges on both sides
    assert hc.face_grid(V, F, g.cell, g.origin, g.dims, capacity=len(g.pairs) - 1).status == mq.ST_CAPACITY


def test_area_and_mixer_equal_numpys():
    V, F, _ = mrn.islands_mesh()
    A, _ = mq.face_areas(V, F)
    same_bytes(np.array([hc.area(V[F[t]]) for t in range(0, len(F), 97)]), A[::97], "area")
    Vs, Fs = mrn.special_mesh()
    As, _ = mq.face_areas(Vs, Fs)
    same_bytes(np.array([hc.area(Vs[Fs[t]]) for t in range(len(Fs))]), As, "area, special")
    rng = np.random.default_rng(1)
    words = rng.integers(0, 1 << 32, (200, 3), dtype=np.uint64).astype(np.uint32)
    words[:4] = [[0, 0, 0], [0xffffffff] * 3, [0, 5, 0xffffffff], [7, 0xffffffff, 1]]
    got = np.array([hc.mix3(*w) for w in words], np.uint32)
    same_bytes(got, mq.mix3(words[:, 0], words[:, 1], words[:, 2]), "mix3")
    assert len(set(got.tolist())) == len(got)


# ---- the closest point against independent spellings ---------------------------------------------------------------------------------
def test_d2_is_below_every_lattice_point_and_above_the_plane_distance():
    V, F, _ = mrn.sphere_mesh()
    Vd = V.astype(np.float64)
    a, b, c = (Vd[F[:, j]] for j in range(3))
    n = np.cross(b - a, c - a)
    nn = np.linalg.norm(n, axis=1)
    assert (nn > 0).all()
    k = 12
    w = np.array([(i / k, j / k) for i in range(k + 1) for j in range(k + 1 - i)])
    lattice = a[:, None] + w[None, :, :1] * (b - a)[:, None] + w[None, :, 1:] * (c - a)[:, None]       # [n, L, 3]
    P = mq.scenes()["sphere"][4]
    P = P[np.isfinite(P).all(axis=1) & (np.abs(P).max(axis=1) < 1e6)][:40]
    for p in P:
        d2, _ = mq.tri_closest(p, a, b, c)
        s = max(np.abs(p).max(), np.abs(Vd).max())
        slack = 16 * 2.0 ** -52 * np.maximum(d2, 1.0) + (64 * 2.0 ** -52 * s) ** 2
        upper = ((p - lattice) ** 2).sum(axis=2).min(axis=1)
        assert (d2 <= upper + slack + 16 * 2.0 ** -52 * upper).all()
        plane = (((p - a) * n).sum(axis=1) / nn) ** 2
        assert (d2 >= plane - slack - 16 * 2.0 ** -52 * plane).all()


def test_the_distance_to_the_sphere_mesh_is_the_distance_to_the_sphere():
    V, F, _ = mrn.sphere_mesh()
    _, _, _, origin, voxel = tnp.sphere_volume(True)
    centre, R = np.asarray(tnp.SPHERE.centre, np.float64), float(tnp.SPHERE.radius)
    L2 = 3.0 * voxel * voxel
    bound = 2.0 * L2 / (8.0 * R) + 2.0 ** -20 * np.abs(V).max()
    P = mq.scenes()["sphere"][4]
    P = P[np.isfinite(P).all(axis=1) & (np.abs(P).max(axis=1) < 1e6)]
    sq, face, _, _ = mq.closest(V, F, P)
    assert (face >= 0).all()
    err = np.abs(np.sqrt(sq) - np.abs(np.linalg.norm(P - centre, axis=1) - R))
    assert err.max() <= bound, (err.max(), bound)


# ---- the ring search against brute force ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("max_cells", (0, mq.MAX_CELLS_DEFAULT, 1 << 30))
def test_the_ring_search_equals_brute_force(name, max_cells):
    """the host build's search (the kernel's loop) over the host build's table, all queries; numpy's search on a few"""
    V, F, _, _, P = mq.scenes()[name]
    g = grid_np(name, max_cells=max_cells)
    sq, face, point, counts = mq.closest(V, F, P)
    hsq, hface, hpoint, hcounts, rings = hc.search(g, V, F, P)
    same_bytes(hsq, sq, f"sqdist, {name}")
    same_bytes(hface, face, f"face, {name}")
    same_bytes(hpoint, point, f"point, {name}")
    assert hcounts.tolist() == counts[:2].tolist()
    if max_cells == 0:
        assert rings.max(initial=0) == 0
    for i in range(0, len(P), 9):
        a, b, c = mq.ring_search(g, V, F, P[i])
        assert (a, b) == (sq[i], face[i]) or (np.isinf(a) and np.isinf(sq[i]) and b == face[i] == -1)
        same_bytes(c, point[i], f"numpy's ring search, {name}, point {i}")


def test_queries_on_vertices_have_distance_zero_and_ties_go_to_the_smaller_index():
    V, F, _, _, _ = mq.scenes()["stacked faces"]
    g = grid_np("stacked faces")
    P = V[F.reshape(-1)].astype(np.float64)
    sq, face, _, _, _ = hc.search(g, V, F, P)
    assert (sq == 0).all()
    assert (face[:6] == 0).all()                                                # faces 0 and 1 coincide: the smaller index
    inside = (V[F[0]].astype(np.float64).mean(axis=0) + [0.0, 0.0, 0.5])[None]
    assert hc.search(g, V, F, inside)[1][0] == 0 and mq.closest(V, F, inside)[1][0] == 0
    Vi, Fi, _ = mrn.islands_mesh()
    gi = grid_np("islands")
    Pv = Vi[::37].astype(np.float64)
    sq, face, _, _, _ = hc.search(gi, Vi, Fi, Pv)
    assert (sq == 0).all() and (face >= 0).all()
    bsq, bface, _, _ = mq.closest(Vi, Fi, Pv)
    same_bytes(face, bface, "faces at vertices")


@pytest.mark.parametrize("name", ("islands", "islands, a given grid smaller than the mesh", "sphere", "quad in a fine grid", "special soup"))
def test_max_distance_just_below_and_just_above_the_true_distance(name):
    V, F, _, _, P = mq.scenes()[name]
    g = grid_np(name)
    sq, face, _, _ = mq.closest(V, F, P)
    for i in np.flatnonzero((face >= 0) & (sq > 0))[:12]:
        d = np.sqrt(sq[i])
        above = d
        while above * above < sq[i]:
            above = np.nextafter(above, np.inf)
        below = np.nextafter(above, -np.inf)
        while below * below >= sq[i]:
            below = np.nextafter(below, -np.inf)
        for md, want in ((above, face[i]), (below, -1)):
            hsq, hface, _, _, _ = hc.search(g, V, F, P[i:i + 1], max_distance=md)
            bsq, bface, _, _ = mq.closest(V, F, P[i:i + 1], max_distance=md)
            assert hface[0] == bface[0] == want, (name, i, md)
            same_bytes(hsq, bsq, "sqdist with max_distance")
    far = hc.search(g, V, F, P, max_distance=0.4 * g.cell)
    ref = mq.closest(V, F, P, max_distance=0.4 * g.cell)
    same_bytes(far[0], ref[0], "sqdist, small max_distance")
    same_bytes(far[1], ref[1], "face, small max_distance")


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
SEEDS = (0, 1, 12345)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_headers_sampler_equals_numpys(seed):
    for name, density in (("islands", 2.0), ("sphere", 7.5), ("square", 3.0), ("stacked faces", 1.0), ("fan", 40.0)):
        V, F, Cc, _, _ = mq.scenes()[name]
        ref = mq.sample(V, F, Cc, density, seed)
        got = hc.sample(V, F, Cc, density, seed)
        assert got.count == len(ref.points) and got.status == ref.status == 0
        same_bytes(got.points, ref.points, f"points, {name}")
        same_bytes(got.face, ref.face, f"face, {name}")
        if Cc is not None:
            same_bytes(got.colors, ref.colors, f"colors, {name}")


def test_a_face_without_a_finite_area_samples_nothing_and_raises_the_status():
    V, F = mrn.special_mesh()
    ref, got = mq.sample(V, F, None, 3.0, 2), hc.sample(V, F, None, 3.0, 2)
    assert ref.status == got.status == mq.ST_BAD_FACE
    same_bytes(got.points, ref.points, "points, special")
    assert np.isfinite(ref.points).all()
    big = hc.sample(*mrn.square_mesh()[:2], None, 1e6, 0)
    assert big.status == mq.ST_BAD_FACE and big.count == 0                       # 32 x 10^6 samples per face: more than 2^20


@pytest.mark.parametrize("seed", SEEDS)
def test_samples_lie_on_their_faces_and_their_number_follows_the_area(seed):
    for name, density in (("islands", 2.0), ("sphere", 7.5)):
        V, F, _, _, _ = mq.scenes()[name]
        s = mq.sample(V, F, None, density, seed)
        Vd = V.astype(np.float64)
        a, b, c = (Vd[F[s.face, j]] for j in range(3))
        d2 = np.array([mq.tri_closest(p, a[i:i + 1], b[i:i + 1], c[i:i + 1])[0][0] for i, p in enumerate(s.points.astype(np.float64))])
        assert d2.max() <= 1.01 * 3.0 * (np.abs(V).max() * 2.0 ** -24) ** 2
        A, _ = mq.face_areas(V, F)
        assert abs(len(s.points) - A.sum() * density) <= 2.0 * np.sqrt(len(F))
        assert (np.diff(s.face) >= 0).all()
    V, F = mrn.square_mesh()                                                     # two triangles of 32 each
    s = mq.sample(V, F, None, 10.0, seed)
    assert np.bincount(s.face, minlength=2).tolist() == [320, 320]


# ---- refusals of the library (before any GPU work) -----------------------------------------------------------------------------------
def _grid_args(**kw):
    fake = 0x1000
    a = L.SfgsMeshGrid(C.sizeof(L.SfgsMeshGrid), 4, 4, 4, (C.c_double * 3)(0.0, 0.0, 0.0), 1.0, 8, 4, -1, 16, fake, fake, fake, fake, fake,
                       fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_library_refuses_bad_arguments_before_any_gpu_work():
    lib = L.load()
    need = lib.sfgs_mesh_grid_scratch_bytes(4, 4, 4)
    assert need > 0
    assert lib.sfgs_mesh_grid_scratch_bytes(0, 4, 4) == 0 and lib.sfgs_mesh_grid_scratch_bytes(1 << 10, 1 << 10, 1 << 9) == 0
    assert lib.sfgs_mesh_grid_scratch_bytes(1 << 10, 1 << 10, 1 << 8) > 0
    assert lib.sfgs_mesh_sample_scratch_bytes(-1) == 0 and lib.sfgs_mesh_sample_scratch_bytes(100) > 0
    fake = C.c_void_p(0x1000)
    for entry in (lib.sfgs_mesh_grid_count, lib.sfgs_mesh_grid_fill):
        assert entry(C.byref(_grid_args()), fake, need - 1, None) == E_ARG
        assert b"scratch too small" in lib.sfgs_last_error()
        for bad in (dict(struct_size=8), dict(nx=0), dict(nx=1 << 12, ny=1 << 12, nz=1 << 5), dict(cell=0.0), dict(cell=float("nan")),
                    dict(cell=float("inf")), dict(max_cells=-2), dict(max_cells=(1 << 30) + 1), dict(capacity=-1), dict(capacity=1 << 31),
                    dict(n=(1 << 29) + 1), dict(m=0), dict(vertices=None), dict(faces=None), dict(cell_start=None), dict(state=None),
                    dict(large=None)):
            assert entry(C.byref(_grid_args(**bad)), fake, need, None) == E_ARG, bad
        assert entry(C.byref(_grid_args()), None, need, None) == E_ARG
    assert lib.sfgs_mesh_grid_fill(C.byref(_grid_args(pairs=None)), fake, need, None) == E_ARG
    close = lambda a, k=4, f64=0, md=1.0, out=fake, state=fake: lib.sfgs_mesh_closest(C.byref(a), fake, f64, k, md, out, out, None, state, None)
    for bad in (dict(k=-1), dict(f64=2), dict(md=-1.0), dict(md=float("nan")), dict(out=None), dict(state=None)):
        assert close(_grid_args(), **bad) == E_ARG, bad
    assert close(_grid_args(nz=0)) == E_ARG and close(_grid_args(pairs=None)) == E_ARG
    sample = lambda m=8, n=4, density=1.0, cap=4, pts=fake, state=fake, scratch=fake, nbytes=lib.sfgs_mesh_sample_scratch_bytes(4): \
        lib.sfgs_mesh_sample(fake, None, fake, m, n, density, 0, cap, pts, pts, None, state, scratch, nbytes, None)
    for bad in (dict(m=0), dict(n=-1), dict(density=-1.0), dict(density=float("inf")), dict(density=float("nan")), dict(cap=-1),
                dict(cap=1 << 31), dict(pts=None), dict(state=None), dict(scratch=None),
                dict(nbytes=lib.sfgs_mesh_sample_scratch_bytes(4) - 1)):
        assert sample(**bad) == E_ARG, bad
    assert lib.sfgs_mesh_sample(fake, None, fake, 8, 4, 1.0, 0, 4, fake, fake, fake, fake, fake, 1 << 20, None) == E_ARG    # colours out of none


# ---- the summary ---------------------------------------------------------------------------------------------------------------------
def test_the_restated_summary_adds_in_a_fixed_order_and_stays_within_the_bound_of_a_plain_sum():
    rng = np.random.default_rng(5)
    for k in (0, 1, 255, 257, 4096, 4097, 50000):
        sq = rng.random(k) ** 2 * 9.0
        face = np.where(rng.random(k) < 0.2, -1, 7).astype(np.int32)
        s = mq.summary(sq, face, (0.0, 1.0, 3.0))
        ok = face >= 0
        d = np.sqrt(sq[ok])
        assert (s.queries, s.answered, s.counts) == (k, int(ok.sum()), (int((d <= 0.0).sum()), int((d <= 1.0).sum()), int(ok.sum())))
        assert s.max == (d.max() if len(d) else 0.0)
        for value, want in ((s.sum_d, d.sum()), (s.sum_d2, sq[ok].sum())):
            assert abs(value - want) <= k * 2.0 ** -52 * abs(want)


def test_the_library_refuses_a_bad_summary_before_any_gpu_work():
    lib = L.load()
    fake = C.c_void_p(0x1000)
    need = lib.sfgs_mesh_distance_summary_scratch_bytes(5000)
    assert need > 0 and lib.sfgs_mesh_distance_summary_scratch_bytes(-1) == 0 and lib.sfgs_mesh_distance_summary_scratch_bytes(1 << 31) == 0
    taus = (C.c_double * 2)(0.5, 1.0)
    call = lambda k=5000, t=taus, nt=2, out=fake, scratch=fake, nbytes=need, sq=fake: \
        lib.sfgs_mesh_distance_summary(sq, fake, k, t, nt, out, scratch, nbytes, None)
    for bad in (dict(k=-1), dict(nt=17), dict(nt=-1), dict(t=None), dict(t=(C.c_double * 2)(0.5, -1.0)),
                dict(t=(C.c_double * 2)(float("nan"), 1.0)), dict(out=None), dict(scratch=None), dict(sq=None), dict(nbytes=need - 1)):
        assert call(**bad) == E_ARG, bad
    assert b"scratch too small" in lib.sfgs_last_error()
