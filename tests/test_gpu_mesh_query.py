"""GPU tests of the mesh queries (csrc/mesh_query.hip): Mesh.face_grid, Mesh.closest, Mesh.sample. The reference is the numpy
restatement tests/mesh_query_np.py (held to the host build of the product's header, to independent spellings and to its own ring
search by tests/test_mesh_query_host.py). Nothing here reads the reference tree.

Bounds. Every comparison is assert-equal on BYTES: the table is integers, a query's answer the minimum of (d2, face index) with d2
a float64 expression written once for the device, the host build and numpy, a sample's row such an expression as well -- there is
nothing to tolerate. The large list alone is compared as a set: its order is that of arrival and no answer depends on it.

Routes. A face whose cell range holds more than max_cells cells goes to the large list that every query tests in full. Every
scene runs with _max_cells = 0 (every face on the list: brute force on the device), the default and 2^30 (every face in the grid),
twice each, with float64 and with float32 points, and must give the same bytes.
Shapes: 17 338 faces over 8 704 vertices (many workgroups of 256, no multiple of it); the fan's cell list of 5 000; the frame-filling
quad whose two faces are large at the default; 1, 63, 64, 65, 129 and 257 queries (partial waves, partial workgroups); grids of one
cell, of 3 x 3 x 1 up to 191 x 126 x 2, and one of 168 x 168 x 152 = 4 290 048 cells = 1 048 chunks of 4 096, where the scan's top
level takes its second round with a carry; a given grid smaller than the mesh (clamped ranges, queries outside the grid)."""
import functools

import numpy as np
import pytest
import torch

import mesh_query_np as mq
import mesh_render_np as mrn
from test_gpu_scratch_contract import contract, refused

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = (0, None, 1 << 30)
SCENES = list(mq.scenes())


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the shared scenes are read-only


def device_mesh(V, F, Cc=None):
    from sfgs.mesh import Mesh
    return Mesh(dev(np.asarray(V, np.float32)), dev(np.asarray(F, np.int32)), dev(Cc))


def same(t, want, what):
    want = np.ascontiguousarray(want)
    assert t.device == torch.device(DEV) and tuple(t.shape) == want.shape and str(t.dtype) == f"torch.{want.dtype}", (what, t.dtype, t.shape)
    np.testing.assert_array_equal(t.cpu().numpy().reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8), err_msg=what)


def same_grid(grid, ref, what):
    assert tuple(grid.dims) == tuple(ref.dims) and grid.cell == ref.cell, what
    np.testing.assert_array_equal(np.asarray(grid.origin, np.float64).view(np.uint64), ref.origin.view(np.uint64), err_msg=what)
    assert grid.check() == (len(ref.pairs), len(ref.large), ref.skipped), what
    same(grid.cell_start, ref.cell_start, f"cell_start, {what}")
    same(grid.pairs, ref.pairs, f"pairs, {what}")
    np.testing.assert_array_equal(np.sort(grid.large[:len(ref.large)].cpu().numpy()), ref.large, err_msg=f"large, {what}")


def same_answer(got, ref, what):
    sq, face, point, counts = ref
    same(got.sqdist, sq, f"sqdist, {what}")
    same(got.face, face, f"face, {what}")
    if got.point is not None:
        same(got.point, point, f"point, {what}")
    assert got.counts.dtype == torch.int64 and got.counts.device == torch.device(DEV)
    assert got.counts.tolist() == counts.tolist() and got.check() == tuple(counts.tolist()), what
    same(got.distance, np.sqrt(sq), f"distance, {what}")


def rows(ref, sel):
    """the brute-force answer for a subset of the queries: every query is answered on its own"""
    sq, face, point, counts = ref
    answered = int((face[sel] >= 0).sum())
    return sq[sel], face[sel], point[sel], np.array([answered, len(face[sel]) - answered, counts[2]], np.int64)


@functools.lru_cache(maxsize=None)
def reference(name, f32=False, max_distance=np.inf):
    V, F, _, _, P = mq.scenes()[name]
    if max_distance != np.inf:               # mq.closest's own last step on the answers without a limit: the brute force runs once
        sq, face, point, counts = reference(name, f32)
        out = [np.array(a) for a in (sq, face, point)]
        for i in range(len(face)):
            out[0][i], out[1][i], out[2][i] = mq._finish(sq[i], face[i], point[i], max_distance)
        answered = int((out[1] >= 0).sum())
        out.append(np.array([answered, len(face) - answered, counts[2]], np.int64))
    else:
        out = mq.closest(V, F, P.astype(np.float32).astype(np.float64) if f32 else P)
    mrn.frozen(*out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference_grid(name, route):
    V, F, _, g, _ = mq.scenes()[name]
    return mq.face_grid(V, F, g["cell"], g["origin"], g["dims"], max_cells=mq.MAX_CELLS_DEFAULT if route is None else route)


# ---- the kernels equal the restatement, by every route, run after run ------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_every_scene_equals_the_restatement_by_every_route(name):
    V, F, Cc, g, P = mq.scenes()[name]
    mesh = device_mesh(V, F, Cc)
    P64, P32 = dev(P), dev(P.astype(np.float32))
    for route in ROUTES:
        for run in (1, 2):
            what = f"{name}, _max_cells {route}, run {run}"
            grid = mesh.face_grid(g["cell"], g["origin"], g["dims"], _max_cells=route)
            same_grid(grid, reference_grid(name, route), what)
            same_answer(mesh.closest(P64, grid, closest_points=True), reference(name), what)
            same_answer(mesh.closest(P32, grid, closest_points=True), reference(name, True), what + ", float32 points")
    md = 0.4 * g["cell"]
    for route in ROUTES:
        same_answer(mesh.closest(P64, g["cell"], max_distance=md, _max_cells=route) if g["origin"] is None else
                    mesh.closest(P64, mesh.face_grid(g["cell"], g["origin"], g["dims"], _max_cells=route), max_distance=md),
                    reference(name, False, md), f"{name}, max_distance, _max_cells {route}")


@pytest.mark.parametrize("k", (1, 63, 64, 65, 257))
def test_partial_waves_and_workgroups_of_queries(k):
    V, F, Cc, g, P = mq.scenes()["islands"]
    mesh = device_mesh(V, F, Cc)
    sel = slice(257 - k, 257)
    got = mesh.closest(dev(P[sel]), g["cell"], closest_points=True)
    same_answer(got, rows(reference("islands"), sel), f"{k} queries")
    none = mesh.closest(dev(P[:0]), got.grid)
    assert none.sqdist.shape == (0,) and none.check() == (0, 0, 0)


def test_a_grid_whose_scan_takes_a_second_round_with_a_carry():
    V, F, Cc, _, P = mq.scenes()["islands"]
    lo, hi = V.astype(np.float64).min(axis=0), V.astype(np.float64).max(axis=0)
    cell, dims = float((hi[2] - lo[2]) / 151.5), (168, 168, 152)                # the top of the mesh in the last layers of cells
    assert dims[0] * dims[1] * dims[2] > 4096 * 1024
    ref = mq.face_grid(V, F, cell, lo, dims)
    assert ref.cell_start[4096 * 1024] > 0 and ref.cell_start[-1] > ref.cell_start[4096 * 1024]      # pairs on both sides of the round
    mesh = device_mesh(V, F, Cc)
    for run in (1, 2):
        grid = mesh.face_grid(cell, lo, dims)
        same_grid(grid, ref, f"168 x 168 x 152, run {run}")
    near = P[np.isfinite(P).all(axis=1) & (np.abs(P).max(axis=1) < 100.0)][:65]
    sq, face, point, counts = mq.closest(V, F, near)
    same_answer(mesh.closest(dev(near), grid, closest_points=True), (sq, face, point, counts), "168 x 168 x 152")


def test_bounds_and_the_default_cell_are_the_restatements():
    from sfgs.mesh import default_cell
    for name in ("islands", "special soup", "no faces", "square"):
        V, F, Cc, _, P = mq.scenes()[name]
        mesh = device_mesh(V, F, Cc)
        m, n = mesh._sizes()
        cell = mq.default_cell(V, F)
        assert default_cell(mesh._grid_bounds(m, n), n) == cell
        got = mesh.closest(dev(P))
        same_grid(got.grid, mq.face_grid(V, F, cell), f"the default grid, {name}")
        same_answer(got, reference(name), f"the default grid, {name}")


def test_a_capacity_one_short_is_reported_by_check_with_the_number_needed():
    V, F, Cc, g, P = mq.scenes()["islands"]
    mesh = device_mesh(V, F, Cc)
    ref = reference_grid("islands", None)
    need = len(ref.pairs)
    exact = mesh.face_grid(g["cell"], capacity=need)
    same_grid(exact, ref, "capacity given exactly")
    roomy = mesh.face_grid(g["cell"], capacity=need + 1000)
    assert roomy.check() == (need, 0, 0)
    same(roomy.pairs[:need], ref.pairs, "pairs, capacity with room")
    same_answer(mesh.closest(dev(P), roomy), reference("islands"), "capacity with room")
    short = mesh.face_grid(g["cell"], capacity=need - 1)
    assert int(short.num_pairs) == need
    with pytest.raises(ValueError, match=f"{need} .* capacity {need - 1}.*{need} would have sufficed"):
        short.check()


def test_the_device_pipeline_with_buffers_longer_than_their_counts():
    """extract -> mesh() -> clean -> face_grid / closest / sample"""
    from sfgs.tsdf import TsdfVolume
    tsdf, weight, rgb, origin, voxel = mrn.mnp.islands_volume(True)
    nz, ny, nx = tsdf.shape
    v = TsdfVolume(origin, (nx, ny, nz), voxel, trunc=1.0, colors=True, device=DEV)
    v.load(dev(tsdf), dev(weight), dev(rgb))
    mesh = v.extract(20000).mesh()
    assert mesh.vertex_buffer.shape[0] > 8704
    V, F, Cc, g, P = mq.scenes()["islands"]
    same_answer(mesh.closest(dev(P), g["cell"], closest_points=True), reference("islands"), "the device's own mesh")
    Vn, Fn, Cn = mrn.mnp.clean(V, F, Cc, min_triangles=64)
    cleaned = mesh.clean(min_triangles=64)
    assert cleaned.face_buffer.shape[0] > len(Fn) and cleaned.vertex_buffer.shape[0] > len(Vn)
    grid = cleaned.face_grid(voxel, origin, (nx, ny, nz))                        # the volume's own grid
    same_grid(grid, mq.face_grid(Vn, Fn, voxel, origin, (nx, ny, nz)), "the cleaned mesh in the volume's grid")
    same_answer(cleaned.closest(dev(P[:65]), grid, closest_points=True), mq.closest(Vn, Fn, P[:65]), "the cleaned mesh")
    ref = mq.sample(Vn, Fn, Cn, 1.0 / (voxel * voxel), 3)
    got = cleaned.sample(1.0 / (voxel * voxel), seed=3)
    same(got.points, ref.points, "samples of the cleaned mesh"), same(got.face, ref.face, "faces"), same(got.colors, ref.colors, "colours")


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, density", (("islands", 2.0), ("sphere", 7.5), ("square", 3.0), ("fan", 40.0), ("no faces", 1.0)))
def test_sample_equals_the_restatement(name, density):
    V, F, Cc, _, _ = mq.scenes()[name]
    mesh = device_mesh(V, F, Cc)
    for seed in (0, 12345):
        ref = mq.sample(V, F, Cc, density, seed)
        for capacity in (None, len(ref.points) + 77):
            for run in (1, 2):
                got = mesh.sample(density, seed=seed, capacity=capacity)
                assert int(got.count) == len(ref.points) and got.point_buffer.shape[0] == (capacity or len(ref.points))
                same(got.points, ref.points, f"points, {name}, seed {seed}")
                same(got.face, ref.face, f"face, {name}, seed {seed}")
                assert (got.colors is None) == (Cc is None)
                if Cc is not None:
                    same(got.colors, ref.colors, f"colors, {name}, seed {seed}")
    assert mesh.sample(density, colors=False).colors is None


def test_a_sample_capacity_too_small_behaves_as_extracts():
    V, F, Cc, _, _ = mq.scenes()["sphere"]
    mesh = device_mesh(V, F, Cc)
    ref = mq.sample(V, F, Cc, 7.5, 1)
    k = len(ref.points)
    got = mesh.sample(7.5, seed=1, capacity=k - 100)
    assert int(got.count) == k
    same(got.point_buffer, ref.points[:k - 100], "the rows that fit"), same(got.face_buffer, ref.face[:k - 100], "their faces")
    with pytest.raises(ValueError, match=f"{k} samples found, capacity {k - 100}"):
        got.points


def test_a_face_that_cannot_be_sampled_raises():
    V, F = mrn.special_mesh()
    mesh = device_mesh(V, F)
    ref = mq.sample(V, F, None, 3.0, 2)
    got = mesh.sample(3.0, seed=2, capacity=len(ref.points) + 5)
    assert int(got.count) == len(ref.points)
    same(got.point_buffer[:len(ref.points)], ref.points, "the other faces' samples")
    with pytest.raises(ValueError, match="area that is not finite"):
        got.points
    with pytest.raises(ValueError, match="area that is not finite"):
        mesh.sample(3.0, seed=2)


# ---- the summary and the comparison of two meshes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, k", (("islands", 257), ("sphere", 129), ("no faces", 1)))
def test_summary_counts_are_exact_and_its_sums_are_numpys(name, k):
    """The two sums against numpy's float64 sums within k 2^-52 relative (k terms, each addition rounded once), as the issue sets;
    and, beyond that, the bytes of the restatement that adds in the kernel's order."""
    V, F, Cc, g, P = mq.scenes()[name]
    md = 2.0 * g["cell"]
    got = device_mesh(V, F, Cc).closest(dev(P), g["cell"], max_distance=md)
    sq, face, _, counts = reference(name, False, md)
    taus = (0.0, 0.25 * g["cell"], g["cell"], md, 1e30)
    first = got.summary(taus)
    ok = face >= 0
    d = np.sqrt(sq[ok])
    assert (first.queries, first.answered) == (k, int(ok.sum())) and first.thresholds == taus
    assert first.counts == tuple(int((d <= t).sum()) for t in taus) and first.counts[-1] == first.answered
    for value, want in ((first.sum_d, d.sum()), (first.sum_d2, sq[ok].sum())):
        assert abs(value - want) <= k * 2.0 ** -52 * abs(want), (value, want)
    ref = mq.summary(sq, face, taus)
    assert (first.sum_d, first.sum_d2, first.max, first.counts) == (ref.sum_d, ref.sum_d2, ref.max, ref.counts)
    assert first.max == (d.max() if len(d) else 0.0)
    if len(d):
        assert first.mean == first.sum_d / len(d) and first.rms == np.sqrt(first.sum_d2 / len(d))
        assert first.fractions == tuple(c / k for c in first.counts)
    second = got.summary(taus)
    assert np.array([second.sum_d, second.sum_d2, second.max]).tobytes() == np.array([first.sum_d, first.sum_d2, first.max]).tobytes()
    assert second.counts == first.counts
    assert got.summary().counts == ()


def test_summary_over_several_workgroups_is_the_same_bytes_run_after_run():
    """20 001 queries: five workgroups of 4 096 and the last one partial, so the pass over the partials has work to do"""
    V, F, Cc, _, _ = mq.scenes()["sphere"]
    mesh = device_mesh(V, F, Cc)
    rng = np.random.default_rng(12)
    P = rng.uniform(V.min(axis=0) - 2.0, V.max(axis=0) + 2.0, (20001, 3))
    got = mesh.closest(dev(P), 1.0, max_distance=1.5)
    sq, face = got.sqdist.cpu().numpy(), got.face.cpu().numpy()
    taus = (0.1, 0.5, 1.5)
    ref = mq.summary(sq, face, taus)
    ok = face >= 0
    assert 0 < ok.sum() < len(P)
    for run in (1, 2, 3):
        s = got.summary(taus)
        assert (s.answered, s.counts) == (int(ok.sum()), ref.counts), run
        assert (s.sum_d, s.sum_d2, s.max) == (ref.sum_d, ref.sum_d2, ref.max), run
        for value, want in ((s.sum_d, np.sqrt(sq[ok]).sum()), (s.sum_d2, sq[ok].sum())):
            assert abs(value - want) <= len(P) * 2.0 ** -52 * abs(want)


def test_compare_of_a_mesh_with_itself_has_mean_exactly_zero():
    """The square [8, 16]^2 at z = 0: a sample is float32 of a point of the square, so it lies in the plane and -- 8 and 16 being
    float32 values -- inside the closed square, hence ON one of the two faces. All coordinates there are multiples of 2^-20 below
    16, the edge vectors are +-8, every product in the closest-point function has at most 46 bits and every denominator is a power of
    two: the function is exact and returns d2 = 0 for each sample, so the mean is exactly 0 and every threshold holds everything."""
    from sfgs.mesh import compare
    V, F = mrn.square_mesh(8.0, 8.0, 8.0)
    a, b = device_mesh(V, F), device_mesh(V, F)
    c = compare(a, b, 40.0, max_distance=1.0, thresholds=(0.0, 0.5), seed=4)
    assert c.a_to_b.queries == c.a_to_b.answered > 2000 and c.b_to_a.answered == c.a_to_b.answered
    assert c.a_to_b.mean == 0.0 and c.b_to_a.mean == 0.0 and c.chamfer == 0.0 and c.a_to_b.max == 0.0 and c.a_to_b.rms == 0.0
    assert c.precision == (1.0, 1.0) and c.recall == (1.0, 1.0) and c.fscore == (1.0, 1.0)
    same = compare(a, a, 40.0, thresholds=(0.0,))
    assert same.chamfer == 0.0 and same.fscore == (1.0,)


def test_compare_is_its_parts_and_tells_two_meshes_apart():
    from sfgs.mesh import compare
    V, F, Cc, _, _ = mq.scenes()["sphere"]
    a, b = device_mesh(V, F, Cc), device_mesh(V + np.float32(0.25), F, Cc)
    taus = (0.1, 0.3, 1.0)
    c = compare(a, b, 5.0, max_distance=2.0, thresholds=taus, seed=2)
    sa, sb = mq.sample(V, F, None, 5.0, 2), mq.sample(V + np.float32(0.25), F, None, 5.0, 2)
    for got, pts in ((c.a_to_b, sa.points), (c.b_to_a, sb.points)):
        assert got.queries == len(pts) and got.answered == len(pts)
    assert 0.0 < c.chamfer < 0.25 * np.sqrt(3.0) + 1e-6 and c.chamfer == 0.5 * (c.a_to_b.mean + c.b_to_a.mean)
    assert c.precision == c.a_to_b.fractions and c.recall == c.b_to_a.fractions and c.precision[-1] == 1.0 and c.precision[0] < 1.0
    assert c.fscore == tuple(2 * p * r / (p + r) if p + r else 0.0 for p, r in zip(c.precision, c.recall))
    ref = mq.summary(*[t.cpu().numpy() for t in (lambda d: (d.sqdist, d.face))(b.closest(dev(sa.points), max_distance=2.0))], taus)
    assert (c.a_to_b.sum_d, c.a_to_b.counts) == (ref.sum_d, ref.counts)


def test_the_summary_keeps_the_scratch_contract(monkeypatch):
    V, F, Cc, g, P = mq.scenes()["islands"]
    d = device_mesh(V, F, Cc).closest(dev(P), g["cell"])

    def run():
        s = d.summary((0.5, 1.0))
        return dict(sums=np.array([s.sum_d, s.sum_d2, s.max]), counts=list(s.counts), answered=s.answered)
    contract(monkeypatch, run)
    refused(monkeypatch, run, short_for="sfgs.mesh.summary")


# ---- faces left out ---------------------------------------------------------------------------------------------------------------------
def test_a_bad_face_index_and_a_nan_vertex_are_left_out_and_counted():
    from sfgs.mesh import Mesh
    V, F, Cc, g, P = mq.scenes()["sphere"]
    bad, Vn = np.array(F), np.array(V)
    bad[5, 1], bad[100, 0] = len(V) + 3, -1
    Vn[bad[200, 2]] = np.nan
    left = int((~mq.usable_faces(Vn, bad)).sum())
    assert left >= 3
    good = device_mesh(Vn, F)
    broken = Mesh._made(good.vertex_buffer, dev(bad), None, torch.tensor([len(V), len(F), 0, 0], device=DEV), "test")
    ref = mq.closest(Vn, bad, P)
    assert ref[3][2] == left
    for route in ROUTES:
        grid = broken.face_grid(g["cell"], _max_cells=route)
        same_grid(grid, mq.face_grid(Vn, bad, g["cell"], max_cells=mq.MAX_CELLS_DEFAULT if route is None else route), f"route {route}")
        assert int(grid.skipped) == left
        got = broken.closest(dev(P), grid, closest_points=True)
        same_answer(got, ref, f"faces left out, route {route}")
        assert got.check()[2] == left
    whole = mq.closest(V, F, P)
    keep = ~np.isin(whole[1], np.flatnonzero(~mq.usable_faces(Vn, bad)))         # the whole mesh's winner is still there
    assert keep.sum() > len(P) // 2
    np.testing.assert_array_equal(ref[1][keep], whole[1][keep])                  # the other answers are unchanged
    np.testing.assert_array_equal(ref[0][keep], whole[0][keep])
    finite = Mesh._made(device_mesh(V, F).vertex_buffer, dev(bad), None, torch.tensor([len(V), len(F), 0, 0], device=DEV), "test")
    with pytest.raises(ValueError, match="face index"):
        finite.sample(1.0).points


# ---- the scratch contract -----------------------------------------------------------------------------------------------------------------
def grid_run(name, route=None):
    V, F, Cc, g, P = mq.scenes()[name]
    mesh, pts = device_mesh(V, F, Cc), dev(P)

    def run():
        grid = mesh.face_grid(g["cell"], g["origin"], g["dims"], _max_cells=route)
        d = mesh.closest(pts, grid, closest_points=True)
        pairs, large, skipped = grid.check()
        return dict(cell_start=grid.cell_start, pairs=grid.pairs, large=torch.sort(grid.large[:large]).values, sizes=[pairs, large, skipped],
                    sqdist=d.sqdist, face=d.face, point=d.point, counts=d.counts)
    return run


def sample_run(name, density):
    V, F, Cc, _, _ = mq.scenes()[name]
    mesh = device_mesh(V, F, Cc)

    def run():
        s = mesh.sample(density, seed=7)
        return dict(points=s.points, face=s.face, colors=s.colors, count=s.count)
    return run


@pytest.mark.parametrize("name, route", (("islands", None), ("quad in a fine grid", None), ("fan", 1 << 30), ("special soup", 0)))
def test_the_grid_keeps_the_scratch_contract(monkeypatch, name, route):
    contract(monkeypatch, grid_run(name, route))


def test_the_sampler_keeps_the_scratch_contract(monkeypatch):
    contract(monkeypatch, sample_run("islands", 2.0))


def test_a_scratch_one_byte_short_is_refused_before_any_launch(monkeypatch):
    refused(monkeypatch, grid_run("islands"), short_for="sfgs.mesh.face_grid")
    refused(monkeypatch, sample_run("islands", 2.0), short_for="sfgs.mesh.sample")


# ---- the wrapper's refusals ---------------------------------------------------------------------------------------------------------------
def test_wrong_arguments_raise_value_error_and_launch_nothing():
    V, F, Cc, g, P = mq.scenes()["square"]
    mesh, other = device_mesh(V, F), device_mesh(V, F)
    pts = dev(P)
    for kw in (dict(cell=0.0), dict(cell=float("nan")), dict(cell=1.0, origin=(0, 0, 0)), dict(cell=1.0, dims=(2, 2, 2)),
               dict(cell=1.0, origin=(0, 0, 0), dims=(0, 2, 2)), dict(cell=1.0, origin=(0, 0, 0), dims=(1 << 10, 1 << 10, 1 << 9)),
               dict(cell=1.0, origin=(0, float("inf"), 0), dims=(2, 2, 2)), dict(cell=1.0, capacity=-1), dict(cell=1.0, _max_cells=-1)):
        with pytest.raises(ValueError):
            mesh.face_grid(**kw)
    grid = other.face_grid(1.0)
    for args, kw in (((pts, grid), {}), ((pts.cpu(),), {}), ((pts.to(torch.float16),), {}), ((pts[:, :2],), {}), ((pts,), dict(max_distance=-1.0)),
                     ((pts,), dict(max_distance=float("nan")))):
        with pytest.raises(ValueError):
            mesh.closest(*args, **kw)
    for kw in (dict(density=-1.0), dict(density=float("inf")), dict(density=1.0, seed=-1), dict(density=1.0, seed=1 << 32),
               dict(density=1.0, capacity=0)):
        with pytest.raises(ValueError):
            mesh.sample(**kw)
