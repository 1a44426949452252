"""numpy restatement of csrc/mesh_query.hip (include/sfgs.h, "Mesh queries"): the face grid as a CSR table, the closest face of a
point as brute force over all faces, a ring search in plain Python that must equal the brute force (the proof of the stop rule,
run on the CPU), the sampler, and the scenes the host and the GPU tests share. Float64, one rounded operation at a time in the
header's order. Test infrastructure only; needs neither torch nor a GPU."""
import functools
import types

import numpy as np

import mesh_render_np as mrn
import mesh_simplify_np as snp

MAX_CELLS_DEFAULT = 4096
MARGIN = 1.0 - 2.0 ** -20
CELL_LIMIT = 2 ** 30
MAX_SAMPLES_PER_FACE = 1 << 20
ST_BAD_INDEX, ST_CAPACITY, ST_PAIRS, ST_BAD_FACE = 8, 32, 64, 128


def _f64(V):
    return np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3).astype(np.float64)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


# ---- the cell function and the grid -------------------------------------------------------------------------------------------------
def cell_of(x, origin, cell):
    with np.errstate(all="ignore"):
        return np.floor((np.asarray(x, dtype=np.float64) - np.float64(origin)) / np.float64(cell))


def usable_faces(V, F):
    """-> bool [n]: the faces NOT left out (every index in range, every coordinate finite)"""
    V, F = _f64(V), np.asarray(F).reshape(-1, 3)
    ok = ((F >= 0) & (F < len(V))).all(axis=1)
    P = V[np.clip(F, 0, max(len(V) - 1, 0))] if len(V) else np.zeros((len(F), 3, 3))
    return ok & np.isfinite(P).all(axis=(1, 2))


def grid_from_bounds(V, F, cell):
    """origin = the minimum of the referenced finite vertices, dims = floor((max - origin) / cell) + 1; (zeros, (1, 1, 1)) without one"""
    ok = usable_faces(V, F)
    if not ok.any():
        return np.zeros(3), (1, 1, 1)
    P = _f64(V)[np.asarray(F).reshape(-1, 3)[ok]].reshape(-1, 3)
    lo, hi = P.min(axis=0) + 0.0, P.max(axis=0) + 0.0                       # + 0.0: a minimum of -0.0 and +0.0 is +0.0 either way
    return lo, tuple(int(d) for d in np.floor((hi - lo) / np.float64(cell)) + 1.0)


def default_cell(V, F):
    ok = usable_faces(V, F)
    n = len(np.asarray(F).reshape(-1, 3))
    if not ok.any():
        return 1.0
    P = _f64(V)[np.asarray(F).reshape(-1, 3)[ok]].reshape(-1, 3)
    ex, ey, ez = (float(h) - float(l) for l, h in zip(P.min(axis=0), P.max(axis=0)))
    cell = max(float(np.sqrt((ex * ey + ey * ez + ez * ex) / n)), max(ex, ey, ez) / 512.0)
    return cell if cell > 0.0 and np.isfinite(cell) else 1.0


def face_ranges(V, F, cell, origin, dims):
    """-> (usable bool [n], lo int64 [n,3], hi int64 [n,3]): the clamped cell range of every usable face"""
    Vd, F = _f64(V), np.asarray(F).reshape(-1, 3)
    ok = usable_faces(V, F)
    lo, hi = np.zeros((len(F), 3), np.int64), np.zeros((len(F), 3), np.int64)
    P = Vd[F[ok]]                                        # [u,3,3]
    for a in range(3):
        lo[ok, a] = np.clip(cell_of(P[:, :, a].min(axis=1), origin[a], cell), 0, dims[a] - 1).astype(np.int64)
        hi[ok, a] = np.clip(cell_of(P[:, :, a].max(axis=1), origin[a], cell), 0, dims[a] - 1).astype(np.int64)
    return ok, lo, hi


def face_grid(V, F, cell, origin=None, dims=None, max_cells=MAX_CELLS_DEFAULT):
    """-> namespace(cell, origin, dims, cell_start int32 [cells + 1], pairs int32, large int32 ascending, skipped)"""
    if origin is None:
        origin, dims = grid_from_bounds(V, F, cell)
    origin, dims = np.asarray(origin, dtype=np.float64), tuple(int(d) for d in dims)
    ok, lo, hi = face_ranges(V, F, cell, origin, dims)
    cover = np.prod(hi - lo + 1, axis=1)
    large = np.flatnonzero(ok & (cover > max_cells)).astype(np.int32)
    cells_of, faces_of = [], []
    for t in np.flatnonzero(ok & (cover <= max_cells)):
        z, y, x = np.mgrid[lo[t, 2]:hi[t, 2] + 1, lo[t, 1]:hi[t, 1] + 1, lo[t, 0]:hi[t, 0] + 1]
        c = ((z * dims[1] + y) * dims[0] + x).reshape(-1)
        cells_of.append(c)
        faces_of.append(np.full(len(c), t, np.int64))
    cells = dims[0] * dims[1] * dims[2]
    c = np.concatenate(cells_of) if cells_of else np.zeros(0, np.int64)
    f = np.concatenate(faces_of) if faces_of else np.zeros(0, np.int64)
    order = np.lexsort((f, c))
    cell_start = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=cells))]).astype(np.int32)
    return types.SimpleNamespace(cell=float(cell), origin=origin, dims=dims, cell_start=cell_start, pairs=f[order].astype(np.int32),
                                 large=large, skipped=int((~ok).sum()))


# ---- the closest point of a triangle -----------------------------------------------------------------------------------------------
def tri_closest(p, a, b, c):
    """p float64 [3]; a, b, c float64 [n,3] -> (d2 [n], q [n,3]): mq_closest over n faces at once"""
    with np.errstate(all="ignore"):
        ab, ac, bc, ap, bp, cp = b - a, c - a, c - b, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6

        def quot(num, den):
            return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)

        s = (va + vb) + vc
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        picks = [a, b, a + quot(d1, d1 - d3)[:, None] * ab, c, a + quot(d2, d2 - d6)[:, None] * ac,
                 b + quot(e43, e43 + e56)[:, None] * bc]
        q = (a + quot(vb, s)[:, None] * ab) + quot(vc, s)[:, None] * ac
        for cond, pick in zip(conds[::-1], picks[::-1]):           # the first condition that holds decides
            q = np.where(cond[:, None], pick, q)
        d = p - q
        return _dot(d, d), q


def _finish(best, face, q, max_distance):
    max_d2 = np.float64(max_distance) * np.float64(max_distance)
    if face >= 0 and best > max_d2:
        face = -1
    if face < 0:
        return np.inf, -1, np.zeros(3, np.float32)
    with np.errstate(all="ignore"):
        return best, face, q.astype(np.float32)


def closest(V, F, points, max_distance=np.inf):
    """Brute force: every point against every face -> (sqdist float64 [k], face int32 [k], point float32 [k,3], counts int64 [3])"""
    Vd, F = _f64(V), np.asarray(F).reshape(-1, 3)
    ok = usable_faces(V, F)
    idx = np.flatnonzero(ok)
    a, b, c = (Vd[F[idx, j]] for j in range(3))
    points = np.asarray(points).reshape(-1, 3).astype(np.float64)
    sq, fo, po = np.full(len(points), np.inf), np.full(len(points), -1, np.int32), np.zeros((len(points), 3), np.float32)
    for i, p in enumerate(points):
        if not np.isfinite(p).all() or not len(idx):
            continue
        d2, q = tri_closest(p, a, b, c)
        d2 = np.where(np.isfinite(d2), d2, np.inf)
        j = int(np.argmin(d2))                                     # the first minimum: the smallest face index
        if np.isfinite(d2[j]):
            sq[i], fo[i], po[i] = _finish(d2[j], int(idx[j]), q[j], max_distance)
    answered = int((fo >= 0).sum())
    return sq, fo, po, np.array([answered, len(points) - answered, int((~ok).sum())], np.int64)


def ring_search(grid, V, F, p, max_distance=np.inf, stats=None):
    """The kernel's search for ONE point, in plain Python over the CSR table `grid` -> (sqdist, face, point float32 [3])"""
    Vd, F = _f64(V), np.asarray(F).reshape(-1, 3)
    p = np.asarray(p, dtype=np.float64)
    best, face, bq = np.inf, -1, np.zeros(3)

    def test(ts):
        nonlocal best, face, bq
        ts = np.asarray(ts, dtype=np.int64)
        if not len(ts):
            return
        d2, q = tri_closest(p, Vd[F[ts, 0]], Vd[F[ts, 1]], Vd[F[ts, 2]])
        for t, d, qq in zip(ts, d2, q):
            if np.isfinite(d) and (d < best or (d == best and (face < 0 or t < face))):
                best, face, bq = d, int(t), qq

    if not np.isfinite(p).all():
        return np.inf, -1, np.zeros(3, np.float32)
    test(grid.large)
    nx, ny, nz = grid.dims
    q = [int(np.clip(cell_of(p[a], grid.origin[a], grid.cell), -CELL_LIMIT, CELL_LIMIT)) for a in range(3)]
    first = max(-q[a] if q[a] < 0 else max(q[a] - (grid.dims[a] - 1), 0) for a in range(3))
    last = max(max(abs(q[a]), abs(grid.dims[a] - 1 - q[a])) for a in range(3))

    def beyond(r):
        return (np.float64(r) * np.float64(grid.cell)) * MARGIN > max_distance

    rings = 0
    if len(grid.pairs):
        for r in range(first, last + 1):
            rings += 1
            lo = [max(q[a] - r, 0) for a in range(3)]
            hi = [min(q[a] + r, grid.dims[a] - 1) for a in range(3)]
            for z in range(lo[2], hi[2] + 1):
                for y in range(lo[1], hi[1] + 1):
                    if abs(z - q[2]) == r or abs(y - q[1]) == r:
                        xs = range(lo[0], hi[0] + 1)
                    else:
                        xs = [x for x in sorted({q[0] - r, q[0] + r}) if 0 <= x <= nx - 1]
                    for x in xs:
                        c = (z * ny + y) * nx + x
                        test(grid.pairs[grid.cell_start[c]:grid.cell_start[c + 1]])
            rc = np.float64(r) * np.float64(grid.cell)
            if best < (rc * rc) * MARGIN or beyond(r):
                break
    if stats is not None:
        stats.append(rings)
    return _finish(best, face, bq, max_distance)


# ---- the summary -----------------------------------------------------------------------------------------------------------------------
SUM_CHUNK, SUM_THREADS = 4096, 256


def _fixed_order_sum(x, op=np.add):
    """the kernel's order: per workgroup of 4096 items thread t adds its items t, t + 256, ... from +0.0, then a binary tree over the
    256 threads; the workgroups' sums are combined the same way, thread t taking workgroups t, t + 256, ..."""
    x = np.asarray(x, dtype=np.float64)
    nb = max(-(-len(x) // SUM_CHUNK), 1)
    pad = np.zeros(nb * SUM_CHUNK)
    pad[:len(x)] = x
    acc = np.zeros((nb, SUM_THREADS))
    for it in range(SUM_CHUNK // SUM_THREADS):
        acc = op(acc, pad.reshape(nb, SUM_CHUNK // SUM_THREADS, SUM_THREADS)[:, it])
    s = SUM_THREADS // 2
    while s:
        acc[:, :s] = op(acc[:, :s], acc[:, s:2 * s])
        s //= 2
    partial = acc[:, 0]
    acc = np.zeros(SUM_THREADS)                                    # one workgroup over the partials
    for b0 in range(0, len(partial), SUM_THREADS):
        part = partial[b0:b0 + SUM_THREADS]
        acc[:len(part)] = op(acc[:len(part)], part)
    s = SUM_THREADS // 2
    while s:
        acc[:s] = op(acc[:s], acc[s:2 * s])
        s //= 2
    return float(acc[0])


def summary(sqdist, face, thresholds=()):
    """-> namespace(queries, answered, sum_d, sum_d2, max, counts): over the answered queries; the sums in the kernel's order.
    An unanswered query adds +0.0 in its place, which changes no sum of values >= 0."""
    sqdist, face = np.asarray(sqdist, dtype=np.float64), np.asarray(face)
    ok = face >= 0
    d2 = np.where(ok, sqdist, 0.0)
    d = np.sqrt(d2)
    return types.SimpleNamespace(queries=len(face), answered=int(ok.sum()), sum_d=_fixed_order_sum(d), sum_d2=_fixed_order_sum(d2),
                                 max=_fixed_order_sum(d, np.maximum), counts=tuple(int((ok & (d <= t)).sum()) for t in thresholds))


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
def _fmix(h):
    h = h ^ (h >> np.uint32(16)); h = h * np.uint32(0x85ebca6b); h = h ^ (h >> np.uint32(13)); h = h * np.uint32(0xc2b2ae35)
    return h ^ (h >> np.uint32(16))


def mix3(seed, face, counter):
    """uint32 arrays (or scalars) -> uint32 array"""
    seed, face, counter = (np.atleast_1d(np.asarray(v, dtype=np.uint32)) for v in (seed, face, counter))
    h = _fmix(seed ^ np.uint32(0x9e3779b9))
    h = _fmix(h ^ face * np.uint32(0x7feb352d))
    return _fmix(h ^ counter * np.uint32(0x846ca68b))


def unit(h):
    return (h.astype(np.float64) + 0.5) * 2.0 ** -32


def face_areas(V, F):
    """float64 [n] over faces whose indices are in range (others NaN)"""
    Vd, F = _f64(V), np.asarray(F).reshape(-1, 3)
    ok = ((F >= 0) & (F < len(Vd))).all(axis=1)
    Fc = np.clip(F, 0, max(len(Vd) - 1, 0))
    a, b, c = Vd[Fc[:, 0]], Vd[Fc[:, 1]], Vd[Fc[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=-1)
        A = 0.5 * np.sqrt(_dot(N, N))
    return np.where(ok, A, np.nan), ok


def sample_counts(V, F, density, seed):
    """-> (count int64 [n], status)"""
    A, ok = face_areas(V, F)
    n = len(A)
    with np.errstate(all="ignore"):
        e = A * np.float64(density)
        fl = np.floor(e)
        bad = ok & (~np.isfinite(e) | (fl > MAX_SAMPLES_PER_FACE))
        u = unit(mix3(seed, np.arange(n, dtype=np.uint32), 0xffffffff))
        good = ok & ~bad
        cnt = np.where(good, np.where(good, fl, 0.0).astype(np.int64) + (u < e - fl), 0)
    over = cnt > MAX_SAMPLES_PER_FACE
    cnt = np.where(over, 0, cnt)
    status = (ST_BAD_INDEX if (~ok).any() else 0) | (ST_BAD_FACE if (bad | over).any() else 0)
    return cnt.astype(np.int64), status


def sample(V, F, C, density, seed=0):
    """-> namespace(points float32 [k,3], face int32 [k], colors float32 [k,3] or None, status)"""
    Vf, F = np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3), np.asarray(F).reshape(-1, 3)
    cnt, status = sample_counts(V, F, density, seed)
    face = np.repeat(np.arange(len(F), dtype=np.int64), cnt)
    j = np.arange(len(face), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    u1 = unit(mix3(seed, face.astype(np.uint32), (2 * j).astype(np.uint32)))
    u2 = unit(mix3(seed, face.astype(np.uint32), (2 * j + 1).astype(np.uint32)))
    flip = u1 + u2 > 1.0
    u1, u2 = np.where(flip, 1.0 - u1, u1), np.where(flip, 1.0 - u2, u2)

    def attr(X):
        a, b, c = (X[F[face, k]].astype(np.float64) for k in range(3))
        with np.errstate(all="ignore"):
            return ((a + u1[:, None] * (b - a)) + u2[:, None] * (c - a)).astype(np.float32)

    colors = None if C is None else attr(np.ascontiguousarray(C, dtype=np.float32).reshape(-1, 3))
    return types.SimpleNamespace(points=attr(Vf), face=face.astype(np.int32), colors=colors, status=status, counts=cnt)


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def queries(V, F, grid, count, seed):
    """`count` float64 points: random ones in the grid's box blown up by a third, then (overwriting the first rows) vertices of the
    mesh, corners and face centres of cells, points far outside, and one that is not finite"""
    rng = np.random.default_rng(seed)
    lo = grid.origin
    ext = np.asarray(grid.dims) * grid.cell
    P = lo - ext / 3 + rng.random((count, 3)) * ext * (5 / 3)
    usable = np.flatnonzero(usable_faces(V, F))
    special = []
    if len(usable):
        Vd = _f64(V)
        for t in usable[rng.integers(0, len(usable), 8)]:
            special.append(Vd[np.asarray(F).reshape(-1, 3)[t, rng.integers(0, 3)]])
    for _ in range(8):
        ijk = rng.integers(0, np.asarray(grid.dims) + 1)
        special.append(lo + ijk * grid.cell)                                   # a cell corner
        special.append(lo + (ijk + np.array([0.5, 0.5, 0.0])) * grid.cell)      # the middle of a cell's face
    special += [lo - 40.0 * ext - 3.0, lo + 55.0 * ext + 1.0, lo + np.array([0.3, -70.0, 0.4]) * ext, np.array([1e30, 0.0, -1e30]),
                np.array([np.nan, 0.0, 0.0]), np.array([0.0, np.inf, 0.0])]
    special = np.array(special)[:count]
    P[:len(special)] = special
    return P


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (V, F, C, face_grid keywords (cell, origin, dims), points float64 [k,3]): what the host and the GPU tests share"""
    out = {}

    def add(name, V, F, C, cell, origin=None, dims=None, count=129, seed=1):
        g = face_grid(V, F, cell, origin, dims)
        P = queries(V, F, g, count, seed)
        mrn.frozen(P)
        out[name] = (V, F, C, dict(cell=cell, origin=None if origin is None else tuple(origin), dims=dims), P)

    V, F, C = mrn.islands_mesh()
    add("islands", V, F, C, 1.5, count=257)
    lo, _ = grid_from_bounds(V, F, 1.0)
    add("islands, a given grid smaller than the mesh", V, F, C, 1.0, lo + 3.25, (7, 5, 4), count=65, seed=2)
    add("islands, one cell", V, F, C, 2.0, lo + 1.0, (1, 1, 1), count=63, seed=3)
    Vs, Fs = mrn.special_mesh()
    add("special soup", Vs, Fs, None, 0.75, seed=4)
    add("stacked faces", *mrn.stacked_mesh(), 2.0, seed=5)
    Vf, Ff = snp.fan_mesh(5000)
    add("fan", Vf, Ff, None, 1.0, count=64, seed=6)
    add("quad in a fine grid", *mrn.quad_mesh("plain"), 1.0, count=65, seed=7)
    Vq, Fq = mrn.square_mesh()
    add("square", Vq, Fq, None, 3.0, seed=8)
    add("sphere", *mrn.sphere_mesh(), 1.0, seed=9)
    Vh, Fh = snp.height_field(33, 17)
    add("height field", Vh, Fh, None, 2.0, seed=10)
    add("no faces", np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32), None, 1.0, count=1, seed=11)
    return out
