"""Decimation by vertex clustering, the vertex -> face adjacency and the vertex normals of sfgs.mesh (csrc/mesh.hip;
include/sfgs.h states the results in words) restated in numpy from the DEFINITIONS -- np.unique over the cell rows, np.add.at
over uint64, a stable argsort, a loop over the position inside a segment -- not from the kernels' mechanism (a hash table,
atomics, scans, per-segment sorts). What the kernels and the host build of csrc/mesh_math.h are held to byte for byte.

  cells                (V, cell, origin) -> (i int64 [m,3], p uint64 [m,3], bad bool [m])
  decimate             -> (V', F' int32, C' or None, vertex_map int32 [m], info): info counts what the fixture guards assert
  vertex_faces         (F, m) -> (offsets int32 [m+1], records int32 [3n])
  face_normals / vertex_normals
  write-side helpers   read_ply (knows normals), fan_mesh, height_field

All float64 arithmetic is one numpy operation at a time, each rounded once."""
import numpy as np

TWO32 = np.float64(4294967296.0)
INV32 = np.float64(1.0) / TWO32
ST_BAD_INDEX, ST_BAD_VERTEX = 8, 16
# the (cell, origin) pairs the islands mesh is decimated at; the last makes every cell index negative (floor, not truncation)
ISLAND_CASES = ((0.75, (0.0, 0.0, 0.0)), (0.5, (0.13, -0.2, 0.31)), (1.0, (0.0, 0.0, 0.0)), (2.0, (0.0, 0.0, 0.0)),
                (0.75, (30.5, 7.25, -3.0)))


def cells(V, cell, origin=(0.0, 0.0, 0.0)):
    """u = (float64(V) - origin) / cell, i = floor(u), f = u - i, p = uint64(floor(f 2^32)); bad: u not finite or i outside int32"""
    V = np.asarray(V, np.float32).reshape(-1, 3)
    org = np.asarray(origin, np.float64).reshape(3)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (V.astype(np.float64) - org[None, :]) / np.float64(cell)
        fl = np.floor(u)
        bad_axis = ~np.isfinite(u) | (fl < -2147483648.0) | (fl > 2147483647.0)
        bad = bad_axis.any(axis=1)
        f = u - fl
        p = np.floor(f * TWO32)
    ok = ~bad
    i = np.zeros(V.shape, np.int64)
    pp = np.zeros(V.shape, np.uint64)
    i[ok] = fl[ok].astype(np.int64)
    pp[ok] = p[ok].astype(np.uint64)
    return i, pp, bad


def color_fix(C):
    """NaN -> 0, clamped to [0, 1] in float64, uint64(floor(x 2^32))"""
    x = np.asarray(C, np.float32).astype(np.float64)
    x = np.where(np.isnan(x), np.float64(0.0), x)
    x = np.minimum(np.maximum(x, np.float64(0.0)), np.float64(1.0))
    return np.floor(x * TWO32).astype(np.uint64)


def decimate(V, F, C=None, cell=1.0, origin=(0.0, 0.0, 0.0), drop_duplicates=True):
    """-> (V' float32 [m',3], F' int32 [n',3], C' or None, vertex_map int32 [m], info dict)"""
    V = np.ascontiguousarray(V, np.float32).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    C = None if C is None else np.ascontiguousarray(C, np.float32).reshape(-1, 3)
    m, n = len(V), len(F)
    org = np.asarray(origin, np.float64).reshape(3)
    cell = np.float64(cell)
    i, p, bad = cells(V, cell, org)
    good = np.nonzero(~bad)[0]
    status = ST_BAD_VERTEX if bad.any() else 0
    # clusters: equal int32 triples, numbered by their smallest member
    cluster_of = np.full(m, -1, np.int64)
    K = 0
    first = np.zeros(0, np.int64)
    if len(good):
        keys = np.ascontiguousarray(i[good].astype(np.int32)).view(np.dtype((np.void, 12))).reshape(-1)
        _, first_u, inverse = np.unique(keys, return_index=True, return_inverse=True)
        order = np.argsort(first_u, kind="stable")
        cid_of_unique = np.empty(len(first_u), np.int64)
        cid_of_unique[order] = np.arange(len(first_u))
        cluster_of[good] = cid_of_unique[inverse.reshape(-1)]
        first = good[first_u[order]]                                                   # the smallest member of every cluster
        K = len(first)
    count = np.bincount(cluster_of[good], minlength=K).astype(np.uint64)
    S = np.zeros((K, 3), np.uint64)
    np.add.at(S, cluster_of[good], p[good])
    single = count == 1
    P = np.zeros((K, 3), np.float32)
    Pc = None
    if K:
        q = S // count[:, None]
        inside = q.astype(np.float64) * INV32
        base = i[first].astype(np.float64) + inside
        prod = base * cell
        with np.errstate(over="ignore"):
            P = (prod + org[None, :]).astype(np.float32)
        P[single] = V[first[single]]
    if C is not None:
        Sc = np.zeros((K, 3), np.uint64)
        np.add.at(Sc, cluster_of[good], color_fix(C[good]))
        Pc = np.zeros((K, 3), np.float32)
        if K:
            Pc = ((Sc // count[:, None]).astype(np.float64) * INV32).astype(np.float32)
            Pc[single] = C[first[single]]
    # faces
    in_range = ((F >= 0) & (F < m)).all(axis=1) if n else np.zeros(0, bool)
    if n and not in_range.all():
        status |= ST_BAD_INDEX
    G = np.zeros((n, 3), np.int64)
    G[in_range] = cluster_of[F[in_range]]
    alive = in_range & (G >= 0).all(axis=1)
    collapsed = alive & ((G[:, 0] == G[:, 1]) | (G[:, 1] == G[:, 2]) | (G[:, 0] == G[:, 2]))
    cand = alive & ~collapsed
    keep_face = cand.copy()
    duplicates = 0
    idx = np.nonzero(cand)[0]
    if len(idx):
        sorted_keys = np.ascontiguousarray(np.sort(G[idx], axis=1).astype(np.int32)).view(np.dtype((np.void, 12))).reshape(-1)
        _, first_f = np.unique(sorted_keys, return_index=True)
        is_first = np.zeros(len(idx), bool)
        is_first[first_f] = True
        duplicates = int((~is_first).sum())
        if drop_duplicates:
            keep_face[idx[~is_first]] = False
    keep_cluster = np.zeros(K, bool)
    keep_cluster[G[keep_face].reshape(-1)] = True
    rank = np.cumsum(keep_cluster) - 1
    Fo = rank[G[keep_face]].astype(np.int32).reshape(-1, 3)
    vmap = np.full(m, -1, np.int32)
    has = cluster_of >= 0
    kept = np.zeros(m, bool)
    kept[has] = keep_cluster[cluster_of[has]]
    vmap[kept] = rank[cluster_of[kept]].astype(np.int32)
    info = {"clusters": K, "single": int(single.sum()), "collapsed": int(collapsed.sum()), "duplicates": duplicates,
            "unreferenced": int(K - keep_cluster.sum()), "bad": int(bad.sum()), "status": status,
            "cluster_of": cluster_of, "keep_cluster": keep_cluster}
    return P[keep_cluster], Fo, None if Pc is None else Pc[keep_cluster], vmap, info


def vertex_faces(F, m):
    """-> (offsets int32 [m+1], records int32 [3n]): the stable argsort of the flattened faces and the cumulative counts"""
    flat = np.asarray(F, np.int64).reshape(-1)
    records = np.argsort(flat, kind="stable").astype(np.int32)
    offsets = np.zeros(m + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(flat, minlength=m)) if m else 0
    return offsets.astype(np.int32), records


def face_normals(V, F):
    """float64 [n,3]: (b - a) x (c - a) from the float32 positions, every product and difference rounded once"""
    V = np.asarray(V, np.float32).astype(np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    e1, e2 = b - a, c - a
    with np.errstate(invalid="ignore", over="ignore"):
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.stack([nx, ny, nz], axis=-1)


def vertex_normals(V, F, adjacency=None):
    """float32 [m,3]: per vertex the sum of its records' face normals in ascending record order from +0.0, normalised"""
    m = len(V)
    offsets, records = vertex_faces(F, m) if adjacency is None else adjacency
    offsets, records = offsets.astype(np.int64), records.astype(np.int64)
    fn = face_normals(V, F)
    N = np.zeros((m, 3), np.float64)
    valence = np.diff(offsets)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(int(valence.max()) if m else 0):                                # the j-th record of every vertex that has one
            at = np.nonzero(valence > j)[0]
            N[at] = N[at] + fn[records[offsets[at] + j] // 3]
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        ok = (length > 0) & np.isfinite(length)
        out = np.zeros((m, 3), np.float32)
        out[ok] = (N[ok] / length[ok, None]).astype(np.float32)
    return out


# ---- helpers of the tests --------------------------------------------------------------------------------------------------------
def read_ply(path):
    """A PLY as Mesh.save_ply writes it, normals included -> (xyz, normals float32 [m,3] or None, rgb uint8 [m,3] or None, F int32)"""
    with open(path, "rb") as f:
        header = []
        while True:
            line = f.readline().decode("ascii").strip()
            header.append(line)
            if line == "end_header":
                break
        body = f.read()
    assert header[:2] == ["ply", "format binary_little_endian 1.0"], header[:2]
    m = int([h for h in header if h.startswith("element vertex")][0].split()[-1])
    n = int([h for h in header if h.startswith("element face")][0].split()[-1])
    props = [h.split()[1:] for h in header if h.startswith("property ") and not h.startswith("property list")]
    names = [p[1] for p in props]
    types = {"double": "<f8", "float": "<f4", "uchar": "u1"}
    vdt = np.dtype([(name, types[kind]) for kind, name in props])
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    assert len(body) == m * vdt.itemsize + n * fdt.itemsize
    vt = np.frombuffer(body, dtype=vdt, count=m)
    ft = np.frombuffer(body, dtype=fdt, count=n, offset=m * vdt.itemsize)
    xyz = np.stack([vt[a] for a in "xyz"], axis=-1)
    normals = np.stack([vt[a] for a in ("nx", "ny", "nz")], axis=-1) if "nx" in names else None
    rgb = np.stack([vt[c] for c in ("red", "green", "blue")], axis=-1) if "red" in names else None
    return xyz, normals, rgb, ft["i"].astype(np.int32), names


def fan_mesh(spokes=5000, seed=5):
    """A fan of `spokes` faces around hub vertex 0 over spokes + 2 vertices, the faces shuffled and their corners rotated, so
    the hub sits in any of the three places -> (V float32 [m,3], F int32 [n,3])"""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0.0, 1.5 * np.pi, spokes + 1)
    V = np.zeros((spokes + 2, 3), np.float32)
    V[1:, 0], V[1:, 1], V[1:, 2] = np.cos(ang), np.sin(ang), 0.01 * np.arange(spokes + 1)
    t = np.arange(spokes)
    F = np.stack([np.zeros(spokes, np.int64), t + 1, t + 2], axis=-1)
    turn = rng.integers(0, 3, spokes)
    F = np.stack([F[t, (0 + turn) % 3], F[t, (1 + turn) % 3], F[t, (2 + turn) % 3]], axis=-1)
    return V, F[rng.permutation(spokes)].astype(np.int32)


def height_field(nx, ny):
    """An nx x ny grid of integer-coordinate vertices (x, y, z = (x // 2 + y // 2) % 3), row-major, two triangles per quad ->
    (V float32 [nx ny, 3], F int32 [2 (nx-1)(ny-1), 3]); with nx, ny even, cell = 2 and origin -0.5 every cluster is a 2 x 2 block
    of one height"""
    x, y = np.meshgrid(np.arange(nx, dtype=np.int64), np.arange(ny, dtype=np.int64), indexing="xy")
    V = np.stack([x, y, (x // 2 + y // 2) % 3], axis=-1).reshape(-1, 3).astype(np.float32)
    qx, qy = np.meshgrid(np.arange(nx - 1, dtype=np.int64), np.arange(ny - 1, dtype=np.int64), indexing="xy")
    v00 = (qy * nx + qx).reshape(-1)
    F = np.empty((len(v00), 2, 3), np.int64)
    F[:, 0] = np.stack([v00, v00 + 1, v00 + nx], axis=-1)
    F[:, 1] = np.stack([v00 + 1, v00 + nx + 1, v00 + nx], axis=-1)
    return V, F.reshape(-1, 3).astype(np.int32)
