"""Weld, connected components and clean of sfgs.mesh (csrc/mesh.hip; include/sfgs.h states the results in words) restated in
numpy from the DEFINITIONS -- np.unique over the twelve bytes, a min-label fixpoint over the edges, boolean masks -- not from the
kernels' mechanism (a hash table, union-find, scans). What the kernels and the host build of csrc/mesh_math.h are held to byte
for byte, and the scenes their tests share.

  weld                 soup -> (V, F int32, colours): first-appearance numbering, first-appearance colours
  components           (F, m) -> (labels, triangles, vertices_in, count)
  clean                the component, face and vertex rules and both order-preserving compactions
  bfs_components       a second, independent component count in plain Python
  islands_volume / strip_mesh / special_soup      the shared scenes"""
import collections

import numpy as np


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def weld(vertices, colors=None):
    """float32 [n,3,3] (, colours of the same shape) -> (V float32 [m,3], F int32 [n,3], colours float32 [m,3] or None).
    key = the twelve bytes; rep = a key's first flat index; vertices are numbered in ascending order of rep."""
    flat = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    if len(flat) == 0:
        return (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32),
                None if colors is None else np.zeros((0, 3), np.float32))
    keys = flat.view(np.dtype((np.void, 12))).reshape(-1)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)       # first[u]: the rep of unique key u
    by_appearance = np.argsort(first, kind="stable")                                  # unique keys in the order of their reps
    vid_of_unique = np.empty(len(first), dtype=np.int64)
    vid_of_unique[by_appearance] = np.arange(len(first))
    reps = first[by_appearance]
    F = vid_of_unique[inverse.reshape(-1)].reshape(-1, 3).astype(np.int32)
    C = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(-1, 3)[reps]
    return flat[reps], F, C


def components(F, m):
    """int [n,3], m -> (labels int32 [m], triangles int32 [m], vertices_in int32 [m], count). Min-label fixpoint: label[v] <= v
    always names a vertex of v's component; every edge hands the smaller of its ends' labels to the larger LABEL, then every
    label follows its own label, until the ends of every edge agree -- a component then shares one label that is its own, and
    its smallest vertex can only have itself."""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    label = np.arange(m, dtype=np.int64)
    if len(F):
        a = np.concatenate([F[:, 0], F[:, 1], F[:, 2]])
        b = np.concatenate([F[:, 1], F[:, 2], F[:, 0]])
        while True:
            la, lb = label[a], label[b]
            if (la == lb).all():                                                      # (and label[label] == label: jumped below)
                break
            np.minimum.at(label, np.maximum(la, lb), np.minimum(la, lb))              # the larger LABEL takes the smaller one
            while True:                                                               # every label follows its own label
                jumped = label[label]
                if (jumped == label).all():
                    break
                label = jumped
    triangles = np.zeros(m, dtype=np.int64)
    if len(F):
        np.add.at(triangles, label[F[:, 0]], 1)
    vertices_in = np.bincount(label, minlength=m) if m else np.zeros(0, dtype=np.int64)
    roots = label == np.arange(m)
    assert (triangles[~roots] == 0).all() and (vertices_in[~roots] == 0).all()
    return label.astype(np.int32), triangles.astype(np.int32), vertices_in.astype(np.int32), int(roots.sum())


def degenerate(F):
    F = np.asarray(F).reshape(-1, 3)
    return (F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 0] == F[:, 2])


def clean(V, F, C=None, min_triangles=None, largest=None, drop_degenerate=False):
    """-> (V', F' int32, C' or None) by the three rules; labels are those of the input mesh."""
    V, F = np.asarray(V, np.float32), np.asarray(F, np.int32).reshape(-1, 3)
    m = len(V)
    label, triangles, _, _ = components(F, m)
    roots = np.nonzero(label == np.arange(m))[0]
    keep_root = np.zeros(m, dtype=bool)
    keep_root[roots] = True
    if min_triangles is not None:
        keep_root &= triangles >= min_triangles
    if largest is not None:
        ranked = sorted(roots.tolist(), key=lambda r: (-int(triangles[r]), r))[:largest]
        top = np.zeros(m, dtype=bool)
        top[ranked] = True
        keep_root &= top
    keep_face = keep_root[label[F[:, 0]]] if len(F) else np.zeros(0, dtype=bool)
    if drop_degenerate:
        keep_face = keep_face & ~degenerate(F)
    keep_vertex = np.zeros(m, dtype=bool)
    keep_vertex[F[keep_face].reshape(-1)] = True
    rank = np.cumsum(keep_vertex) - 1
    Fo = rank[F[keep_face]].astype(np.int32).reshape(-1, 3)
    return V[keep_vertex], Fo, None if C is None else np.asarray(C, np.float32)[keep_vertex]


def bfs_components(F, m):
    """Plain Python breadth-first search -> the sorted list of (triangles, vertices, smallest vertex) per component"""
    adj = collections.defaultdict(set)
    for a, b, c in np.asarray(F).reshape(-1, 3).tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            adj[u].add(v)
            adj[v].add(u)
    seen, comp = [-1] * m, []
    for s in range(m):
        if seen[s] >= 0:
            continue
        seen[s], queue, members = s, collections.deque([s]), 0
        while queue:
            u = queue.popleft()
            members += 1
            for v in adj[u]:
                if seen[v] < 0:
                    seen[v] = s
                    queue.append(v)
        comp.append([0, members, s])
    index = {c[2]: k for k, c in enumerate(comp)}
    for a, _, _ in np.asarray(F).reshape(-1, 3).tolist():
        comp[index[seen[a]]][0] += 1
    return sorted(tuple(c) for c in comp)


def ply_vertex_colors(C):
    """The PLY colour rule: (x * 255 + 0.5).clip(0, 255) in float32, NaN -> 0, as uint8"""
    C = np.asarray(C, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(C), np.float32(0), (C * np.float32(255) + np.float32(0.5)).clip(0, 255)).astype(np.uint8)


def read_ply(path):
    """A PLY as Mesh.save_ply / TriangleSoup.save_ply write it -> (xyz [m,3] in the file's float type, rgb uint8 [m,3] or None, F int32 [n,3])"""
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
    assert "property list uchar int vertex_indices" in header
    ftype = "<f8" if "property double x" in header else "<f4"
    colours = "property uchar red" in header
    vdt = np.dtype([(a, ftype) for a in "xyz"] + ([(c, "u1") for c in ("red", "green", "blue")] if colours else []))
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    assert len(body) == m * vdt.itemsize + n * fdt.itemsize
    vt = np.frombuffer(body, dtype=vdt, count=m)
    ft = np.frombuffer(body, dtype=fdt, count=n, offset=m * vdt.itemsize)
    assert (ft["n"] == 3).all()
    xyz = np.stack([vt[a] for a in "xyz"], axis=-1)
    rgb = np.stack([vt[c] for c in ("red", "green", "blue")], axis=-1) if colours else None
    return xyz, rgb, ft["i"].astype(np.int32)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
ISLAND_SPHERES = (((11.3, 12.6, 14.2), 8.4), ((29.7, 11.2, 9.1), 5.3), ((27.4, 26.8, 20.6), 6.7), ((9.2, 28.1, 24.3), 3.2),
                  ((19.6, 20.3, 5.4), 2.1))
ISLAND_DIMS = (40, 36, 32)


def islands_volume(colors=True):
    """Five spheres and a few single-voxel specks on a 40 x 36 x 32 grid of 0.5 voxels at origin 0: eight components, two of
    them with the same triangle count, some degenerate faces (a voxel that is exactly 0) and an unobserved block that opens
    one sphere -> (tsdf, weight, rgb or None, origin, voxel_size) as tsdf_np's scenes."""
    nx, ny, nz = ISLAND_DIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    dist = np.full((nz, ny, nx), np.inf)
    for (cx, cy, cz), r in ISLAND_SPHERES:
        dist = np.minimum(dist, np.sqrt((i - cx) ** 2 + (j - cy) ** 2 + (k - cz) ** 2) - r)
    tsdf = np.clip(dist / 2.0, -1.0, 1.0).astype(np.float32)
    for x, y, z in ((36, 30, 4), (3, 3, 28), (20, 33, 29)):
        tsdf[z, y, x] = -0.4
    tsdf[28, 3, 4] = -0.7
    tsdf[16, 18, 20] = 0.0
    weight = np.ones_like(tsdf)
    weight[:, 10:14, 8:12] = 0.0
    rgb = np.stack([i / nx, 0.5 + 0.5 * np.sin(0.7 * j), (k * k) / (nz * nz)]).astype(np.float32) if colors else None
    return tsdf, weight, rgb, (0.0, 0.0, 0.0), 0.5


def strip_mesh(faces=200_000, seed=3):
    """A triangle strip of `faces` faces over faces + 2 vertices, vertex numbering and face order shuffled (seeded): one
    component whose union chains are long -> (V float32 [m,3], F int32 [n,3])"""
    rng = np.random.default_rng(seed)
    m = faces + 2
    t = np.arange(faces)
    F = np.stack([t, t + 1, t + 2], axis=-1)
    F[1::2] = F[1::2][:, [1, 0, 2]]
    number = rng.permutation(m)                                                       # strip position -> vertex index
    F = number[F][rng.permutation(faces)].astype(np.int32)
    V = np.zeros((m, 3), np.float32)
    V[number, 0] = np.arange(m) // 2
    V[number, 1] = np.arange(m) % 2
    return V, F


def special_soup():
    """Six triangles whose vertices mix +0.0 / -0.0 and NaNs with equal and with different payloads -> float32 [6,3,3]"""
    nan_a, nan_b = np.uint32(0x7fc00000), np.uint32(0x7fc00001)                       # two quiet NaNs, different payloads
    neg_nan = np.uint32(0xffc00000)
    words = np.zeros((6, 3, 3), dtype=np.uint32)
    one, neg_zero = np.float32(1.0).view(np.uint32), np.uint32(0x80000000)
    words[0] = [[0, 0, 0], [one, 0, 0], [0, one, 0]]
    words[1] = [[neg_zero, 0, 0], [one, 0, 0], [0, one, neg_zero]]                    # -0.0 is not +0.0; (1,0,0) is shared
    words[2] = [[nan_a, 0, 0], [nan_b, 0, 0], [nan_a, 0, 0]]                          # equal payloads weld, different ones do not
    words[3] = [[neg_nan, 0, 0], [nan_a, 0, 0], [0, 0, 0]]
    words[4] = [[0, neg_zero, 0], [0, 0, neg_zero], [neg_zero, 0, 0]]
    words[5] = [[nan_b, 0, 0], [0, one, 0], [nan_a, nan_a, nan_a]]
    return words.view(np.float32)
