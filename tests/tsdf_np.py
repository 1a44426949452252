"""TSDF fusion and marching-tetrahedra extraction of sfgs.tsdf (csrc/tsdf.hip, csrc/tsdf_math.h; include/sfgs.h states both
sequences in words) restated in vectorised numpy -- what the kernels and the host build of the header are held to byte for
byte -- and the scenes their tests share. Integration runs in float64 on the stored float32 values, extraction in float32;
every product, sum and quotient is spelled elementwise in the order the header takes it.

  integrate                    views into a volume, in the order given, with the outcome counts on the side
  TETS / triangles_of / winding_table      the six-tetrahedra split, the triangles of an inside mask, the 6 x 16 swap bits
  extract                      volume -> triangle soup (and colours), ordered by cell, tetrahedron, triangle
  weld / mesh_report           byte-equal vertices merged; edge counts, Euler characteristic, signed volume
  sphere_volume / fusion_scene / wavy_volume      the shared scenes"""
import collections
import itertools
import types

import numpy as np

import consistency_np as cnp

OUTCOMES = ("behind", "outside", "unused", "beyond_trunc", "update_s_one", "update_s_below_one", "update_at_cap")
# corner k of a cell has the offsets (k & 1, (k >> 1) & 1, (k >> 2) & 1) along x, y, z; a tetrahedron is a path 0 -> 7
TETS = tuple((0, 1 << a, (1 << a) | (1 << b), 7) for a, b, _ in itertools.permutations((0, 1, 2)))
Volume = collections.namedtuple("Volume", "origin dims voxel_size trunc max_weight")


def corner_offset(k):
    return np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])


# ---- integration -----------------------------------------------------------------------------------------------------------------
def empty_state(dims, colors=False):
    nx, ny, nz = dims
    return types.SimpleNamespace(tsdf=np.zeros((nz, ny, nx), np.float32), weight=np.zeros((nz, ny, nx), np.float32),
                                 rgb=np.zeros((3, nz, ny, nx), np.float32) if colors else None)


def voxel_centres(vol):
    """float64 [nz*ny*nx, 3] in the volume's linear order (x fastest): origin + (i + 0.5) * voxel_size, as written"""
    nx, ny, nz = vol.dims
    o, s = np.asarray(vol.origin, dtype=np.float64), np.float64(vol.voxel_size)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([o[a] + (idx.reshape(-1).astype(np.float64) + 0.5) * s for a, idx in enumerate((i, j, k))], axis=-1)


def integrate(state, vol, views, images=None, counters=None):
    """Fuses `views` (consistency_np.View: depth, camera, mask) into `state`, in place, in the order given. images: None or one
    float32 [3,H,W] per view (needed exactly when the state has colours). counters: a dict that receives, under the names of
    OUTCOMES, how many (voxel, view) pairs took each outcome; the first six partition the pairs, the seventh counts the updates
    whose new weight the cap cut (they are also counted under one of the two update outcomes)."""
    trunc, cap = np.float64(vol.trunc), np.float64(vol.max_weight)
    w = voxel_centres(vol)
    D, W = state.tsdf.reshape(-1), state.weight.reshape(-1)                   # views of the state: updated in place
    C = None if state.rgb is None else state.rgb.reshape(3, -1)
    n = dict.fromkeys(OUTCOMES, 0)
    for k, view in enumerate(views):
        H, Wd = view.depth.shape
        kc = cnp.constants(view.camera, H, Wd)
        alive = np.arange(len(w))
        u, v, z = cnp.project(kc, w)
        with np.errstate(invalid="ignore"):
            ok = z > 0
        n["behind"] += int((~ok).sum())
        alive, u, v, z = alive[ok], u[ok], v[ok], z[ok]
        with np.errstate(invalid="ignore"):
            fu, fv = np.floor(u + 0.5), np.floor(v + 0.5)
            ok = (fu >= 0) & (fu < Wd) & (fv >= 0) & (fv < H)
        n["outside"] += int((~ok).sum())
        alive, z, su, sv = alive[ok], z[ok], fu[ok].astype(np.int64), fv[ok].astype(np.int64)
        ok = cnp.used_pixels(view.depth, view.mask)[sv, su]
        n["unused"] += int((~ok).sum())
        alive, z, su, sv = alive[ok], z[ok], su[ok], sv[ok]
        sdf = view.depth[sv, su].astype(np.float64) - z
        ok = ~(sdf < -trunc)
        n["beyond_trunc"] += int((~ok).sum())
        alive, sdf, su, sv = alive[ok], sdf[ok], su[ok], sv[ok]
        s = np.minimum(1.0, sdf / trunc)
        n["update_s_one"] += int((s == 1.0).sum())
        n["update_s_below_one"] += int((s < 1.0).sum())
        Wo, Do = W[alive].astype(np.float64), D[alive].astype(np.float64)
        D[alive] = ((Wo * Do + s) / (Wo + 1.0)).astype(np.float32)
        if C is not None:
            for ch in range(3):
                pix = images[k][ch][sv, su].astype(np.float64)
                C[ch, alive] = ((Wo * C[ch, alive].astype(np.float64) + pix) / (Wo + 1.0)).astype(np.float32)
        n["update_at_cap"] += int((Wo + 1.0 > cap).sum())
        W[alive] = np.minimum(Wo + 1.0, cap).astype(np.float32)
    if counters is not None:
        counters.update(n)
    return state


# ---- the split and its triangles -------------------------------------------------------------------------------------------------
def triangles_of(mask):
    """Inside mask over a tetrahedron's four local vertices (bit l: vertex l is inside) -> its triangles BEFORE the winding swap:
    a list of triangles, each three edges (i, j) of local vertices, inside end first."""
    ins = [l for l in range(4) if mask >> l & 1]
    outs = [l for l in range(4) if not mask >> l & 1]
    if len(ins) == 1:
        return [tuple((ins[0], j) for j in outs)]
    if len(ins) == 3:
        return [tuple((i, outs[0]) for i in ins)]
    if len(ins) == 2:
        q = ((ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0]))
        return [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return []


def winding_table():
    """bool [6,16]: swap the last two vertices of the triangles of (tetrahedron, inside mask)? Decided by geometry with every cut
    at its edge's midpoint: (b - a) x (c - a) must point from the inside vertices toward the outside ones."""
    swap = np.zeros((6, 16), dtype=bool)
    for t, tet in enumerate(TETS):
        p = np.array([corner_offset(k) for k in tet], dtype=np.float64)
        for mask in range(1, 15):
            ins = [l for l in range(4) if mask >> l & 1]
            outs = [l for l in range(4) if not mask >> l & 1]
            outward = p[outs].mean(axis=0) - p[ins].mean(axis=0)
            signs = []
            for tri in triangles_of(mask):
                a, b, c = (0.5 * (p[i] + p[j]) for i, j in tri)
                signs.append(float(np.dot(np.cross(b - a, c - a), outward)))
            assert all(s != 0 for s in signs) and len({s > 0 for s in signs}) == 1, (t, mask, signs)
            swap[t, mask] = signs[0] < 0
    return swap


def extract(tsdf, weight, origin, voxel_size, rgb=None):
    """-> (vertices float32 [n,3,3], colors float32 [n,3,3] or None): the soup in the order cell, tetrahedron, triangle."""
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    nz, ny, nx = tsdf.shape
    o32, s32 = np.asarray(origin, dtype=np.float64).astype(np.float32), np.float32(voxel_size)
    swap = winding_table()
    if min(nx, ny, nz) < 2:
        return np.zeros((0, 3, 3), np.float32), None if rgb is None else np.zeros((0, 3, 3), np.float32)

    def corner(a, k):
        dx, dy, dz = corner_offset(k)
        return a[..., dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].reshape(a.shape[:-3] + (-1,))

    val = [corner(tsdf, k) for k in range(8)]
    col = None if rgb is None else [corner(np.asarray(rgb, np.float32), k) for k in range(8)]
    with np.errstate(invalid="ignore"):
        used = np.all([corner(weight, k) > 0 for k in range(8)], axis=0)
        inside = [v < 0 for v in val]
    cz, cy, cx = (a.reshape(-1) for a in np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij"))
    base = (cx, cy, cz)
    keys, rows, crows = [], [], []
    for t, tet in enumerate(TETS):
        mt = sum(inside[k].astype(np.int64) << l for l, k in enumerate(tet))
        for mask in range(1, 15):
            cells = np.nonzero(used & (mt == mask))[0]
            if not len(cells):
                continue
            points = {}

            def point(edge):
                la, lb = min(edge), max(edge)                                 # canonical: the lower linear voxel index is `a`
                if (la, lb) not in points:
                    ka, kb = tet[la], tet[lb]
                    va, vb = val[ka][cells], val[kb][cells]
                    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                        tt = va / (va - vb)
                        xyz = []
                        for ax in range(3):
                            pa = (base[ax][cells] + corner_offset(ka)[ax]).astype(np.float32)
                            pb = (base[ax][cells] + corner_offset(kb)[ax]).astype(np.float32)
                            pos = pa + tt * (pb - pa)
                            xyz.append(o32[ax] + (pos + np.float32(0.5)) * s32)
                        c = None if col is None else [col[ka][ch][cells] + tt * (col[kb][ch][cells] - col[ka][ch][cells]) for ch in range(3)]
                    points[la, lb] = (np.stack(xyz, axis=-1), None if c is None else np.stack(c, axis=-1))
                return points[la, lb]

            for j, tri in enumerate(triangles_of(mask)):
                if swap[t, mask]:
                    tri = (tri[0], tri[2], tri[1])
                pts = [point(e) for e in tri]
                rows.append(np.stack([p[0] for p in pts], axis=1))
                if col is not None:
                    crows.append(np.stack([p[1] for p in pts], axis=1))
                keys.append(cells * 16 + t * 2 + j)
    if not rows:
        return np.zeros((0, 3, 3), np.float32), None if rgb is None else np.zeros((0, 3, 3), np.float32)
    order = np.argsort(np.concatenate(keys), kind="stable")
    verts = np.concatenate(rows)[order].astype(np.float32)
    return verts, None if col is None else np.concatenate(crows)[order].astype(np.float32)


# ---- mesh properties -------------------------------------------------------------------------------------------------------------
def weld(vertices):
    """float32 [n,3,3] -> (V float32 [m,3], F int64 [n,3]): vertices with the same twelve bytes become one"""
    flat = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    keys = flat.view(np.dtype((np.void, 12))).reshape(-1)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    return flat[first], inverse.reshape(-1, 3).astype(np.int64)


def mesh_report(vertices):
    """Welds the soup -> namespace: V, F, degenerate (triangles with two equal vertex indices), undirected / directed (arrays of
    the multiplicities of the undirected and the directed edges), euler, volume (float64, by the divergence theorem)"""
    V, F = weld(vertices)
    degenerate = int(((F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 0] == F[:, 2])).sum())
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    directed = np.unique(e, axis=0, return_counts=True)[1]
    und, undirected = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    p = V.astype(np.float64)[F]
    volume = float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
    return types.SimpleNamespace(V=V, F=F, degenerate=degenerate, undirected=undirected, directed=directed,
                                 euler=len(V) - len(und) + len(F), volume=volume)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
SPHERE = types.SimpleNamespace(n=14, centre=(6.37, 6.61, 6.53), radius=4.3, trunc=2.0)


def sphere_volume(colors=False):
    """-> (tsdf, weight, rgb or None, origin, voxel_size): the signed distance to SPHERE on a 14^3 grid of unit voxels whose index
    IS the position (origin -0.5), clipped at +-trunc; every weight 1. The colours are smooth functions of the position."""
    n = SPHERE.n
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    c = SPHERE.centre
    dist = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - SPHERE.radius
    tsdf = np.clip(dist, -SPHERE.trunc, SPHERE.trunc).astype(np.float32)
    rgb = np.stack([i / n, 0.5 + 0.5 * np.sin(0.7 * j), (k * k) / (n * n)]).astype(np.float32) if colors else None
    return tsdf, np.ones_like(tsdf), rgb, (-0.5, -0.5, -0.5), 1.0


def look_at(eye, target, W, H, up=(0.0, 0.0, 1.0)):
    """A Camera-like object (R, T as geometry_np.look_down_camera forms them) at `eye` looking at `target` (x right, y down, z forward): fx = 0.9 W, fy = 1.1 fx, the principal point off
    centre by (+1.3, -0.7) pixels."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    A = np.stack([r, d, f], axis=1)                                           # columns: the camera's axes in the world
    fx = 0.9 * W
    return types.SimpleNamespace(R=A, T=-A @ eye, focal_x=fx, focal_y=1.1 * fx, cx=2 * 1.3 / W, cy=2 * -0.7 / H, eye=eye)


def scene_depth(cam, H, W):
    """float64 [H,W]: depth along the forward axis of the nearest of the plane z = 0 and the sphere of radius 1.5 at (0,0,1.5);
    0 where a ray meets neither"""
    k = cnp.constants(cam, H, W)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    dirs = np.stack([(u - k.cx_pix) / k.focal_x, (v - k.cy_pix) / k.focal_y, np.ones_like(u)], axis=-1) @ k.M      # forward part 1
    with np.errstate(divide="ignore", invalid="ignore"):
        t_plane = -cam.eye[2] / dirs[..., 2]
    t_plane = np.where(t_plane > 0, t_plane, np.inf)
    oc = cam.eye - np.array([0.0, 0.0, 1.5])
    a, b, c = (dirs * dirs).sum(-1), 2.0 * (dirs @ oc), oc @ oc - 1.5 * 1.5
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        t_sph = (-b - np.sqrt(disc)) / (2 * a)
    t_sph = np.where((disc >= 0) & (t_sph > 0), t_sph, np.inf)
    t = np.minimum(t_plane, t_sph)
    return np.where(np.isfinite(t), t, 0.0)


FUSION = Volume(origin=(-6.0, -5.0, -1.0), dims=(24, 20, 16), voxel_size=0.5, trunc=1.5, max_weight=2.0)
FUSION_EYES = ((8.0, -6.0, 9.0), (-7.0, 5.0, 8.0), (1.0, 9.0, 7.0), (0.5, 0.5, 3.2), (-9.0, -9.0, 6.0))


def fusion_scene(seed=5):
    """-> (FUSION, views, images): five views of the plane and the sphere, 48 x 40 but the third at 37 x 29, 3 % NaN pixels plus
    one each of +inf, 0 and -1 per view, a random mask on the second view; images are seeded noise."""
    rng = np.random.default_rng(seed)
    views, images = [], []
    for n, eye in enumerate(FUSION_EYES):
        W, H = (37, 29) if n == 2 else (48, 40)
        cam = look_at(eye, (0.0, 0.0, 1.0), W, H)
        depth = scene_depth(cam, H, W).astype(np.float32)
        depth[rng.random((H, W)) < 0.03] = np.nan
        for bad in (np.inf, 0.0, -1.0):
            depth[rng.integers(H), rng.integers(W)] = bad
        mask = rng.random((H, W)) > 0.15 if n == 1 else None
        views.append(cnp.View(depth, cam, mask))
        images.append(rng.random((3, H, W)).astype(np.float32))
    return FUSION, views, images


def wavy_volume(dims=(72, 64, 64), colors=False):
    """A wavy height field z = h(x, y) as a TSDF on dims = (nx, ny, nz) voxels of 0.25 (trunc 4 voxels), weights 1 but for an
    unobserved block -> (tsdf, weight, rgb or None, origin, voxel_size)"""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    h = 0.5 * nz + 0.45 * nz * np.sin(0.21 * i + 0.3) * np.cos(0.17 * j - 0.2)
    tsdf = np.clip((k - h) / 4.0, -1.0, 1.0).astype(np.float32)
    weight = np.ones_like(tsdf)
    weight[:, 5:11, 7:15] = 0.0
    rgb = np.stack([i / nx, j / ny, k / nz]).astype(np.float32) if colors else None
    return tsdf, weight, rgb, (3.0, -2.0, 10.0), 0.25
