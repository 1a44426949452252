"""The mesh rasteriser (include/sfgs.h, "Mesh rendering"; csrc/mesh_raster_math.h) restated in numpy from those definitions, and the
scenes its tests share. The kernels and the host build of the header are held to render() byte for byte. Test infrastructure only;
needs neither torch nor a GPU."""
import functools
import types

import numpy as np

import consistency_np as cnp
import mesh_np as mnp
import mesh_simplify_np as snp
import tsdf_np as tnp
import tsdf_raycast_np as rnp

SNAP = 256
GUARD = 1 << 28
EMPTY = np.uint64(0xffffffffffffffff)
SMALL_MAX_DEFAULT = 64
COUNTS = ("drawn", "culled", "clipped", "degenerate")
ST_BAD_INDEX = 8


def camera_sign(k):
    """+1 / -1: the sign of focal_x focal_y det(M), det in the header's order"""
    M = k.M.reshape(-1)
    det = (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6])
    return -1 if (det < 0.0) != ((k.focal_x < 0.0) != (k.focal_y < 0.0)) else 1


def project_vertices(V, k, near=0.0):
    """-> (X int64 [m], Y int64 [m], z float64 [m], usable bool [m]); X, Y, z are 0 where the vertex is unusable"""
    w = np.asarray(V, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u, v, z = cnp.project(k, w)
        ok = np.isfinite(u) & np.isfinite(v) & np.isfinite(z) & ~(z <= np.float64(near))
        xd, yd = np.rint(u * np.float64(SNAP)), np.rint(v * np.float64(SNAP))
        ok &= (np.abs(xd) <= GUARD) & (np.abs(yd) <= GUARD)
    X, Y = np.where(ok, xd, 0.0).astype(np.int64), np.where(ok, yd, 0.0).astype(np.int64)
    return X, Y, np.where(ok, z, 0.0), ok


def face_setup(V, F, k, near=0.0, cull=None):
    """-> namespace X, Y int64 [n,3], z float64 [n,3], As, A int64 [n], sgn int64 [n], outcome int [n] (index into COUNTS),
    bad_index bool"""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    m = len(np.asarray(V).reshape(-1, 3))
    X, Y, z, ok = project_vertices(V, k, near)
    index_ok = ((F >= 0) & (F < m)).all(axis=1) if len(F) else np.zeros(0, bool)
    Fc = np.where(index_ok[:, None], F, 0)
    clipped = ~index_ok | ~ok[Fc].all(axis=1) if m else np.ones(len(F), bool)
    fx, fy, fz = (X[Fc], Y[Fc], z[Fc]) if m else (np.zeros((len(F), 3), np.int64),) * 2 + (np.zeros((len(F), 3)),)
    As = (fx[:, 1] - fx[:, 0]) * (fy[:, 2] - fy[:, 0]) - (fy[:, 1] - fy[:, 0]) * (fx[:, 2] - fx[:, 0])
    degenerate = ~clipped & (As == 0)
    facing = (As < 0) == (camera_sign(k) > 0)
    culled = ~clipped & ~degenerate & ~facing if cull == "back" else np.zeros(len(F), bool)
    outcome = np.where(clipped, 2, np.where(degenerate, 3, np.where(culled, 1, 0)))
    return types.SimpleNamespace(X=fx, Y=fy, z=fz, As=As, A=np.abs(As), sgn=np.where(As < 0, -1, 1).astype(np.int64), outcome=outcome,
                                 bad_index=bool((~index_ok).any()))


def edge_dir(S, t, i):
    j, kk = (i + 1) % 3, (i + 2) % 3
    return S.sgn[t] * (S.X[t, kk] - S.X[t, j]), S.sgn[t] * (S.Y[t, kk] - S.Y[t, j])


def edges(S, t, col, row):
    """faces t, pixels (col, row), arrays of one length -> (E int64 [3,k], inside bool [k])"""
    t, col, row = np.asarray(t, np.int64), np.asarray(col, np.int64), np.asarray(row, np.int64)
    E, inside = [], np.ones(len(t), bool)
    for i in range(3):
        j = (i + 1) % 3
        dx, dy = edge_dir(S, t, i)
        e = dx * (SNAP * row - S.Y[t, j]) - dy * (SNAP * col - S.X[t, j])
        inside &= (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
        E.append(e)
    return np.stack(E), inside


def depth_of(S, t, E):
    """-> (depth float32 [k], q float64 [3,k], s float64 [k])"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = np.stack([E[i].astype(np.float64) / S.z[t, i] for i in range(3)])
        s = (q[0] + q[1]) + q[2]
        return (S.A[t].astype(np.float64) / s).astype(np.float32), q, s


def boxes(S, H, W):
    """-> c0, c1, r0, r1 int64 [n]: the clipped box of every face (meaningless where it is not drawn)"""
    c0 = np.maximum((S.X.min(axis=1) + 255) >> 8, 0)
    c1 = np.minimum(S.X.max(axis=1) >> 8, W - 1)
    r0 = np.maximum((S.Y.min(axis=1) + 255) >> 8, 0)
    r1 = np.minimum(S.Y.max(axis=1) >> 8, H - 1)
    return c0, c1, r0, r1


def normalize(N):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        ok = (length > 0) & np.isfinite(length)
        out = np.zeros((len(N), 3), np.float32)
        out[ok] = (N[ok] / length[ok, None]).astype(np.float32)
    return out


def interp(q, s, a0, a1, a2):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        b0, b1, b2 = q[0] / s, q[1] / s, q[2] / s
        return (b0 * a0.astype(np.float64) + b1 * a1.astype(np.float64)) + b2 * a2.astype(np.float64)


def render(V, F, C, camera, H, W, near=0.0, far=np.inf, normals=True, cull=None):
    """-> namespace depth float32 [1,H,W], face int32 [H,W], normal float32 [3,H,W] or None, rgb float32 [3,H,W] or None, counts
    int64 [4], status, cover int32 [H,W] (how many drawn faces cover each pixel centre, before the depth test), setup.
    normals: True (flat), False, or float32 [m,3] (interpolated)."""
    V = np.asarray(V, np.float32).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    k = cnp.constants(camera, H, W)
    S = face_setup(V, F, k, near, cull)
    P = H * W
    keys, cover = np.full(P, EMPTY, np.uint64), np.zeros(P, np.int32)
    far = np.float64(far)

    def rasterise(t, col, row):
        E, inside = edges(S, t, col, row)
        t, col, row, E = t[inside], col[inside], row[inside], E[:, inside]
        np.add.at(cover, row * W + col, 1)
        d, _, _ = depth_of(S, t, E)
        with np.errstate(invalid="ignore"):
            kept = (d > 0) & (d.astype(np.float64) <= far)
        key = (d[kept].view(np.uint32).astype(np.uint64) << np.uint64(32)) | t[kept].astype(np.uint64)
        np.minimum.at(keys, (row * W + col)[kept], key)

    c0, c1, r0, r1 = boxes(S, H, W)
    drawn = np.nonzero((S.outcome == 0) & (c0 <= c1) & (r0 <= r1))[0]
    bw, bh = c1[drawn] - c0[drawn] + 1, r1[drawn] - r0[drawn] + 1
    small = (bw <= 8) & (bh <= 8)
    ts = drawn[small]
    for oy in range(int(bh[small].max()) if len(ts) else 0):            # the faces with small boxes together, an offset at a time
        for ox in range(int(bw[small].max())):
            sel = ts[(c0[ts] + ox <= c1[ts]) & (r0[ts] + oy <= r1[ts])]
            if len(sel):
                rasterise(sel, c0[sel] + ox, r0[sel] + oy)
    for t in drawn[~small]:                                               # the others a face at a time, its box at once
        rows, cols = np.mgrid[r0[t]:r1[t] + 1, c0[t]:c1[t] + 1]
        rasterise(np.full(rows.size, t, np.int64), cols.reshape(-1), rows.reshape(-1))

    hit = np.nonzero(keys != EMPTY)[0]
    face = np.full(P, -1, np.int32)
    depth = np.zeros(P, np.float32)
    t = (keys[hit] & np.uint64(0xffffffff)).astype(np.int64)
    face[hit] = t
    depth[hit] = (keys[hit] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    E, inside = edges(S, t, hit % W, hit // W)
    assert inside.all()
    _, q, s = depth_of(S, t, E)
    ia, ib, ic = F[t, 0], F[t, 1], F[t, 2]
    normal = rgb = None
    if normals is not False:
        normal = np.zeros((3, P), np.float32)
        if normals is True:
            N = snp.face_normals(V, F[t])
        else:
            vn = np.asarray(normals, np.float32).reshape(-1, 3)
            N = np.stack([interp(q, s, vn[ia, a], vn[ib, a], vn[ic, a]) for a in range(3)], axis=-1)
        normal[:, hit] = normalize(N.reshape(-1, 3)).T
        normal = normal.reshape(3, H, W)
    if C is not None:
        C = np.asarray(C, np.float32).reshape(-1, 3)
        rgb = np.zeros((3, P), np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            rgb[:, hit] = np.stack([interp(q, s, C[ia, a], C[ib, a], C[ic, a]).astype(np.float32) for a in range(3)])
        rgb = rgb.reshape(3, H, W)
    counts = np.bincount(S.outcome, minlength=4).astype(np.int64)
    return types.SimpleNamespace(depth=depth.reshape(1, H, W), face=face.reshape(H, W), normal=normal, rgb=rgb, counts=counts,
                                 status=ST_BAD_INDEX if S.bad_index else 0, cover=cover.reshape(H, W), setup=S)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def islands_mesh():
    """mesh_np.islands_volume extracted and welded -> (V [8704,3], F int32 [17338,3], C)"""
    tsdf, weight, rgb, origin, voxel = mnp.islands_volume(True)
    soup, colors = tnp.extract(tsdf, weight, origin, voxel, rgb)
    return frozen(*mnp.weld(soup, colors))


def island_camera(which):
    """-> (camera, H, W): camera `which` of tsdf_raycast_np.fused_volume() as it is, at its own size (40 x 48; the third 29 x 37).
    These cameras were placed for another scene and barely see the islands: camera 0 is essentially an OFF-SCREEN case (17 280
    faces drawn, 2 pixels hit), camera 3 sits among the faces and is an ALL-CLIPPED case (every face has a vertex behind it, 0
    pixels), camera 2 sees 91 pixels and clips 9 422 faces. The coverage of colours and normals is carried by
    islands_orbit_camera below and by camera 2 (tests/test_mesh_render_host.py pins these counts)."""
    _, views, _, _ = rnp.fused_volume()
    H, W = views[which].depth.shape
    return views[which].camera, H, W


ISLAND_VIEWS = (0, 3, 2)


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    tsdf, weight, rgb, origin, voxel = tnp.sphere_volume(True)
    soup, colors = tnp.extract(tsdf, weight, origin, voxel, rgb)
    return frozen(*mnp.weld(soup, colors))


def inside_sphere_camera(W=24, H=20):
    return tnp.look_at(tnp.SPHERE.centre, (19.0, -7.0, 15.0), W, H)


def pixel_camera(W, H, eye_z=-4.0, focal=4.0):
    """Looking along +z from (0, 0, eye_z) with the principal point on pixel (0, 0)'s centre: a point (x, y, 0) lands on the pixel
    (focal x / -eye_z, focal y / -eye_z), exactly when those are powers of two"""
    return types.SimpleNamespace(R=np.eye(3), T=np.array([0.0, 0.0, -eye_z]), focal_x=focal, focal_y=focal, cx=-1.0, cy=-1.0)


def square_mesh(x0=2.0, y0=3.0, side=8.0, z=0.0):
    """Two triangles over the square [x0, x0 + side] x [y0, y0 + side] at height z, the diagonal from its top-right to its
    bottom-left corner, both wound toward a camera that looks along +z"""
    V = np.array([[x0, y0, z], [x0 + side, y0, z], [x0 + side, y0 + side, z], [x0, y0 + side, z]], np.float32)
    return V, np.array([[0, 3, 1], [1, 3, 2]], np.int32)


def quad_mesh(kind="plain"):
    """The frame-filling quad for a 70 x 130 view of pixel_camera: its corners lie outside the image. kind: "plain", "guard" (one
    vertex beyond the guard band) or "behind" (one vertex behind the camera)"""
    V = np.array([[-20.0, -30.0, 0.5], [150.0, -25.0, 0.0], [170.0, 95.0, 1.0], [-15.0, 95.0, 0.25]], np.float32)
    if kind == "guard":
        V[2] = [3.0e6, 95.0, 1.0]
    if kind == "behind":
        V[2] = [170.0, 95.0, -9.0]
    C = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.5, 0.5, 0.5]], np.float32)
    return V, np.array([[0, 3, 1], [1, 3, 2]], np.int32), C


def fan_camera(W=40, H=32):
    """snp.fan_mesh seen from above its hub, the hub (0, 0, 0) exactly on pixel (20, 16)'s centre"""
    return types.SimpleNamespace(R=np.diag([1.0, -1.0, -1.0]), T=np.array([0.0, 0.0, 64.0]), focal_x=1024.0, focal_y=1024.0,
                                 cx=0.0, cy=0.0)


def field_camera(W=96, H=72):
    """snp.height_field(33, 17) from a low oblique eye close to one corner: faces from sub-pixel to tens of pixels"""
    return tnp.look_at((-3.0, -2.0, 3.5), (20.0, 10.0, 0.0), W, H)


def special_mesh():
    """mesh_np.special_soup welded (NaN vertices, signed zeros), two degenerate faces added: A == 0 by position and two equal indices"""
    V, F, _ = mnp.weld(mnp.special_soup())
    V = np.concatenate([V, np.array([[2.0, 2.0, 0.0], [3.0, 3.0, 0.0], [4.0, 4.0, 0.0]], np.float32)])
    m = len(V)
    F = np.concatenate([F, np.array([[m - 3, m - 2, m - 1], [0, 0, 1]], np.int32)])
    return V, F


def stacked_mesh():
    """Four faces over one triangle's outline: 0 and 1 coincide (the smaller index wins), 2 lies exactly behind them at twice
    the distance from pixel_camera's eye and is hidden, 3 is half of 2 moved in front of everything"""
    tri = np.array([[1.0, 1.0, 0.0], [13.0, 2.0, 0.0], [4.0, 12.0, 0.0]], np.float32)
    back = tri * np.float32(2.0) + np.array([0.0, 0.0, 4.0], np.float32)             # the same rays from (0, 0, -4)
    front = np.array([[1.0, 1.0, -1.0], [6.0, 1.5, -1.0], [2.0, 6.0, -1.0]], np.float32)
    V = np.concatenate([tri, tri, back, front])
    C = np.linspace(0.0, 1.0, V.size, dtype=np.float32).reshape(-1, 3)
    return V, np.arange(12, dtype=np.int32).reshape(4, 3)[[1, 0, 2, 3]], C


def islands_orbit_camera(W=48, H=40):
    """A camera of this module's own that sees all the islands from outside their volume"""
    return tnp.look_at((21.0, -4.0, 19.0), (10.0, 9.0, 8.0), W, H)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (V, F, C, camera, H, W, keyword arguments of render): every view the host and the GPU tests share"""
    out = {}
    V, F, C = islands_mesh()
    vn = snp.vertex_normals(V, F)
    vn.setflags(write=False)
    for which in ISLAND_VIEWS:
        cam, H, W = island_camera(which)
        out[f"islands, fused camera {which}"] = (V, F, C, cam, H, W, {})
    out["islands, orbit"] = (V, F, C, islands_orbit_camera(), 40, 48, {})
    out["islands, orbit 29 x 37"] = (V, F, C, islands_orbit_camera(37, 29), 29, 37, {"cull": "back"})
    out["islands, orbit, no colours, no normals"] = (V, F, None, islands_orbit_camera(), 40, 48, {"normals": False})
    out["islands, orbit, no colours, flat normals"] = (V, F, None, islands_orbit_camera(), 40, 48, {})
    out["islands, orbit, vertex normals"] = (V, F, C, islands_orbit_camera(), 40, 48, {"normals": vn})
    out["islands, fused camera 2, vertex normals"] = (V, F, C) + island_camera(2) + ({"normals": vn},)
    for kind in ("plain", "guard", "behind"):
        out[f"quad, {kind}"] = quad_mesh(kind) + (pixel_camera(130, 70), 70, 130, {})
    out["fan"] = snp.fan_mesh(5000) + (None, fan_camera(), 32, 40, {})
    out["height field"] = snp.height_field(33, 17) + (None, field_camera(), 72, 96, {})
    out["stacked faces"] = stacked_mesh() + (pixel_camera(16, 16), 16, 16, {})
    out["special soup"] = special_mesh() + (None, pixel_camera(16, 16), 16, 16, {})
    out["no faces"] = (np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32), None, pixel_camera(16, 16), 9, 11, {})
    Vs, Fs, Cs = sphere_mesh()
    out["sphere"] = (Vs, Fs, Cs, rnp.sphere_camera(), 20, 24, {})
    out["sphere, cull"] = (Vs, Fs, Cs, rnp.sphere_camera(), 20, 24, {"cull": "back"})
    out["sphere from inside"] = (Vs, Fs, Cs, inside_sphere_camera(), 20, 24, {})
    out["sphere from inside, cull"] = (Vs, Fs, Cs, inside_sphere_camera(), 20, 24, {"cull": "back"})
    out["sphere, near"] = (Vs, Fs, Cs, rnp.sphere_camera(), 20, 24, {"near": SPHERE_CUT})
    out["sphere, far"] = (Vs, Fs, Cs, rnp.sphere_camera(), 20, 24, {"far": SPHERE_CUT})
    out["sphere, far through the near cap"] = (Vs, Fs, Cs, rnp.sphere_camera(), 20, 24, {"far": SPHERE_CAP_FAR})
    out["sphere from inside, near and far"] = (Vs, Fs, Cs, inside_sphere_camera(), 20, 24, {"near": 1.0, "far": SPHERE_INSIDE_FAR})
    out["stacked faces, far behind the front face"] = stacked_mesh() + (pixel_camera(16, 16), 16, 16, {"far": 3.5})
    out["stacked faces, far on the coincident faces"] = stacked_mesh() + (pixel_camera(16, 16), 16, 16, {"far": 4.0})
    out["square"] = square_mesh() + (None, pixel_camera(16, 16), 16, 16, {})
    return out


# the depth of the sphere's centre along sphere_camera's forward axis: near = this draws the far half, far = this the near half
# (from outside every visible pixel is nearer than the centre, so far = SPHERE_CUT alone removes nothing: the two below do)
SPHERE_CUT = float(np.linalg.norm(np.asarray(tnp.SPHERE.centre) - np.array([19.0, -7.0, 15.0])))


# between the sphere's near pole (centre depth - radius = 16.1) and its silhouette (19.4): the middle of the cap disappears
SPHERE_CAP_FAR = SPHERE_CUT - 0.6 * tnp.SPHERE.radius
# from the centre every face is about one radius away, nearer along the forward axis toward the image's corners
SPHERE_INSIDE_FAR = 0.9 * tnp.SPHERE.radius


@functools.lru_cache(maxsize=None)
def rendered(name):
    """render() of scenes()[name], computed once and read-only"""
    V, F, C, cam, H, W, kw = scenes()[name]
    r = render(V, F, C, cam, H, W, **kw)
    frozen(r.depth, r.face, r.normal, r.rgb, r.counts, r.cover)
    return r
