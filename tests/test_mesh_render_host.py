"""Host tests of Mesh.render: the host build of csrc/mesh_raster_math.h against the numpy restatement tests/mesh_render_np.py byte
for byte, the per-element functions at their edges, the restatement against independent spellings (coverage in Fractions, the hit
point against the unsnapped triangle, brute-force ray casting), the top-left rule on shared edges and vertices, and the refusals of
the wrapper and of the library. No GPU: every refusal is made before any GPU work.

The two tolerances here are derived, not measured. With e = 1/512 pixel, the most a coordinate moves when it is snapped:

  HIT POINT. The rendered depth is the exact perspective interpolation over the SNAPPED triangle, whose corners V'_i are the true
  corners V_i moved sideways by at most e z_i / |focal| per image axis at unchanged depth. A point inside the snapped triangle is
  sum b_i V'_i with weights that sum to 1, so it lies within max_i |V'_i - V_i| <= sqrt(2) e max z / min |focal| of the point
  sum b_i V_i of the true triangle. The float32 rounding of the depth moves the hit point along its ray by at most 2^-24 depth |ray|.
  The distance from the unprojected hit point to the true triangle is held to the sum of the two, times 1.01 for the float64
  roundings of the test itself.

  BRUTE FORCE. On the plane of a face 1 / z is affine in the pixel coordinates, 1 / z = a . p + b. The snapped plane takes the
  true corner depths at corners moved by e_i, |e_i|_inf <= e, so g = 1 / z' - 1 / z is affine and equals -a . e_i at the snapped
  corners: |g| <= e (|a_x| + |a_y|) there and therefore inside the snapped triangle. Hence |z' - z| <= z z' e (|a_x| + |a_y|),
  plus 2^-24 z' for the float32 rounding, as long as the pixel is covered by the same face before and after the snap. A pixel
  whose centre lies within sqrt(2) e of a projected edge of ANY face may change faces and is excluded: that is a band of
  0.0055 pixels around the edges, a share of a few per cent of the hit pixels at most; the test caps it at 25 %."""
import ctypes as C
import fractions
import os
import re

import numpy as np
import pytest
import torch

import consistency_np as cnp
import mesh_render_hostcheck as hc
import mesh_render_np as mr
import tsdf_raycast_np as rnp
from sfgs import _lib as L

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
E_ARG = -1
ENTRY_POINTS = ("sfgs_mesh_render_scratch_bytes", "sfgs_mesh_render")
SNAP_E = 1.0 / 512.0


def same(got, want, what):
    assert (got is None) == (want is None), what
    if got is not None:
        assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
        assert got.tobytes() == want.tobytes(), (what, int((got.view(np.uint32) != want.view(np.uint32)).sum()) if got.itemsize == 4 else "")


# ---- the host build of mesh_raster_math.h against the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(mr.scenes()))
def test_host_build_renders_byte_for_byte(name):
    V, F, Cc, cam, H, W, kw = mr.scenes()[name]
    want = mr.rendered(name)
    got = hc.render(V, F, Cc, cam, H, W, **kw)
    for field in ("depth", "face", "normal", "rgb", "counts", "cover"):
        same(getattr(got, field), getattr(want, field), (name, field))
    assert got.status == want.status == 0
    assert int(want.counts.sum()) == len(F)
    assert ((want.depth[0] == 0) == (want.face == -1)).all()
    for plane in (want.normal, want.rgb):
        assert plane is None or not plane[:, want.depth[0] == 0].any()


def test_the_fixtures_are_what_the_tests_count_on():
    V, F, _ = mr.islands_mesh()
    assert (len(V), len(F)) == (8704, 17338)
    hits = {name: int((mr.rendered(name).depth > 0).sum()) for name in mr.scenes()}
    assert hits["islands, orbit"] > 500 and hits["islands, fused camera 2"] > 50 and hits["quad, plain"] == 70 * 130
    assert hits["no faces"] == 0 and hits["sphere from inside"] == 20 * 24 and hits["sphere from inside, cull"] == 0
    # the fused cameras were placed for another scene: camera 0 is an off-screen case, camera 3 an all-clipped one
    assert hits["islands, fused camera 0"] == 2 and mr.rendered("islands, fused camera 0").counts.tolist() == [17280, 0, 0, 58]
    assert mr.rendered("islands, fused camera 3").counts.tolist() == [0, 0, len(F), 0] and hits["islands, fused camera 3"] == 0
    assert hits["islands, fused camera 2"] == 91 and mr.rendered("islands, fused camera 2").counts[2] == 9422
    assert mr.rendered("quad, guard").counts.tolist() == [1, 0, 1, 0] == mr.rendered("quad, behind").counts.tolist()
    assert 0 < hits["quad, behind"] < 70 * 130
    assert mr.rendered("special soup").counts.tolist() == [2, 0, 3, 3]
    field = mr.rendered("height field")
    S = field.setup
    c0, c1, r0, r1 = mr.boxes(S, 72, 96)
    px = ((c1 - c0 + 1) * (r1 - r0 + 1))[(S.outcome == 0) & (c0 <= c1) & (r0 <= r1)]
    assert px.min() <= 4 and px.max() > mr.SMALL_MAX_DEFAULT and (px <= mr.SMALL_MAX_DEFAULT).any()    # both routes in one frame
    fan = mr.rendered("fan")
    assert fan.counts[0] == 5000 and fan.cover.max() == 1                   # 5000 faces meet on pixel (20, 16), none twice
    st = mr.rendered("stacked faces")
    assert set(np.unique(st.face)) == {-1, 0, 3} and st.cover.max() == 4     # the smaller of two coincident faces, never the hidden one


def test_culling_the_sphere_pins_the_sign_of_the_area():
    a, b = mr.rendered("sphere"), mr.rendered("sphere, cull")
    for field in ("depth", "face", "normal", "rgb"):
        same(getattr(b, field), getattr(a, field), field)                   # from outside only faces turned toward the camera are seen
    n = int(a.counts.sum())
    assert 0.35 * n < b.counts[1] < 0.65 * n and b.counts[0] + b.counts[1] == a.counts[0]
    inside, culled = mr.rendered("sphere from inside"), mr.rendered("sphere from inside, cull")
    assert culled.counts[0] == 0 and culled.counts[1] == inside.counts[0] > 0 and not culled.depth.any()
    # the flat normal of every pixel seen from outside points away from the sphere's centre: extract's winding is outward
    V, F, _, cam, H, W, _ = mr.scenes()["sphere"]
    k = cnp.constants(cam, H, W)
    hit = a.depth[0] > 0
    rows, cols = np.nonzero(hit)
    p = cnp.unproject_pixels(k, rows, cols, a.depth[0][hit])
    outward = p - np.asarray(mr.tnp.SPHERE.centre)
    assert (np.einsum("ij,ij->i", a.normal[:, hit].T.astype(np.float64), outward) > 0).all()
    near, far = mr.rendered("sphere, near"), mr.rendered("sphere, far")
    assert 0 < near.counts[2] < n and (near.depth[near.depth > 0] > mr.SPHERE_CUT).all() and (far.depth <= mr.SPHERE_CUT).all()
    assert (near.depth > 0).sum() > 20 and (far.depth > 0).sum() > 20


def test_far_removes_pixels_that_would_have_won():
    """far is observed: a pixel whose nearest face lies deeper than far is EMPTY, and a depth equal to far is kept"""
    whole, cut = mr.rendered("sphere"), mr.rendered("sphere, far through the near cap")
    assert whole.depth.max() > mr.SPHERE_CAP_FAR > whole.depth[whole.depth > 0].min()        # far lies inside the visible depths
    gone = (whole.depth[0] > 0) & (cut.depth[0] == 0)
    assert gone.sum() >= 10 and (whole.depth[0][gone] > mr.SPHERE_CAP_FAR).all()
    stay = cut.depth[0] > 0
    assert stay.sum() >= 40 and (cut.depth[0][stay] <= mr.SPHERE_CAP_FAR).all()
    for field in ("depth", "face", "normal", "rgb"):                                           # what stays is unchanged, what goes is zeros
        a, b = getattr(whole, field), getattr(cut, field)
        a, b = (a, b) if a.ndim == 3 else (a[None], b[None])
        assert (a[:, stay] == b[:, stay]).all()
        assert (b[:, gone] == (-1 if field == "face" else 0)).all()
    assert cut.counts.tolist() == whole.counts.tolist() and np.array_equal(cut.cover, whole.cover)   # far is a test per pixel, not per face
    same(mr.rendered("sphere, far").depth, whole.depth, "far behind everything visible changes nothing")
    inside, both = mr.rendered("sphere from inside"), mr.rendered("sphere from inside, near and far")
    assert 0 < (both.depth > 0).sum() < (inside.depth > 0).sum() and both.depth.max() <= mr.SPHERE_INSIDE_FAR < inside.depth.max()
    assert both.counts[2] > inside.counts[2]                                                   # near = 1 clips more faces as well
    st, front, on = (mr.rendered(n) for n in ("stacked faces", "stacked faces, far behind the front face",
                                              "stacked faces, far on the coincident faces"))
    assert set(np.unique(st.face)) == {-1, 0, 3} and set(np.unique(front.face)) == {-1, 3}     # faces 0 / 1 at depth 4 are beyond far = 3.5
    assert ((st.face == 0) == ((front.face == -1) & (st.face != -1))).all() and ((st.face == 3) == (front.face == 3)).all()
    assert float(st.depth[0][st.face == 0].max()) == 4.0
    for field in ("depth", "face", "normal", "rgb"):
        same(getattr(on, field), getattr(st, field), f"{field}: a depth equal to far is kept")


# ---- the per-element functions at their edges ------------------------------------------------------------------------------------
def exact_camera(focal=4.0):
    """u = focal x / 4 and v = focal y / 4 exactly for points at z = 0"""
    return cnp.constants(mr.pixel_camera(16, 16, focal=focal), 16, 16)


def test_vertex_records_at_their_edges():
    k = exact_camera()
    for x, want in ((0.5 / 256, 0), (1.5 / 256, 2), (2.5 / 256, 2), (-0.5 / 256, 0), (-1.5 / 256, -2), (3.25 / 256, 3), (7.0, 1792)):
        ok, X, Y, z = hc.project(k, (x, -x, 0.0))
        assert ok and (X, Y, z) == (want, -want, 4.0), (x, X, Y, z)                           # rint: ties to even
        Xn, Yn, zn, okn = mr.project_vertices(np.array([[x, -x, 0.0]], np.float32), k)
        assert okn[0] and (int(Xn[0]), int(Yn[0]), float(zn[0])) == (X, Y, z)
    for snapped, usable in ((1 << 28, True), ((1 << 28) + 1, False), (-(1 << 28), True), (-(1 << 28) - 1, False)):
        kk = exact_camera(focal=snapped / 64.0)                                               # 256 u = snapped for x = 1
        for p in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)):
            ok, X, Y, _ = hc.project(kk, p)
            assert ok == usable == bool(mr.project_vertices(np.array([p], np.float32), kk)[3][0]), (snapped, p)
            assert not ok or snapped in (X, Y)
    p = (1.0, 2.0, 0.0)                                                                       # depth 4 exactly
    for near, usable in ((4.0, False), (np.nextafter(4.0, 0.0), True), (np.nextafter(4.0, 9.0), False), (0.0, True)):
        assert hc.project(k, p, near)[0] == usable == bool(mr.project_vertices(np.array([p], np.float32), k, near)[3][0]), near
    for bad in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -4.0), (0.0, 0.0, -5.0), (3e38, 0.0, 0.0)):
        assert not hc.project(k, bad)[0] and not mr.project_vertices(np.array([bad], np.float32), k)[3][0], bad
    assert hc.camera_sign(k) == mr.camera_sign(k) == 1
    flipped = cnp.constants(mr.pixel_camera(16, 16, focal=-4.0), 16, 16)
    flipped.focal_y = 4.0
    assert hc.camera_sign(flipped) == mr.camera_sign(flipped) == -1


def test_face_set_up_at_its_edges():
    tri = [(0, 0), (2560, 0), (0, 2560)]                                                      # As > 0: turned away under camera sign +1
    assert hc.face(tri) == (mr.COUNTS.index("drawn"), 2560 * 2560, 1)
    assert hc.face(tri, cull=True)[0] == mr.COUNTS.index("culled") and hc.face(tri, camera_sign=-1, cull=True)[0] == 0
    assert hc.face(tri[::-1]) == (0, 2560 * 2560, -1) and hc.face(tri[::-1], cull=True)[0] == 0
    for flat in ([(0, 0), (256, 256), (512, 512)], [(5, 5), (5, 5), (9, 70)], [(1, 1), (1, 1), (1, 1)]):
        assert hc.face(flat)[0] == hc.face(flat, cull=True)[0] == mr.COUNTS.index("degenerate")
    big = 1 << 28
    assert hc.face([(-big, -big), (big, -big), (-big, big)]) == (0, 4 * big * big, 1)         # 2^58: inside int64


def test_an_edge_value_of_zero_belongs_to_one_direction_only():
    # the edge from (0, 0) to (10, 10) pixels through the centres (k, k), as the side of the face below it and of the face above
    lower, upper = [(0, 0), (2560, 2560), (0, 2560)], [(0, 0), (2560, 0), (2560, 2560)]
    for k in range(1, 10):
        got = [hc.covers(xy, k, k) for xy in (lower, upper)]
        zero = [int(np.nonzero(E == 0)[0][0]) for _, E, _ in got]
        assert [int((E == 0).sum()) for _, E, _ in got] == [1, 1]
        assert got[0][2][zero[0]] != got[1][2][zero[1]]                                       # opposite directions, opposite answers
        assert got[0][0] != got[1][0] and got[0][0] == bool(got[0][2][zero[0]])
    for xy in (lower, upper, lower[::-1], upper[::-1]):                                        # either winding: the same pixels
        assert hc.covers(xy, 3, 3)[0] == hc.covers(xy[::-1], 3, 3)[0]
    # left and top edges own their zeros, right and bottom edges do not
    box = [(256, 256), (256 * 9, 256), (256, 256 * 9)]
    assert hc.covers(box, 1, 4)[0] and hc.covers(box, 4, 1)[0] and hc.covers(box, 1, 1)[0] and not hc.covers(box, 5, 5)[0]


# ---- the restatement against independent spellings -------------------------------------------------------------------------------
def fraction_cover(S, H, W):
    """How many drawn faces cover each pixel centre, by exact rational arithmetic on the snapped corners and a geometric spelling
    of the rule: strictly inside, or on an edge that is a LEFT edge (the face lies to its right) or a TOP edge (horizontal, the
    face below it)"""
    Fr = fractions.Fraction
    cover = np.zeros((H, W), np.int32)
    for t in np.nonzero(S.outcome == 0)[0]:
        P = [(Fr(int(S.X[t, i]), 256), Fr(int(S.Y[t, i]), 256)) for i in range(3)]
        for row in range(H):
            for col in range(W):
                inside = True
                for i in range(3):
                    (px, py), (qx, qy), (rx, ry) = P[i], P[(i + 1) % 3], P[(i + 2) % 3]
                    side = (qx - px) * (ry - py) - (qy - py) * (rx - px)                  # where the third corner lies
                    here = (qx - px) * (row - py) - (qy - py) * (col - px)
                    if here == 0:
                        if py == qy:
                            owns = ry > py                                                # horizontal: a top edge has the face below
                        else:
                            owns = rx > px + (qx - px) * (ry - py) / (qy - py)            # the face lies to the right of the edge
                        inside = inside and owns
                    else:
                        inside = inside and (here > 0) == (side > 0)
                cover[row, col] += inside
    return cover


@pytest.mark.parametrize("name", ("square", "stacked faces", "special soup"))
def test_coverage_equals_exact_rational_arithmetic(name):
    V, F, _, cam, H, W, kw = mr.scenes()[name]
    want = mr.rendered(name)
    assert np.array_equal(fraction_cover(want.setup, H, W), want.cover), name
    rng = np.random.default_rng(11)                                                           # ... and random faces on the half-pixel lattice
    Vr = np.concatenate([rng.integers(0, 33, (60, 2)) / 2.0, np.zeros((60, 1))], axis=1).astype(np.float32)
    Fr = rng.integers(0, 60, (40, 3)).astype(np.int32)
    r = mr.render(Vr, Fr, None, mr.pixel_camera(16, 16), 16, 16)
    assert np.array_equal(fraction_cover(r.setup, 16, 16), r.cover) and r.cover.max() > 3


def closest_point_on_triangle(p, a, b, c):
    """Ericson, Real-Time Collision Detection 5.1.5"""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return a
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return b
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return a + ab * (d1 / (d1 - d3))
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return c
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return a + ac * (d2 / (d2 - d6))
    va = d3 * d6 - d5 * d4
    if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        return b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))
    denom = 1.0 / (va + vb + vc)
    return a + ab * (vb * denom) + ac * (vc * denom)


@pytest.mark.parametrize("name", ("islands, orbit", "islands, fused camera 2", "height field", "quad, plain", "sphere from inside"))
def test_every_hit_point_lies_on_its_face(name):
    V, F, _, cam, H, W, kw = mr.scenes()[name]
    r = mr.rendered(name)
    k = cnp.constants(cam, H, W)
    rows, cols = np.nonzero(r.depth[0] > 0)
    assert len(rows) > 50
    d = r.depth[0][rows, cols]
    points = cnp.unproject_pixels(k, rows, cols, d)
    ray = np.linalg.norm(cnp.unproject_pixels(k, rows, cols, np.ones_like(d)) - k.c, axis=1)
    Vd = V.astype(np.float64)
    worst = 0.0
    for p, t, depth, length in zip(points, r.face[rows, cols], d.astype(np.float64), ray):
        a, b, c = Vd[F[t, 0]], Vd[F[t, 1]], Vd[F[t, 2]]
        zmax = max(float(z) for z in r.setup.z[t])
        bound = 1.01 * (np.sqrt(2.0) * SNAP_E * zmax / min(abs(k.focal_x), abs(k.focal_y)) + 2.0 ** -24 * depth * length)
        dist = float(np.linalg.norm(p - closest_point_on_triangle(p, a, b, c)))
        worst = max(worst, dist / bound)
        assert dist <= bound, (name, int(t), dist, bound)
    assert worst > 0.0


def brute_force_depth(V, F, k, H, W):
    """float64 [H,W] depth of the nearest face along every pixel's ray (Moeller-Trumbore over all faces, both sides), 0 = none;
    and the face"""
    Vd = V.astype(np.float64)
    a, e1, e2 = Vd[F[:, 0]], Vd[F[:, 1]] - Vd[F[:, 0]], Vd[F[:, 2]] - Vd[F[:, 0]]
    depth, face = np.zeros((H, W)), np.full((H, W), -1)
    for row in range(H):
        for col in range(W):
            x, y = (col - k.cx_pix) / k.focal_x, (row - k.cy_pix) / k.focal_y
            d = x * k.M[0] + y * k.M[1] + k.M[2]
            h = np.cross(d, e2)
            det = np.einsum("ij,ij->i", e1, h)
            with np.errstate(divide="ignore", invalid="ignore"):
                s = k.c - a
                u = np.einsum("ij,ij->i", s, h) / det
                q = np.cross(s, e1)
                v = (q @ d) / det
                t = np.einsum("ij,ij->i", e2, q) / det
                ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
            if ok.any():
                best = np.nonzero(ok)[0][np.argmin(t[ok])]
                depth[row, col], face[row, col] = t[best], best
    return depth, face


def test_brute_force_ray_casting_agrees_on_the_sphere():
    V, F, _, cam, H, W, _ = mr.scenes()["sphere"]
    r = mr.rendered("sphere")
    k = cnp.constants(cam, H, W)
    depth, face = brute_force_depth(V, F, k, H, W)
    # the projected corners, unsnapped, and every pixel centre's distance to every edge of every face
    u, v, z = cnp.project(k, V.astype(np.float64))
    pu, pv = u[F], v[F]                                                                       # [n,3]
    rows, cols = np.mgrid[0:H, 0:W]
    near_edge = np.zeros((H, W), bool)
    for i in range(3):
        ax, ay, bx, by = pu[:, i], pv[:, i], pu[:, (i + 1) % 3], pv[:, (i + 1) % 3]
        ex, ey = bx - ax, by - ay
        ll = np.maximum(ex * ex + ey * ey, 1e-300)
        for row in range(H):
            tt = np.clip(((cols[row][:, None] - ax) * ex + (row - ay) * ey) / ll, 0.0, 1.0)
            dist = np.hypot(cols[row][:, None] - (ax + tt * ex), row - (ay + tt * ey))
            near_edge[row] |= (dist <= np.sqrt(2.0) * SNAP_E).any(axis=1)
    hit = (depth > 0) | (r.depth[0] > 0)
    assert hit.sum() > 60
    share = (near_edge & hit).sum() / hit.sum()
    assert share <= 0.25, share                                                               # (it is 0: no centre lies that close to an edge)
    keep = hit & ~near_edge
    assert ((depth > 0) == (r.depth[0] > 0))[keep].all()
    assert (face == r.face)[keep].all()
    for row, col in zip(*np.nonzero(keep)):
        t = face[row, col]
        # 1 / z = a . p + b over the face's true projection
        A = np.stack([pu[t], pv[t], np.ones(3)], axis=1)
        ax, ay, _ = np.linalg.solve(A, 1.0 / z[F[t]])
        zt, zr = depth[row, col], float(r.depth[0, row, col])
        bound = 1.01 * (zt * zr * SNAP_E * (abs(ax) + abs(ay)) + 2.0 ** -24 * zr)
        assert abs(zt - zr) <= bound, (row, col, zt, zr, bound)


# ---- shared edges and vertices ---------------------------------------------------------------------------------------------------
def test_a_shared_edge_and_a_shared_vertex_belong_to_one_face():
    V, F, _, cam, H, W, _ = mr.scenes()["square"]
    r = mr.rendered("square")
    k = cnp.constants(cam, H, W)
    X, Y, _, ok = mr.project_vertices(V, k)
    assert ok.all() and not (X % 256).any() and not (Y % 256).any()                           # the corners sit on pixel centres
    c0, c1, r0, r1 = int(X.min()) // 256, int(X.max()) // 256, int(Y.min()) // 256, int(Y.max()) // 256
    assert (c1 - c0, r1 - r0) == (8, 8)
    want = np.zeros((H, W), np.int32)
    want[r0:r1, c0:c1] = 1                                                                    # the top and left sides in, the bottom and right sides out
    assert np.array_equal(r.cover, want)
    on_diagonal = [(r0 + 8 - j, c0 + j) for j in range(1, 8)]                                 # ... through pixel centres, each counted once
    assert all(r.cover[p] == 1 for p in on_diagonal)
    assert {int(r.face[p]) for p in on_diagonal} == {1} and r.face[r0, c0] == 0 and r.face[r1 - 1, c1 - 1] == 1
    fan = mr.rendered("fan")
    S = fan.setup
    hub = np.nonzero((S.X == 20 * 256) & (S.Y == 16 * 256))
    assert len(hub[0]) == 5000                                                                # every face has the hub, on pixel (20, 16)'s centre
    assert fan.cover[16, 20] <= 1 and fan.cover.max() == 1
    # a closed fan around a pixel centre covers it exactly once
    ang = np.linspace(0.0, 2 * np.pi, 8)[:-1]
    Vc = np.concatenate([[[5.0, 5.0, 0.0]], np.stack([5 + 3 * np.cos(ang), 5 + 3 * np.sin(ang), 0 * ang], axis=1)]).astype(np.float32)
    Fc = np.array([[0, 1 + j, 1 + (j + 1) % 7] for j in range(7)], np.int32)
    closed = mr.render(Vc, Fc, None, mr.pixel_camera(16, 16), 16, 16)
    assert closed.cover[5, 5] == 1 and closed.cover.max() == 1


# ---- header, library, binding, refusals ------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfgs.h"
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    assert int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == lib.sfgs_abi_version() == 28
    fields = [f for f, _ in L.SfgsMeshRender._fields_]
    body = re.search(r"typedef struct SfgsMeshRender \{(.*?)\} SfgsMeshRender;", hdr, re.S).group(1)
    declared = re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert declared == fields
    import subprocess
    prints = "\n".join(f'  printf("{f} %zu\\n", offsetof(SfgsMeshRender, {f}));' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {{\n'
                   f'  printf("sizeof %zu\\n", sizeof(SfgsMeshRender));\n{prints}\n  return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SfgsMeshRender)
    for f in fields:
        assert int(out[f]) == getattr(L.SfgsMeshRender, f).offset, f
    math_h = open(os.path.join(ROOT, "skyfall-gs_amd", "csrc", "mesh_raster_math.h")).read()
    assert re.search(r"MR_DRAWN = 0, MR_CULLED = 1, MR_CLIPPED = 2, MR_DEGENERATE = 3", math_h)
    assert mr.COUNTS == ("drawn", "culled", "clipped", "degenerate")
    raster = open(os.path.join(ROOT, "skyfall-gs_amd", "csrc", "mesh_raster.hip")).read()
    assert int(re.search(r"MR_SMALL_MAX_DEFAULT = (\d+)", raster).group(1)) == mr.SMALL_MAX_DEFAULT


def test_the_library_refuses_bad_arguments_before_any_gpu_work():
    lib = L.load()
    dummy = (C.c_double * 8)()
    p = C.cast(dummy, C.c_void_p).value                   # never dereferenced: every call below is refused first
    big = 1 << 40

    def refused(rc, what):
        assert rc == E_ARG, what
        assert lib.sfgs_last_error(), what

    sb = lib.sfgs_mesh_render_scratch_bytes
    assert sb(-1, 5, 4, 4) == 0 and sb(5, -1, 4, 4) == 0 and sb(1 << 31, 5, 4, 4) == 0 and sb(5, (1 << 29) + 1, 4, 4) == 0
    assert sb(0, 5, 4, 4) == 0 and sb(5, 5, 0, 4) == 0 and sb(5, 5, 4, -1) == 0 and sb(5, 5, 1 << 15, (1 << 15) + 1) == 0
    assert sb(1000, 2000, 30, 50) >= 16 * 1000 + 16 * 2000 + 8 * 30 * 50 and sb(0, 0, 3, 3) > 0
    eye = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)

    def args(**kw):
        a = L.SfgsMeshRender(C.sizeof(L.SfgsMeshRender), 6, 8, 0, eye, (C.c_double * 3)(), 4.0, 3.0, 10.0, 10.0, 0.0, float("inf"), 5, 5, -1,
                             p, None, p, None, p, p, None, None, p)
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    def render_with(scratch=p, nbytes=big, **kw):
        return lib.sfgs_mesh_render(C.byref(args(**kw)), scratch, nbytes, None)

    nan, inf = float("nan"), float("inf")
    for kw in ({"struct_size": 8}, {"H": 0}, {"W": -1}, {"H": 1 << 15, "W": (1 << 15) + 1}, {"m": -1}, {"n": -1}, {"m": 0}, {"m": 1 << 31},
               {"n": (1 << 29) + 1}, {"cull": 2}, {"cull": -1}, {"cx_pix": nan}, {"cy_pix": inf}, {"focal_x": 0.0}, {"focal_y": nan},
               {"focal_x": inf}, {"near": -1.0}, {"near": inf}, {"near": nan}, {"near": 2.0, "far": 2.0}, {"far": nan}, {"small_max": -2},
               {"small_max": (1 << 30) + 1}, {"vertices": None}, {"faces": None}, {"depth": None}, {"face": None}, {"state": None},
               {"colors": p}, {"rgb": p}, {"vertex_normals": p}, {"M": (C.c_double * 9)(nan, 0, 0, 0, 1, 0, 0, 0, 1)},
               {"c": (C.c_double * 3)(0, inf, 0)}):
        refused(render_with(**kw), kw)
    refused(lib.sfgs_mesh_render(None, p, big, None), "NULL arguments")
    refused(render_with(scratch=None), "NULL scratch")
    refused(render_with(nbytes=16), "scratch too small")
    assert b"scratch too small" in lib.sfgs_last_error()


def cpu_mesh(V, F, Cc=None):
    from sfgs.mesh import Mesh
    return Mesh._made(torch.from_numpy(np.array(V)), torch.from_numpy(np.array(F)), None if Cc is None else torch.from_numpy(np.array(Cc)),
                      torch.tensor([len(V), len(F), 0, 0]), "test")


def test_wrong_arguments_raise_value_error_without_a_gpu():
    from sfgs.mesh import MeshView
    V, F, Cc = mr.sphere_mesh()
    mesh, cam = cpu_mesh(V, F, Cc), rnp.sphere_camera()
    view = MeshView(torch.zeros((1, 20, 24)), torch.zeros((20, 24), dtype=torch.int32), torch.zeros((3, 20, 24)), torch.zeros((3, 20, 24)),
                    torch.zeros(8, dtype=torch.int64))
    for kw, match in (({"height": 0}, "height"), ({"height": 2.0}, "height"), ({"width": True}, "width"), ({"height": 1 << 16, "width": 1 << 15}, "2\\^30"),
                      ({"near": -1.0}, "near"), ({"near": float("nan")}, "near"), ({"near": 2.0, "far": 2.0}, "far"), ({"far": 0.0}, "far"),
                      ({"cull": "front"}, "cull"), ({"cull": True}, "cull"), ({"normals": 1}, "normals"), ({"normals": None}, "normals"),
                      ({"normals": torch.zeros((len(V), 2))}, "normals"), ({"normals": torch.zeros((len(V), 3), dtype=torch.float64)}, "normals"),
                      ({"normals": torch.zeros((len(V), 3))}, "GPU"), ({"_small_max": -1}, "_small_max"), ({"_small_max": 1.5}, "_small_max"),
                      ({"out": object()}, "MeshView"), ({"out": view, "normals": False}, "other normals"), ({"out": view, "height": 21}, "out.depth"),
                      ({"out": view}, "GPU"), ({}, "GPU")):
        a = {"height": 20, "width": 24}
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            mesh.render(cam, **a)
    with pytest.raises(ValueError, match="other normals"):
        cpu_mesh(V, F).render(cam, 20, 24, out=view)                                          # a mesh without colours, a view with rgb
    with pytest.raises(ValueError, match="camera"):
        mesh.render(object(), 20, 24)
    # check(): ONE read, the counts, and a status raises
    state = torch.tensor([5, 1, 2, 3, 0, 0, 0, 0])
    assert MeshView(None, None, None, None, state).check() == (5, 1, 2, 3)
    assert MeshView(None, None, None, None, state).counts.tolist() == [5, 1, 2, 3]
    with pytest.raises(ValueError, match="face index"):
        MeshView(None, None, None, None, torch.tensor([5, 1, 2, 3, 8, 0, 0, 0])).check()
    with pytest.raises(RuntimeError, match="trip bound"):                                     # status bit 0: a list of larger faces ran over
        MeshView(None, None, None, None, torch.tensor([5, 1, 2, 3, 1, 0, 0, 0])).check()
