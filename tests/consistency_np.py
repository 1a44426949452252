"""The multi-view depth consistency check of sfgs.consistency (csrc/consistency.hip; include/sfgs.h states the pair test)
restated in vectorised numpy, float64 throughout -- what the kernel is held to byte for byte -- and the scenes its tests share.
Every product is spelled elementwise (no `@` on per-pixel data), in the order the kernel takes it; the camera constants are
formed as sfgs.geometry._check_view(..., centre_from_view=True) forms them for the point cloud (tests/geometry_np.unproject's
way), with no origin.

  constants / unproject_pixels / project     the two maps between a view's pixels and the world
  check                                      view i against all the others -> (count, keep), with the branch counts on the side
  masks                                      keep of every view
  blur3                                      the stand-in for a splatting depth map's blend at a depth edge"""
import collections
import types

import numpy as np

import geometry_np as gnp

View = collections.namedtuple("View", "depth camera mask")        # depth float32 [H,W]; mask None or bool / uint8 [H,W]
BRANCHES = ("behind_or_outside", "source_unused", "depth_failed", "round_trip_failed", "accepted")


def constants(camera, H, W):
    """-> namespace M [3,3] (world = cam @ M + c), c [3], cx_pix, cy_pix, focal_x, focal_y, H, W"""
    M = np.asarray(camera.R, dtype=np.float64).T
    c = -M @ np.asarray(camera.T, dtype=np.float64)
    return types.SimpleNamespace(M=M, c=c, cx_pix=gnp.pixel_centre(float(getattr(camera, "cx", 0.0)), W),
                                 cy_pix=gnp.pixel_centre(float(getattr(camera, "cy", 0.0)), H), focal_x=float(camera.focal_x),
                                 focal_y=float(camera.focal_y), H=H, W=W)


def used_pixels(depth, mask):
    with np.errstate(invalid="ignore"):
        ok = (depth > 0) & (depth < np.inf)
    return ok if mask is None else ok & (np.asarray(mask).reshape(depth.shape) != 0)


def unproject_pixels(k, row, col, d):
    """float64 world points [n,3] of the pixels (row, col) (integer arrays) at float32 depths d: geometry_np.unproject's
    sequence on explicit pixels"""
    z = d.astype(np.float64)
    x = (col.astype(np.float64) - k.cx_pix) * z / k.focal_x
    y = (row.astype(np.float64) - k.cy_pix) * z / k.focal_y
    return np.stack([((x * k.M[0, j] + y * k.M[1, j]) + z * k.M[2, j]) + k.c[j] for j in range(3)], axis=-1)


def project(k, w):
    """world points [n,3] -> (u, v, z): columns, rows, depth along the forward axis. z is not tested here."""
    q0, q1, q2 = w[:, 0] - k.c[0], w[:, 1] - k.c[1], w[:, 2] - k.c[2]
    cam = [(q0 * k.M[a, 0] + q1 * k.M[a, 1]) + q2 * k.M[a, 2] for a in range(3)]
    z = cam[2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = cam[0] * k.focal_x / z + k.cx_pix
        v = cam[1] * k.focal_y / z + k.cy_pix
    return u, v, z


def check(views, i, rel_tol=0.01, px_tol=1.0, min_views=2, branches=None):
    """-> (count uint8 [H_i,W_i], keep uint8 [H_i,W_i]). branches: a dict that receives the number of (pixel, source) pairs that
    left at each test, under the names of BRANCHES."""
    rel_tol, px_tol2 = np.float64(rel_tol), np.float64(px_tol) * np.float64(px_tol)
    K = [constants(v.camera, *v.depth.shape) for v in views]
    ref, kr = views[i], K[i]
    H, W = ref.depth.shape
    row, col = np.nonzero(used_pixels(ref.depth, ref.mask))
    w = unproject_pixels(kr, row, col, ref.depth[row, col])
    n = np.zeros(len(row), dtype=np.int64)
    left = dict.fromkeys(BRANCHES, 0)
    for j, (src, ks) in enumerate(zip(views, K)):
        if j == i:
            continue
        alive = np.arange(len(row))
        u, v, z = project(ks, w)
        with np.errstate(invalid="ignore"):
            fu, fv = np.floor(u + 0.5), np.floor(v + 0.5)
            ok = (z > 0) & (fu >= 0) & (fu < ks.W) & (fv >= 0) & (fv < ks.H)
        left["behind_or_outside"] += int((~ok).sum())
        alive, z, su, sv = alive[ok], z[ok], fu[ok].astype(np.int64), fv[ok].astype(np.int64)
        ok = used_pixels(src.depth, src.mask)[sv, su]
        left["source_unused"] += int((~ok).sum())
        alive, z, su, sv = alive[ok], z[ok], su[ok], sv[ok]
        dj = src.depth[sv, su]
        ok = np.abs(dj.astype(np.float64) - z) <= rel_tol * z
        left["depth_failed"] += int((~ok).sum())
        alive, su, sv, dj = alive[ok], su[ok], sv[ok], dj[ok]
        u2, v2, z2 = project(kr, unproject_pixels(ks, sv, su, dj))
        du, dv = u2 - col[alive].astype(np.float64), v2 - row[alive].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            ok = (z2 > 0) & (du * du + dv * dv <= px_tol2)
        left["round_trip_failed"] += int((~ok).sum())
        left["accepted"] += int(ok.sum())
        n[alive[ok]] += 1
    if branches is not None:
        branches.update(left)
    count = np.zeros((H, W), dtype=np.uint8)
    count[row, col] = n
    return count, (count >= min_views).astype(np.uint8)


def masks(views, rel_tol=0.01, px_tol=1.0, min_views=2):
    return [check(views, i, rel_tol, px_tol, min_views)[1] for i in range(len(views))]


def blur3(depth):
    """float32 [H,W] -> float32 [H,W]: the 3 x 3 box mean (edge-padded, float64, the nine terms added row by row), 0 where the
    depth was 0 -- roughly what alpha blending does to a depth edge"""
    depth = np.asarray(depth)
    H, W = depth.shape
    pad = np.pad(depth.astype(np.float64), 1, mode="edge")
    s = np.zeros((H, W))
    for dy in range(3):
        for dx in range(3):
            s = s + pad[dy:dy + H, dx:dx + W]
    return np.where(depth == 0, 0.0, s / 9.0).astype(np.float32)


def city(n_views, H, W, seed=3, blurred=False):
    """geometry_np.city_views as Views -> (grid, terrain, views, origin)"""
    grid, terrain, cams, depths, origin = gnp.city_views(n_views, H, W, seed=seed)
    return grid, terrain, [View(blur3(d) if blurred else d, c, None) for d, c in zip(depths, cams)], origin


def dsm_of(views, grid, origin, view_masks=None):
    """geometry_np.dsm_max over the views' used (and, with view_masks, kept) pixels -> float64 [ysize,xsize], NaN where empty"""
    pts = [gnp.unproject(v.depth, v.camera.R, v.camera.T, v.camera.focal_x, v.camera.focal_y, v.camera.cx, v.camera.cy, origin=origin,
                         mask=v.mask if view_masks is None else view_masks[k]) for k, v in enumerate(views)]
    return gnp.dsm_max(np.vstack(pts), grid)[0]
