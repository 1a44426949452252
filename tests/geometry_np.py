"""The reference's geometry evaluation (evaluate_gs_geometry.py:132-215, :270-312, :528-585 and dsmr.py) restated in vectorised
numpy, float64 throughout -- what csrc/geometry.hip is held to -- and the seeded scenes the geometry tests,
tests/golden/make_golden_geometry.py and tools/bench_geometry.py share: a terrain with boxes ("buildings"), a pinhole camera
looking down at it from a given elevation, and depth maps of it.

Three stages:
  1. unproject / cell_coords / dsm_max / dsm_mean     depth map -> points -> height grid
  2. downsample2x / mean_std / compute_ncc / recursive_ncc / compute_shift     dsmr registration
  3. apply_shift / dsm_metrics / register_simple      shift + compare

Decisions the reference leaves open or that differ from it on purpose (sfgs/geometry.py lists them for users):
  * unproject() drops +inf depths (the reference's `depth > 0` keeps them; its caller scrubs them to 0 first);
  * a shift whose pairs are empty or whose sigma_u * sigma_v is 0 -- the reference divides by zero there -- is skipped;
    with every shift skipped (dx, dy) stay at their start and b is NaN;
  * dsm_mean() IS the specification of mode="mean" (plyflatten's own cell rule is unpinned): every point adds its height to
    all cells within `radius` columns and rows of its own cell, a point whose own cell is outside the grid is dropped,
    cell = sum / count."""
import types

import numpy as np


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------------
def pixel_centre(c, size):
    return c / 2 * size + size / 2


def unproject(depth, R, T, focal_x, focal_y, cx=0.0, cy=0.0, origin=None, mask=None):
    """-> float64 [N,3] (east, north, up) of the used pixels in row-major order."""
    depth = np.asarray(depth)
    depth = depth.reshape(depth.shape[-2:])
    H, W = depth.shape
    valid = (depth > 0) & np.isfinite(depth)
    if mask is not None:
        valid &= np.asarray(mask).reshape(H, W) != 0
    v, u = np.nonzero(valid)
    z = depth[valid].astype(np.float64)
    x = (u - pixel_centre(cx, W)) * z / focal_x
    y = (v - pixel_centre(cy, H)) * z / focal_y
    M = np.asarray(R, dtype=np.float64).T
    c = -M @ np.asarray(T, dtype=np.float64)
    p = np.stack([x * M[0, j] + y * M[1, j] + z * M[2, j] + c[j] for j in range(3)], axis=-1)
    if origin is not None:
        p = p + np.asarray(origin, dtype=np.float64)
    return p


def cell_coords(points, grid):
    """grid: (xoff, yoff_top, xsize, ysize, resolution) -> (qx, qy) float64 cell coordinates before truncation"""
    xoff, yoff_top, _, _, res = grid
    return (points[:, 0] - xoff) / res, (yoff_top - points[:, 1]) / res


def cells(points, grid):
    """-> (gx, gy, inside): truncation toward zero, as astype(int)"""
    qx, qy = cell_coords(points, grid)
    _, _, xsize, ysize, _ = grid
    with np.errstate(invalid="ignore"):
        gx, gy = np.trunc(qx), np.trunc(qy)
        inside = (gx >= 0) & (gx < xsize) & (gy >= 0) & (gy < ysize)
    return gx[inside].astype(np.int64), gy[inside].astype(np.int64), inside


def dsm_max(points, grid):
    _, _, xsize, ysize, _ = grid
    gx, gy, inside = cells(points, grid)
    out = np.full((ysize, xsize), -np.inf)
    np.maximum.at(out, (gy, gx), points[inside, 2])
    out[out == -np.inf] = np.nan
    return out, int(inside.sum())


def dsm_mean_sums(points, grid, radius):
    _, _, xsize, ysize, _ = grid
    gx, gy, inside = cells(points, grid)
    h = points[inside, 2]
    total, count = np.zeros((ysize, xsize)), np.zeros((ysize, xsize), dtype=np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            cx, cy = gx + dx, gy + dy
            ok = (cx >= 0) & (cx < xsize) & (cy >= 0) & (cy < ysize)
            np.add.at(total, (cy[ok], cx[ok]), h[ok])
            np.add.at(count, (cy[ok], cx[ok]), 1)
    return total, count, int(inside.sum())


def dsm_mean(points, grid, radius=1):
    total, count, n = dsm_mean_sums(points, grid, radius)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(count > 0, total / count, np.nan), n


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------------
def downsample2x(u):
    """[H,W] -> [ceil(H/2), ceil(W/2)]: the finite-mean of the 2 x 2 window whose corner is the LAST pixel of
    {2J, 2J+1} x {2I, 2I+1} inside the raster (the reference's loop writes out[j // 2, i // 2] for every (j, i))."""
    u = np.asarray(u, dtype=np.float64)
    H, W = u.shape
    pad = np.full((H + 1, W + 1), np.nan)
    pad[:H, :W] = u
    j0 = np.minimum(2 * np.arange((H + 1) // 2) + 1, H - 1)[:, None]
    i0 = np.minimum(2 * np.arange((W + 1) // 2) + 1, W - 1)[None, :]
    s, n = np.zeros((j0.size, i0.size)), np.zeros((j0.size, i0.size), dtype=np.int64)
    for k in range(2):            # the reference's order: column offset outer, row offset inner
        for l in range(2):
            t = pad[j0 + l, i0 + k]
            f = np.isfinite(t)
            s = np.where(f, s + np.where(f, t, 0.0), s)
            n += f
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / n, np.nan)


def shifted(v, shape, dx, dy):
    """v(i + dx, j + dy) over a raster of `shape`, NaN outside v (dsmr.valnan)"""
    H, W = shape
    Hv, Wv = v.shape
    out = np.full((H, W), np.nan)
    j0, j1 = max(0, -dy), min(H, Hv - dy)
    i0, i1 = max(0, -dx), min(W, Wv - dx)
    if j1 > j0 and i1 > i0:
        out[j0:j1, i0:i1] = v[j0 + dy:j1 + dy, i0 + dx:i1 + dx]
    return out


def mean_std(u, v, dx=0, dy=0):
    """-> (mu_u, mu_v, sigma_u, sigma_v, xcorr, count); count == 0: the five numbers are NaN"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    vv = shifted(v, u.shape, dx, dy)
    m = np.isfinite(u) & np.isfinite(vv)
    n = int(m.sum())
    if n == 0:
        return (np.nan,) * 5 + (0,)
    a, b = u[m], vv[m]
    mu, mv = a.sum() / n, b.sum() / n
    a, b = a - mu, b - mv
    return mu, mv, np.sqrt((a * a).sum() / n), np.sqrt((b * b).sum() / n), (a * b).sum() / n, n


def scores(u, v, irange, initdx, initdy):
    """-> float64 [2 irange + 1, 2 irange + 1] indexed [y, x]: the NCC of every shift, NaN where the shift is skipped"""
    S = 2 * irange + 1
    out = np.full((S, S), np.nan)
    for iy in range(S):
        for ix in range(S):
            _, _, su, sv, xc, n = mean_std(u, v, initdx - irange + ix, initdy - irange + iy)
            if n > 0 and su * sv != 0.0:
                out[iy, ix] = xc / (su * sv)
    return out


def compute_ncc(u, v, irange, initdx, initdy):
    """-> (dx, dy, best score, runner-up score): y outer, x inner, strict >; skipped and NaN shifts never win"""
    sc = scores(u, v, irange, initdx, initdy)
    dx, dy, maxv = initdx, initdy, -np.inf
    for iy in range(sc.shape[0]):
        for ix in range(sc.shape[1]):
            if sc[iy, ix] > maxv:
                dx, dy, maxv = initdx - irange + ix, initdy - irange + iy, sc[iy, ix]
    rest = np.sort(sc[np.isfinite(sc)])
    return dx, dy, (maxv if np.isfinite(maxv) else np.nan), (rest[-2] if rest.size > 1 else np.nan)


def recursive_ncc(u, v, irange=5, dx=0, dy=0, margins=None):
    """dsmr.recursive_ncc. margins: a list that receives (best, runner-up) per level, coarsest first."""
    if min(u.shape) > 100:
        dx, dy = recursive_ncc(downsample2x(u), downsample2x(v), irange, dx // 2, dy // 2, margins)
        dx, dy = dx * 2, dy * 2
    dx, dy, best, second = compute_ncc(u, v, irange, dx, dy)
    if margins is not None:
        margins.append((best, second))
    return dx, dy


def compute_shift(u, v, irange=5, scaling=False, init=(0, 0), margins=None):
    """dsmr.compute_shift on arrays -> (dx, dy, a, b, stats); stats = (mu_u, mu_v, sigma_u, sigma_v, xcorr) at the shift"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    levels = []
    dx, dy = recursive_ncc(u, v, irange, int(init[0]), int(init[1]), levels)
    if margins is not None:
        margins.extend(levels)
    if not np.isfinite(levels[-1][0]):                 # every shift of the finest level was skipped
        return dx, dy, (np.nan if scaling else 1.0), np.nan, (np.nan,) * 5
    mu, mv, su, sv, xc, _ = mean_std(u, v, dx, dy)
    a = su / sv if scaling else 1.0
    return dx, dy, a, mu - mv * a, (mu, mv, su, sv, xc)


# ---- stage 3 ---------------------------------------------------------------------------------------------------------------------
def apply_shift(v, dx, dy, a, b):
    v = np.asarray(v, dtype=np.float64)
    return (a * shifted(v, v.shape, dx, dy) + b) + 0.0


def dsm_metrics(pred, gt, mask=None, shift=None):
    """compute_dsm_metrics; shift: (dx, dy, a, b) applied to pred first. -> dict, plus "dz" = register_dsms_simple's offset"""
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    if shift is not None:
        pred = apply_shift(pred, *shift)
    if mask is not None:
        keep = np.asarray(mask) != 0
        pred, gt = np.where(keep, pred, np.nan), np.where(keep, gt, np.nan)
    both = ~np.isnan(pred) & ~np.isnan(gt)
    n, ngt = int(both.sum()), int((~np.isnan(gt)).sum())
    if n == 0:
        return {"mae": np.nan, "rmse": np.nan, "valid_pixels": 0, "completeness": 0.0, "dz": 0.0}
    d = pred[both] - gt[both]
    return {"mae": np.abs(d).mean(), "rmse": np.sqrt((d * d).mean()), "valid_pixels": n, "completeness": n / ngt,
            "dz": (gt[both] - pred[both]).mean()}


def register_simple(pred, gt):
    return dsm_metrics(pred, gt)["dz"]


# ---- seeded scenes ---------------------------------------------------------------------------------------------------------------
def make_terrain(rows, cols, seed, boxes=8, nan_fraction=0.0):
    """-> float64 [rows, cols] heights in metres: low hills, `boxes` flat-roofed blocks, a little roughness"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    h = 12.0 + 4.0 * np.sin(x / (7.0 + cols / 9.0) + rng.uniform(0, 6)) * np.cos(y / (5.0 + rows / 11.0) + rng.uniform(0, 6))
    for _ in range(boxes):
        r0, c0 = int(rng.integers(0, max(1, rows - 3))), int(rng.integers(0, max(1, cols - 3)))
        r1, c1 = r0 + int(rng.integers(2, max(3, rows // 4 + 3))), c0 + int(rng.integers(2, max(3, cols // 4 + 3)))
        h[r0:r1, c0:c1] = 15.0 + rng.uniform(5.0, 40.0)
    h += rng.uniform(-0.3, 0.3, h.shape)
    if nan_fraction > 0:
        h[rng.random(h.shape) < nan_fraction] = np.nan
    return h


def shifted_pair(rows, cols, seed, dx, dy, dz, sec_shape=None, nan_fraction=0.07, scale=1.0, noise=0.05):
    """-> (ref [rows, cols], sec [sec_shape]) with ref(i, j) ~ scale * sec(i + dx, j + dy) + dz (i: column, j: row), noise and
    NaN holes in both: registering sec on ref finds (dx, dy)"""
    rng = np.random.default_rng(seed + 1)
    pad = 2 * (abs(dx) + abs(dy)) + 16
    sr, sc = sec_shape if sec_shape is not None else (rows, cols)
    big = make_terrain(max(rows, sr) + 2 * pad, max(cols, sc) + 2 * pad, seed, boxes=14)
    ref = big[pad:pad + rows, pad:pad + cols].copy()
    sec = (big[pad - dy:pad - dy + sr, pad - dx:pad - dx + sc] - dz) / scale + rng.normal(0, noise, (sr, sc))
    ref[rng.random(ref.shape) < nan_fraction] = np.nan
    sec[rng.random(sec.shape) < nan_fraction] = np.nan
    return np.round(ref * 16) / 16, np.round(sec * 16) / 16     # multiples of 1/16 m below 128 m: exact in float16


def look_down_camera(target, elevation_deg, azimuth_deg, distance, focal, cx=0.0, cy=0.0):
    """A Camera-like object (R, T, focal_x, focal_y, cx, cy as evaluate_gs_geometry.py reads them) at `distance` from
    `target`, `elevation_deg` above the horizon, looking at the target; camera axes: x right, y down, z forward."""
    e, a = np.deg2rad(elevation_deg), np.deg2rad(azimuth_deg)
    C = np.asarray(target, dtype=np.float64) + distance * np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
    f = (np.asarray(target, dtype=np.float64) - C) / distance
    up = np.array([0.0, 0.0, 1.0]) if abs(f[2]) < 0.999 else np.array([0.0, 1.0, 0.0])
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    A = np.stack([r, d, f], axis=1)                    # columns: the camera's axes in the world
    return types.SimpleNamespace(R=A, T=-A @ C, focal_x=float(focal), focal_y=float(focal) * 1.01, cx=float(cx), cy=float(cy),
                                 centre=C, axes=A)


def render_depth(terrain, res, cam, H, W, steps=192, reach=(0.5, 1.6)):
    """float32 [H,W] depth (z along the camera's forward axis) of the height field `terrain` (row 0 = north edge, cell size
    `res`, south-west corner at the world's origin) by marching every pixel's ray; 0 where the ray leaves without a hit."""
    rows, cols = terrain.shape
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    dirs = np.stack([(u - pixel_centre(cam.cx, W)) / cam.focal_x, (v - pixel_centre(cam.cy, H)) / cam.focal_y,
                     np.ones_like(u)], axis=-1) @ cam.axes.T
    dist = np.linalg.norm(cam.centre - np.array([cols * res / 2, rows * res / 2, 0.0]))
    depth = np.zeros((H, W))
    for z in np.linspace(reach[0] * dist, reach[1] * dist, steps):
        p = cam.centre + dirs * z
        gx, gy = np.floor(p[..., 0] / res).astype(np.int64), np.floor((rows * res - p[..., 1]) / res).astype(np.int64)
        inside = (gx >= 0) & (gx < cols) & (gy >= 0) & (gy < rows)
        ground = np.where(inside, np.nan_to_num(terrain, nan=0.0)[gy.clip(0, rows - 1), gx.clip(0, cols - 1)], -np.inf)
        hit = (depth == 0) & inside & (p[..., 2] <= ground)
        depth[hit] = z
    return depth.astype(np.float32)


def city_views(n_views, H, W, seed, cells=64, res=0.5, origin=(4.0e5, 3.3e6, 20.0), elevation=62.0):
    """A terrain of cells x cells at `res` metres and `n_views` depth maps of it from a ring of cameras.
    -> (grid 5-tuple in UTM, terrain, cameras, depths, origin)"""
    terrain = make_terrain(cells, cells, seed)
    side = cells * res
    target = np.array([side / 2, side / 2, 12.0])
    cams, depths = [], []
    for k in range(n_views):
        cam = look_down_camera(target, elevation + 3.0 * (k % 3), 360.0 * k / n_views + 11.0, 3.0 * side,
                               focal=2.6 * max(H, W), cx=0.02 * (k % 2), cy=-0.01 * (k % 3))
        cams.append(cam)
        depths.append(render_depth(terrain, res, cam, H, W))
    grid = (origin[0], origin[1] + side, cells, cells, res)
    return grid, terrain, cams, depths, np.asarray(origin, dtype=np.float64)
