"""The orthophoto of sfgs.ortho (csrc/ortho.hip) restated in numpy -- what the kernels are held to, bit for bit -- and the seeded
scene its tests share. It builds on tests/geometry_np.py (the pixel rule, the float64 unprojection, the cell rule) and changes
nothing there.

  quantize            sfgs_frame_quantize's rule in float32: img * 255 + 0.5, clip, truncate, NaN -> 0
  key32 / unkey32     the order-preserving integer key of a float32 and its inverse; no number has key 0
  unproject           geometry_np.unproject's sequence with the camera centre formed as sfgs.geometry._check_view forms it for
                      the DSM: c = -(np.ascontiguousarray(R.T)) @ T (the last bit of numpy's product depends on the memory order)
  keys                views -> one uint64 per cell with np.maximum.at: K32(float32(up)) << 32 | r << 24 | g << 16 | b << 8 | tag,
                      0 = empty; the winner is the maximum over (float32 height, r, g, b, tag), lexicographically
  resolve             keys -> rgb, height, source, state, coverage; with fill r an EMPTY cell takes the maximum key among the
                      non-empty cells of its (2r + 1)^2 window clipped to the grid (one pass: donated values do not propagate)"""
import collections
import functools

import numpy as np

import geometry_np as gnp

View = collections.namedtuple("View", "depth image camera mask tag")
Result = collections.namedtuple("Result", "rgb height source state coverage")


def quantize(img):
    with np.errstate(invalid="ignore"):
        t = np.asarray(img, dtype=np.float32) * np.float32(255.0) + np.float32(0.5)
        return np.where(np.isnan(t), np.float32(0.0), np.clip(t, np.float32(0.0), np.float32(255.0))).astype(np.uint8)


def key32(h):
    """float32 array -> uint32 keys: a < b <=> key32(a) < key32(b)"""
    b = np.ascontiguousarray(h, dtype=np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey32(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k >> np.uint32(31), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def used_pixels(depth, mask=None):
    depth = np.asarray(depth)
    depth = depth.reshape(depth.shape[-2:])
    valid = (depth > 0) & np.isfinite(depth)
    if mask is not None:
        valid &= np.asarray(mask).reshape(depth.shape) != 0
    return valid


def unproject(depth, cam, origin=None, mask=None):
    """-> float64 [N,3] (east, north, up) of the used pixels in row-major order"""
    depth = np.asarray(depth)
    depth = depth.reshape(depth.shape[-2:])
    H, W = depth.shape
    valid = used_pixels(depth, mask)
    v, u = np.nonzero(valid)
    z = depth[valid].astype(np.float64)
    x = (u - gnp.pixel_centre(getattr(cam, "cx", 0.0), W)) * z / cam.focal_x
    y = (v - gnp.pixel_centre(getattr(cam, "cy", 0.0), H)) * z / cam.focal_y
    M = np.ascontiguousarray(np.asarray(cam.R, dtype=np.float64).T)
    c = -M @ np.asarray(cam.T, dtype=np.float64)
    org = np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float64)
    return np.stack([(x * M[0, j] + y * M[1, j] + z * M[2, j] + c[j]) + org[j] for j in range(3)], axis=-1)


def view_keys(view, grid, origin=None):
    """-> (gy, gx, uint64 key) of the view's landed points"""
    depth, image, cam, mask, tag = view
    assert 1 <= int(tag) <= 255
    pts = unproject(depth, cam, origin, mask)
    col = quantize(image)[:, used_pixels(depth, mask)].T.astype(np.uint64)          # [N,3], the rows' order
    finite = np.isfinite(pts[:, 2])
    pts, col = pts[finite], col[finite]
    gx, gy, inside = gnp.cells(pts, grid)
    with np.errstate(over="ignore"):
        hi = key32(pts[inside, 2].astype(np.float32)).astype(np.uint64)              # astype: round to nearest even
    col = col[inside]
    return gy, gx, (hi << np.uint64(32)) | (col[:, 0] << np.uint64(24)) | (col[:, 1] << np.uint64(16)) | (col[:, 2] << np.uint64(8)) | np.uint64(int(tag))


def keys(views, grid, origin=None):
    """views: View tuples -> (uint64 [ysize, xsize], landed points)"""
    _, _, xsize, ysize, _ = grid
    acc, n = np.zeros((ysize, xsize), dtype=np.uint64), 0
    for view in views:
        gy, gx, k = view_keys(view, grid, origin)
        np.maximum.at(acc, (gy, gx), k)
        n += len(k)
    return acc, n


def resolve(acc, fill=0):
    acc = np.asarray(acc, dtype=np.uint64)
    ysize, xsize = acc.shape
    best = acc.copy()
    if fill > 0:
        pad = np.zeros((ysize + 2 * fill, xsize + 2 * fill), dtype=np.uint64)
        pad[fill:fill + ysize, fill:fill + xsize] = acc
        around = np.zeros_like(acc)
        for dy in range(2 * fill + 1):
            for dx in range(2 * fill + 1):
                around = np.maximum(around, pad[dy:dy + ysize, dx:dx + xsize])
        best = np.where(acc == 0, around, acc)
    state = np.where(acc != 0, 1, np.where(best != 0, 2, 0)).astype(np.uint8)
    lo = (best & np.uint64(0xffffffff)).astype(np.uint32)
    rgb = np.stack([(lo >> np.uint32(s)).astype(np.uint8) for s in (24, 16, 8)], axis=-1)
    source = lo.astype(np.uint8)
    height = np.where(best != 0, unkey32((best >> np.uint64(32)).astype(np.uint32)), np.float32(np.nan)).astype(np.float32)
    coverage = np.bincount(source.reshape(-1), minlength=256).astype(np.int64)
    return Result(rgb, height, source, state, coverage)


def seeded_images(depths, seed):
    """float32 [3,H,W] per depth map, values a little beyond [0, 1]"""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.1, 1.1, (3,) + d.shape[-2:]).astype(np.float32) for d in depths]


@functools.lru_cache(maxsize=None)
def base_scene():
    """geometry_np.city_views(3, 40, 48, seed=1, cells=24) with seeded images: 1920 pixels per view (7 full workgroups of 256
    and a half one) onto 576 cells. -> (grid, cameras, depths, images, origin), read-only"""
    grid, _, cams, depths, origin = gnp.city_views(3, 40, 48, seed=1, cells=24)
    images = seeded_images(depths, 77)
    for a in depths + images + [origin]:
        a.setflags(write=False)
    return grid, tuple(cams), tuple(depths), tuple(images), origin
