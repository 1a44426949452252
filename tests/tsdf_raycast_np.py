"""The ray-cast of sfgs.tsdf (TsdfVolume.raycast: csrc/tsdf.hip, csrc/tsdf_math.h; include/sfgs.h states the sequence in words)
restated in numpy -- what the kernel and the host build of the header are held to byte for byte -- with the empty-space table
and the scenes the tests share. Float64 on the stored float32 values, every product, sum and quotient spelled elementwise in
the order the header takes it. Only the UNIFORM march is stated here: every sample of every ray is evaluated until the ray's
hit, so the skipping marches of the kernel and the host build are checked against something that skips nothing.

  raycast          volume + camera -> depth, normal, rgb, a branch code per pixel and the samples evaluated
  skip_table       the byte per brick of 8 x 8 x 8 cells
  scenes           sphere / fusion / wavy volumes and the cameras of the tests"""
import functools
import types

import numpy as np

import consistency_np as cnp
import tsdf_np as tnp

MAX_SAMPLES = 1 << 20
BRICK = 8
# bits of the per-pixel branch code
ZERO_COMPONENT = 1        # a direction component is exactly 0
MISSED_BOX = 2            # the clip left nothing
STARTS_AT_NEAR = 4        # z0 == near: the ray begins inside the box
FIRST_VALID_NEGATIVE = 8  # the first valid sample of the ray has a value < 0
UNBRACKETED = 16          # a valid negative sample k >= 1 behind an invalid one: a crossing that is no hit
NEGATIVE_TO_POSITIVE = 32 # a valid sample >= 0 right behind a valid negative one
HIT = 64
RAN_OUT = 128             # all K samples evaluated, no hit
BRANCHES = {"zero_component": ZERO_COMPONENT, "missed_box": MISSED_BOX, "starts_at_near": STARTS_AT_NEAR,
            "first_valid_negative": FIRST_VALID_NEGATIVE, "unbracketed": UNBRACKETED, "negative_to_positive": NEGATIVE_TO_POSITIVE,
            "hit": HIT, "ran_out": RAN_OUT}


def lerp(a, b, f):
    return a + f * (b - a)


def count(code, name):
    return int(((code & BRANCHES[name]) != 0).sum())


def _corners(plane, cell):
    """plane [nz,ny,nx], cell int [n,3] (x, y, z) -> the eight corner values, float32 [8,n]"""
    x, y, z = cell[:, 0], cell[:, 1], cell[:, 2]
    return np.stack([plane[z + ((k >> 2) & 1), y + ((k >> 1) & 1), x + (k & 1)] for k in range(8)])


def _trilinear(v, f):
    v = v.astype(np.float64)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    x00, x10, x01, x11 = lerp(v[0], v[1], fx), lerp(v[2], v[3], fx), lerp(v[4], v[5], fx), lerp(v[6], v[7], fx)
    y0, y1 = lerp(x00, x10, fy), lerp(x01, x11, fy)
    return lerp(y0, y1, fz)


def _gradient(v, f):
    v = v.astype(np.float64)
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    x00, x10, x01, x11 = lerp(v[0], v[1], fx), lerp(v[2], v[3], fx), lerp(v[4], v[5], fx), lerp(v[6], v[7], fx)
    y0, y1 = lerp(x00, x10, fy), lerp(x01, x11, fy)
    gz = y1 - y0
    gy = lerp(x10 - x00, x11 - x01, fz)
    gx = lerp(lerp(v[1] - v[0], v[3] - v[2], fy), lerp(v[5] - v[4], v[7] - v[6], fy), fz)
    return np.stack([gx, gy, gz], axis=-1)


def raycast(tsdf, weight, rgb, origin, voxel_size, camera, H, W, step=None, near=0.0, far=np.inf, normals=True):
    """-> namespace depth float32 [1,H,W], normal float32 [3,H,W] (None without normals), rgb float32 [3,H,W] (None without
    colours), code uint8 [H,W] (bits of BRANCHES), samples (how many samples the uniform march evaluated), hits."""
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    nz, ny, nx = tsdf.shape
    n = (nx, ny, nz)
    o, vox = np.asarray(origin, dtype=np.float64), np.float64(voxel_size)
    inv = np.float64(1.0) / vox
    step = vox if step is None else np.float64(step)
    near, far = np.float64(near), np.float64(far)
    k = cnp.constants(camera, H, W)
    P = H * W
    depth = np.zeros(P, np.float32)
    normal = np.zeros((3, P), np.float32) if normals else None
    colour = None if rgb is None else np.zeros((3, P), np.float32)
    code = np.zeros(P, np.uint8)
    out = types.SimpleNamespace(depth=depth.reshape(1, H, W), normal=None if normal is None else normal.reshape(3, H, W),
                                rgb=None if colour is None else colour.reshape(3, H, W), code=code.reshape(H, W), samples=0, hits=0)
    if min(n) < 2:                                                            # no cell: every ray misses
        code[:] = MISSED_BOX
        return out
    row, col = (a.reshape(-1).astype(np.float64) for a in np.mgrid[0:H, 0:W])
    # 1. the ray
    x, y = (col - k.cx_pix) / k.focal_x, (row - k.cy_pix) / k.focal_y
    d = np.stack([(x * k.M[0, a] + y * k.M[1, a]) + k.M[2, a] for a in range(3)], axis=-1)
    c = k.c
    # 2. the clip
    z0, z1, inside = np.full(P, near), np.full(P, far), np.ones(P, bool)
    for a in range(3):
        lo, hi = o[a] + 0.5 * vox, o[a] + (np.float64(n[a]) - 0.5) * vox
        zero = d[:, a] == 0.0
        code[zero] |= ZERO_COMPONENT
        inside &= ~zero | ((lo <= c[a]) & (c[a] <= hi))
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - c[a]) / d[:, a], (hi - c[a]) / d[:, a]
            swap = t0 > t1
            t0, t1 = np.where(swap, t1, t0), np.where(swap, t0, t1)
            z0 = np.where(~zero & (t0 > z0), t0, z0)
            z1 = np.where(~zero & (t1 < z1), t1, z1)
    with np.errstate(invalid="ignore"):
        alive = inside & (z0 <= z1)
    code[~alive] |= MISSED_BOX
    code[alive & (z0 == near)] |= STARTS_AT_NEAR
    # 3. the lattice
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.floor((z1 - z0) / step)
        K = np.where(q < MAX_SAMPLES - 1, q + 1, MAX_SAMPLES)
    K = np.where(alive, K, 0).astype(np.int64)

    def sample(rays, kk):
        """-> cell int [m,3], f float64 [m,3] of sample kk (a number or an array) of `rays`"""
        z = z0[rays] + np.float64(kk) * step if np.isscalar(kk) else z0[rays] + kk.astype(np.float64) * step
        cell, f = np.empty((len(rays), 3), np.int64), np.empty((len(rays), 3))
        for a in range(3):
            p = c[a] + z * d[rays, a]
            g = (p - o[a]) * inv - 0.5
            with np.errstate(invalid="ignore"):
                i = np.floor(g)
                i = np.where(i >= 0.0, i, 0.0)
                i = np.where(i > n[a] - 2, np.float64(n[a] - 2), i)
                r = g - i
                r = np.where(r >= 0.0, r, 0.0)
                r = np.where(r > 1.0, 1.0, r)
            cell[:, a], f[:, a] = i.astype(np.int64), r
        return cell, f

    # 4., 5. the uniform march: every ray in step, k ascending
    rays = np.nonzero(alive)[0]
    before, prev = np.zeros(P, bool), np.zeros(P)                            # of sample k - 1: valid with a value >= 0; its value
    seen_valid, last_negative = np.zeros(P, bool), np.zeros(P, bool)
    last_invalid = np.zeros(P, bool)
    hit_k, vp, vc = np.zeros(P, np.int64), np.zeros(P), np.zeros(P)
    kk = 0
    while len(rays):
        rays = rays[K[rays] > kk]
        if not len(rays):
            break
        cell, f = sample(rays, kk)
        valid = (_corners(weight, cell) > 0).all(axis=0)
        val = _trilinear(_corners(tsdf, cell), f)
        out.samples += len(rays)
        with np.errstate(invalid="ignore"):
            neg, pos = valid & (val < 0.0), valid & (val >= 0.0)
        code[rays[neg & ~seen_valid[rays]]] |= FIRST_VALID_NEGATIVE
        seen_valid[rays] |= valid
        if kk >= 1:
            code[rays[neg & last_invalid[rays]]] |= UNBRACKETED
            code[rays[pos & last_negative[rays]]] |= NEGATIVE_TO_POSITIVE
        hit = neg & before[rays] if kk >= 1 else np.zeros(len(rays), bool)
        h = rays[hit]
        hit_k[h], vp[h], vc[h] = kk, prev[h], val[hit]
        before[rays], prev[rays], last_negative[rays], last_invalid[rays] = pos, val, neg, ~valid
        rays = rays[~hit]
        kk += 1
    # 6. the outputs of the hits
    h = np.nonzero(hit_k >= 1)[0]
    code[h] |= HIT
    code[alive & (hit_k == 0)] |= RAN_OUT
    out.hits = len(h)
    if len(h):
        zp, zc = z0[h] + (hit_k[h] - 1).astype(np.float64) * step, z0[h] + hit_k[h].astype(np.float64) * step
        w = vp[h] / (vp[h] - vc[h])
        depth[h] = (zp + w * (zc - zp)).astype(np.float32)
        (cp, fp), (cc, fc) = sample(h, hit_k[h] - 1), sample(h, hit_k[h])
        if normals:
            gp, gc = _gradient(_corners(tsdf, cp), fp), _gradient(_corners(tsdf, cc), fc)
            g = gp + w[:, None] * (gc - gp)
            length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            with np.errstate(invalid="ignore", divide="ignore"):
                normal[:, h] = np.where((length > 0)[:, None], g / length[:, None], 0.0).T.astype(np.float32)
        if rgb is not None:
            for ch in range(3):
                plane = np.asarray(rgb[ch], np.float32)
                a, b = _trilinear(_corners(plane, cp), fp), _trilinear(_corners(plane, cc), fc)
                colour[ch, h] = (a + w * (b - a)).astype(np.float32)
    return out


def skip_bricks(n):
    return 1 if n < 2 else (n - 1 + BRICK - 1) // BRICK


def skip_table(tsdf, weight):
    """uint8 [bz,by,bx]: 1 where some voxel of the brick's footprint -- voxels 8b ... min(8b + 8, n - 1) per axis -- has
    weight > 0 and tsdf < 0. Zeros for a volume without cells."""
    nz, ny, nx = tsdf.shape
    table = np.zeros((skip_bricks(nz), skip_bricks(ny), skip_bricks(nx)), np.uint8)
    if min(nx, ny, nz) < 2:
        return table
    with np.errstate(invalid="ignore"):
        flag = (weight > 0) & (tsdf < 0)
    for bz in range(table.shape[0]):
        for by in range(table.shape[1]):
            for bx in range(table.shape[2]):
                table[bz, by, bx] = flag[8 * bz:min(8 * bz + 8, nz - 1) + 1, 8 * by:min(8 * by + 8, ny - 1) + 1,
                                         8 * bx:min(8 * bx + 8, nx - 1) + 1].any()
    return table


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def nadir_camera(eye, W, H, focal):
    """Looking straight down -z from `eye` with x right and y toward -Y; the principal point on the centre of pixel
    (W // 2, H // 2), so that pixel's ray has two direction components that are exactly 0."""
    A = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])      # columns: the camera's axes in the world
    eye = np.asarray(eye, np.float64)
    return types.SimpleNamespace(R=A, T=-A @ eye, focal_x=float(focal), focal_y=float(focal), cx=0.0, cy=0.0, eye=eye)


@functools.lru_cache(maxsize=None)
def fused_volume(which=(0, 1, 2, 3, 4), colors=True):
    """tsdf_np.fusion_scene's views `which` fused by the restatement -> (vol, views, images, state), read-only"""
    vol, views, images = tnp.fusion_scene()
    state = tnp.empty_state(vol.dims, colors)
    tnp.integrate(state, vol, [views[k] for k in which], [images[k] for k in which] if colors else None)
    for a in (state.tsdf, state.weight, state.rgb):
        if a is not None:
            a.setflags(write=False)
    return vol, views, images, state


def sphere_camera(W=24, H=20):
    return tnp.look_at((19.0, -7.0, 15.0), tnp.SPHERE.centre, W, H)


def wavy_top_camera(dims=(72, 64, 64), W=48, H=40):
    """Above wavy_volume(dims), looking down on all of it, a little off the axis"""
    _, _, _, origin, voxel = tnp.wavy_volume((2, 2, 2))
    nx, ny, nz = dims
    mid = np.array(origin) + 0.5 * voxel * np.array([nx, ny, nz])
    return tnp.look_at(mid + np.array([1.7, -2.3, 1.6 * voxel * nz]), mid, W, H, up=(0.0, 1.0, 0.0))


WAVY = (72, 64, 64)


def volume_of(state, vol):
    return state.tsdf, state.weight, state.rgb, vol.origin, vol.voxel_size


@functools.lru_cache(maxsize=None)
def wavy():
    case = tnp.wavy_volume(WAVY, colors=True)
    for a in case[:3]:
        a.setflags(write=False)
    return case


BRANCH_SCENES = ("a direction component exactly 0", "rays that miss the box", "a camera inside the box",
                 "a first valid sample that is negative", "a crossing behind an invalid sample", "near beyond the surface",
                 "far in front of the surface", "a step of 0.37 voxels", "a step of 2.5 voxels", "a volume with a dimension of 1")


def branch_scenes():
    """name -> (case, camera, H, W, keywords, {branch: its exact count in the restatement}); the CPU and the GPU suite run the same"""
    vol, views, _, state = fused_volume()
    fus, wav, top = volume_of(state, vol), wavy(), wavy_top_camera(WAVY)
    mid = np.array(wav[3]) + 0.5 * wav[4] * np.array(WAVY)
    nadir = nadir_camera(mid + np.array([0.0, 0.0, 14.0]), 16, 12, 14.0)
    flat = np.full((1, 10, 11), -1.0, np.float32)
    flat[0, :, 5:] = 1.0
    thin = (flat, np.ones_like(flat), None, (0.0, 0.0, 0.0), 1.0)
    return {
        "a direction component exactly 0": (wav, nadir, 12, 16, {}, {"zero_component": 27, "hit": 188}),
        "rays that miss the box": (tnp.sphere_volume(True), sphere_camera(), 20, 24, {}, {"missed_box": 135, "hit": 74}),
        "a camera inside the box": (fus, views[3].camera, 40, 48, {}, {"starts_at_near": 1920, "hit": 1920}),
        "a first valid sample that is negative": (fus, views[0].camera, 40, 48, {}, {"first_valid_negative": 19, "hit": 840}),
        "a crossing behind an invalid sample": (wav, top, 40, 48, {}, {"unbracketed": 31, "negative_to_positive": 1, "hit": 896}),
        "near beyond the surface": (wav, top, 40, 48, {"near": 30.0}, {"starts_at_near": 650, "first_valid_negative": 544, "hit": 100}),
        "far in front of the surface": (wav, top, 40, 48, {"far": 19.0}, {"ran_out": 1636, "hit": 42}),
        "a step of 0.37 voxels": (wav, top, 40, 48, {"step": 0.37 * 0.25}, {"hit": 906, "ran_out": 784}),
        "a step of 2.5 voxels": (wav, top, 40, 48, {"step": 2.5 * 0.25}, {"hit": 880, "ran_out": 810}),
        "a volume with a dimension of 1": (thin, nadir_camera((5.0, 5.0, 9.0), 16, 12, 14.0), 12, 16, {}, {"missed_box": 192, "hit": 0}),
    }
