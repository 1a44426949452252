"""Seeded scenes under a general camera (TEST INFRASTRUCTURE; DESIGN.md section 8.7, "General cameras"): what sfgs.synth.scene never sets.

sfgs.synth.scene puts the pinhole at the world origin with the identity rotation (or a pitch that leaves the view-space
coordinates unchanged), a centred principal point, scale_modifier 1, fovy derived from fovx, and every Gaussian in front
of the camera inside the guard band of the EWA Jacobian. Here:

  pose       camera-to-world R = Rz(37 deg) Rx(25 deg) Ry(-15 deg), centre C = (12, -7, 3), t = -R^T C: every entry of the
             view matrix is non-zero and none equals another, campos is far from the origin;
  cx, cy     principal-point offsets in NDC units (sfgs.camera.projection);
  fovy_scale fovy = fovy_scale x the equal-focal-length fovy: fx != fy;
  fill       the NDC half-extent the centres fill: > 1.3 puts visible splats beyond the Jacobian's guard band;
  zrange     down to the tz > 0.2 cull and below it;
  behind     a leading share of the points mirrored to -z (behind the camera).

Points are drawn in camera space as ((u_x - cx) z tanfovx, (u_y - cy) z tanfovy, z), u ~ U(-fill, fill)^2, z ~ U(zrange), so
that their NDC position is u whatever the principal point, moved to the world by p R^T + C in float64 and cast to float32.
Scales, quaternions, opacities and colours / SH are drawn as sfgs.synth.scene draws them. Everything is seeded and
float32: every backend sees the same bits.
"""
import math

import numpy as np
import torch

from sfgs.camera import fovy_from_fovx, make_frame

GUARD = 1.3          # the guard band of the EWA Jacobian, in units of tanfov (raster_math.h: ewa_jacobian)
NEAR = 0.2           # the near cull: visible needs tz > NEAR
NEAR_BAND = 0.3      # "just above the cull": NEAR < tz < NEAR_BAND


def _rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]),
            "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


POSE_R = _rot("z", 37.0) @ _rot("x", 25.0) @ _rot("y", -15.0)     # camera-to-world
POSE_C = np.array([12.0, -7.0, 3.0])

# the cases at GPU size (one forward + backward each, well under a second of GPU work)
CASES = {
    "pose_offcentre_sh3": dict(n=4000, W=200, H=120, cx=0.12, cy=-0.08, mode="sh", sh_degree=3, zrange=(4., 8.),
                               scale_range=(0.01, 0.2)),
    "modifier_0p8": dict(n=3000, W=200, H=120, scale_modifier=0.8, zrange=(4., 8.), scale_range=(0.01, 0.2)),
    "modifier_1p7_sh1": dict(n=3000, W=130, H=77, scale_modifier=1.7, mode="sh", sh_degree=1, zrange=(4., 8.),
                             scale_range=(0.01, 0.2)),
    "anamorphic": dict(n=3000, W=200, H=120, fovy_scale=1.25, cx=0.05, zrange=(4., 8.), scale_range=(0.01, 0.2)),
    "clamped_jacobian": dict(n=600, W=256, H=192, fill=1.6, zrange=(3., 6.), scale_range=(0.3, 1.5),
                             opacity_range=(0.02, 0.3)),
    "near_plane": dict(n=4000, W=160, H=100, zrange=(0.15, 1.2), scale_range=(0.003, 0.03)),
    "behind_camera": dict(n=4000, W=160, H=100, behind=0.4, zrange=(0.5, 6.), scale_range=(0.01, 0.2), mode="sh",
                          sh_degree=2),
}
# every other case: seed 3. clamped_jacobian masks 1.07 % of its pixels at seed 3 (tests/grad_bounds.py: MASK_CAP = 1 %,
# "another seed, never another cap"); seed 4, the next one, masks 0.87 %
SEEDS = {"clamped_jacobian": 4}


def camera_scene(n, W, H, seed=3, zrange=(4., 8.), scale_range=(0.01, 0.2), fovx_deg=60.0, fovy_scale=1.0, cx=0.0, cy=0.0,
                 scale_modifier=1.0, mode="precomp", sh_degree=1, fill=1.0, behind=0.0, opacity_range=(0.05, 0.95),
                 kernel_size=0.1):
    """(frame, g, reach): frame and g as sfgs.synth.scene returns them; reach = dict(txtz, tytz, tz) of float64 [n] arrays,
    the view-space position of every Gaussian (float32 means through the frame's float32 view matrix, in float64)."""
    gen = torch.Generator().manual_seed(seed)
    fovx = math.radians(fovx_deg)
    fovy = fovy_from_fovx(fovx, W, H) * fovy_scale
    tanx, tany = math.tan(fovx / 2), math.tan(fovy / 2)
    z = torch.empty(n).uniform_(zrange[0], zrange[1], generator=gen).double()
    u = torch.empty(n, 2).uniform_(-1.0, 1.0, generator=gen).double() * fill
    cam = torch.stack([(u[:, 0] - cx) * z * tanx, (u[:, 1] - cy) * z * tany, z], 1)
    cam[: int(round(behind * n)), 2] *= -1.0
    means = (cam @ torch.tensor(POSE_R.T) + torch.tensor(POSE_C)).float().contiguous()
    lo, hi = math.log(scale_range[0]), math.log(scale_range[1])
    scales = torch.exp(torch.empty(n, 3).uniform_(lo, hi, generator=gen))
    rots = torch.randn(n, 4, generator=gen)
    rots = rots / rots.norm(dim=1, keepdim=True)
    opac = torch.empty(n, 1).uniform_(opacity_range[0], opacity_range[1], generator=gen)
    g = dict(means3D=means, scales=scales, rotations=rots, opacities=opac, colors_precomp=None, shs=None)
    if mode == "precomp":
        g["colors_precomp"] = torch.rand(n, 3, generator=gen)
    else:
        shs = torch.randn(n, (sh_degree + 1) ** 2, 3, generator=gen)
        shs[:, 1:] *= 0.3
        g["shs"] = shs.contiguous()
    frame = make_frame(POSE_R, -POSE_R.T @ POSE_C, fovx, fovy, W, H, cx=cx, cy=cy, kernel_size=kernel_size,
                       scale_modifier=scale_modifier, sh_degree=sh_degree if mode == "sh" else 0)
    t = torch.cat([means.double(), torch.ones(n, 1, dtype=torch.float64)], 1) @ frame["view"].double()
    t = t.numpy()
    return frame, g, dict(txtz=t[:, 0] / t[:, 2], tytz=t[:, 1] / t[:, 2], tz=t[:, 2])


def case(name, **override):
    """(frame, g, reach) of a named case; `override` (n=, W=, H=) gives the CPU-sized variant of the same settings."""
    kw = dict(CASES[name], seed=SEEDS.get(name, 3))
    kw.update(override)
    return camera_scene(kw.pop("n"), kw.pop("W"), kw.pop("H"), **kw)


def clamped(frame, reach):
    """(x, y) bool [n]: in front of the near cull and beyond the guard band on that axis"""
    front = reach["tz"] > NEAR
    return (front & (np.abs(reach["txtz"]) > GUARD * frame["tanfovx"]),
            front & (np.abs(reach["tytz"]) > GUARD * frame["tanfovy"]))


def near_band(reach):
    """(visible side, culled side) bool [n]: NEAR < tz < NEAR_BAND, and 0 < tz <= NEAR"""
    tz = reach["tz"]
    return (tz > NEAR) & (tz < NEAR_BAND), (tz > 0) & (tz <= NEAR)
