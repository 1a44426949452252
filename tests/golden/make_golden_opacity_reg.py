#!/usr/bin/env python
"""Golden vectors of the opacity regulariser: the reference's REAL GaussianModel.get_opacity driven by the two statements
of train.py:239-240,

    opacity = gaussians.get_opacity.clamp(1.0e-3, 1.0 - 1.0e-3)
    opacity_loss = torch.nn.functional.binary_cross_entropy(opacity, opacity)

followed by backward(), once with a float32 `_opacity` and once with the float64 one the real reset_opacity() leaves behind
(scene/gaussian_model.py:483-501; tests/test_reset_opacity_f64.py). reset_opacity() puts every opacity at or below 0.01, so
the float64 parameter it created is then filled in place with the case's values: the dtype comes from the real method, the
spread from here.

N = 4 099 raw values: half uniform over [-12, 12], half normal(0, 2.5), resampled until none lies within 0.01 of the
clamp's thresholds |x| = 6.906755 (there the gradient jumps and the side an element falls on depends on the exp
implementation). Recorded per dtype: x, the value, `_opacity.grad`. tests/test_gpu_opacity_reg.py replays them into
sfgs.loss.opacity_entropy on the GPU.

Runs only in the authoring container (it imports /root/reference read-only, through make_golden_r2's loader).

usage: python tests/golden/make_golden_opacity_reg.py [--check]     (--check: regenerate and compare with the committed file)
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.path.join(HERE, "reference_opacity_reg.npz")
N = 4099
THRESHOLD = math.log((1.0 - 1.0e-3) / 1.0e-3)   # 6.906755: |logit| of both clamp bounds
BAND = 0.01


def raw_opacities(n, dtype, gen):
    """[n,1] raw opacities of `dtype`: uniform [-12, 12] and a normal bulk, none within BAND of +-THRESHOLD."""
    def draw(k):
        u = torch.rand(k, generator=gen, dtype=dtype) * 24.0 - 12.0
        z = torch.randn(k, generator=gen, dtype=dtype) * 2.5
        return torch.where(torch.arange(k) % 2 == 0, u, z)
    x = draw(n)
    while True:
        bad = (x.abs() - THRESHOLD).abs() < BAND
        if not bad.any():
            return x.reshape(n, 1)
        x = torch.where(bad, draw(n), x)


def generate():
    import make_golden_r2 as mg2
    mg2.mg._cpu_redirect()
    sys.path.insert(0, mg2.REF)
    gm = mg2._gaussian_model_module()
    gen = torch.Generator().manual_seed(2024)
    g = dict(means3D=torch.randn(N, 3, generator=gen) * 5, scales=torch.exp(torch.randn(N, 3, generator=gen) - 2),
             rotations=torch.randn(N, 4, generator=gen), opacities=torch.rand(N, 1, generator=gen) * 0.9 + 0.05)
    m = mg2._model_from_scene(gm, g, 0.01)
    m.filter_3D = torch.exp(torch.randn(N, 1, generator=gen, dtype=torch.float64) - 3.0)   # float64 like compute_3D_filter
    out = {}
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        if dtype == torch.float64:
            for grp in m.optimizer.param_groups:               # one Adam step: reset_opacity() replaces an EXISTING state
                for q in grp["params"]:
                    q.grad = torch.zeros_like(q)
            m.optimizer.step()
            m.optimizer.zero_grad(set_to_none=True)
            m.reset_opacity()                                  # the REAL method: `_opacity` is a float64 parameter from here on
        assert m._opacity.dtype == dtype, m._opacity.dtype
        with torch.no_grad():
            m._opacity.copy_(raw_opacities(N, dtype, gen))
        m._opacity.grad = None
        opacity = m.get_opacity.clamp(1.0e-3, 1.0 - 1.0e-3)                               # train.py:239
        opacity_loss = torch.nn.functional.binary_cross_entropy(opacity, opacity)         # train.py:240
        opacity_loss.backward()
        assert opacity_loss.dtype == dtype and m._opacity.grad.dtype == dtype
        out[f"{tag}_x"] = m._opacity.detach().numpy().copy()
        out[f"{tag}_value"] = opacity_loss.detach().numpy().copy()
        out[f"{tag}_grad"] = m._opacity.grad.numpy().copy()
    return out


def main():
    out = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert set(old.files) == set(out), set(old.files) ^ set(out)
        for k in out:
            assert old[k].dtype == out[k].dtype, k
            np.testing.assert_array_equal(old[k], out[k], err_msg=k)
        print("reference_opacity_reg.npz reproduced exactly")
        return
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
