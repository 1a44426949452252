"""bench.py's plain run: it times exactly --steps steps, prints the headline without the --full measurements, and
--dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    N, W, H = 100_000, 640, 360
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(N), "--width", str(W),
                        "--height", str(H), "--steps", "7", "--warmup", "2", "--prewarm-steps", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["full"] is False
    assert line["unit"] == "Gaussians/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] - N / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    for key in ("box", "train_shaped", "roofline", "roofline_step", "cpu_baseline", "allreduce_ms_per_step"):
        assert line[key] is None, key
    z = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(z) == ["alpha", "color", "depth", "grad_colors_precomp", "grad_means2D", "grad_means3D", "grad_opacities",
                         "grad_rotations", "grad_scales", "radii"]
    assert all(a.dtype == np.float32 for a in z.values())
    assert z["color"].shape == (3, H, W) and z["alpha"].shape == (1, H, W) and z["radii"].shape == (N,)
    assert np.isfinite(z["color"]).all() and z["alpha"].max() > 0 and (z["radii"] > 0).any()
    for k, a in z.items():
        if k.startswith("grad_"):
            assert a.shape[0] == N and np.isfinite(a).all() and np.abs(a).max() > 0, k
