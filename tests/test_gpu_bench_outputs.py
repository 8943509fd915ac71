"""A plain bench.py run times the headline only and, with --dump-outputs, writes what its last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    B, N = 1024, 5
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(B),
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and line["success_rate"] > 0.99
    for k in ("batch_1024", "cpu_baseline", "config_c3", "closed_loop", "x0_first", "open_loop"):     # --full only
        assert k not in line, k
    shapes = {"xopt": (B, 3, N + 1), "uopt": (B, 2, N), "ts_opt": (B,), "status": (B,), "iters": (B,), "info": (B, 4)}
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in shapes)
    out = {k: np.load(os.path.join(tmp_path, k + ".npy")) for k in shapes}
    for k, shp in shapes.items():
        assert out[k].dtype == np.float64 and out[k].shape == shp, (k, out[k].dtype, out[k].shape)
    ok = np.isin(out["status"], (0, 1))
    assert ok.mean() == pytest.approx(line["success_rate"])
    assert np.all(np.isfinite(out["xopt"][ok])) and np.all(out["ts_opt"][ok] > 0)
