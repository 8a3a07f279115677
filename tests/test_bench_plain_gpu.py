"""
The plain bench line (`bench.py --gpus 1 --steps K --warmup W`, no --full): exactly K timed steps, ms_per_step of one of them, none of
the --full legs, and --dump-outputs writing the state the last timed step left.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--burnin", "3", "--docs", "3000",
           "--clock-warmup", "0", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == 7 and r["warmup"] == 2 and r["n_gpus"] == 1 and r["unit"] == "VB iters/sec" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["value"] > 0 and r["ms_per_step"] == pytest.approx(1e3 / r["value"], rel=1e-5)
    assert r["roofline"]["estep_ms"] > 0
    assert r["cpu_baseline"] is None and r["parity"] is None
    assert "cold_start" not in r and "elbo_plateau" not in r and "other_configs" not in r and "multi_gpu_check" not in r
    K, V, M = 50, 25319, 3000
    alpha, beta = np.load(out_dir / "alpha.npy"), np.load(out_dir / "beta.npy")
    gamma, elog = np.load(out_dir / "gamma.npy"), np.load(out_dir / "Elogtheta.npy")
    assert alpha.dtype == np.float64 and alpha.shape == (K,) and np.all(alpha > 0)
    for a, shape in ((beta, (K, V)), (gamma, (K, M)), (elog, (K, M))):
        assert a.dtype == np.float32 and a.shape == shape and np.all(np.isfinite(a))
    assert np.allclose(beta.sum(axis=1, dtype=np.float64), 1.0, rtol=1e-4)
    assert np.all(gamma > 0) and np.all(elog < 0)
    assert sum(os.path.getsize(out_dir / f) for f in os.listdir(out_dir)) <= 64 * 1024 * 1024
