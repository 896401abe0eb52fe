"""complete_point_ddpm.py end to end on one GPU with the synthetic-weights fallback: cut clouds in, completions out."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_complete_point_ddpm_script(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "complete_point_ddpm.py"), "--num-samples", "2", "--num-points", "128",
                        "--steps", "12", "--resample", "2", "--jump", "4", "--out", str(tmp_path / "o")], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(tmp_path / "o" / "completions.npz")
    partial, counts, done = z["partial"], z["counts"], z["completion"]
    assert partial.shape == done.shape == (2, 128, 3) and counts.shape == (2,) and np.isfinite(done).all()
    assert z["metrics"].shape == (2, 3) and np.isfinite(z["metrics"][:, 0]).all()
    assert ((0 < counts) & (counts < 128)).all()                       # a cut through the cloud: ragged, neither empty nor whole
    for b, c in enumerate(counts):
        assert np.array_equal(done[b, :c], partial[b, :c])
        assert (partial[b, :c, 0] < 0.0).all() and not np.array_equal(done[b, c:], partial[b, c:])
    log = open(tmp_path / "test" / "logs" / "point_ddpm_complete.log").read()
    assert "Average Chamfer Distance between completion and original" in log
