"""The mesh flags of the point-cloud entry points end to end on one GPU, each in a child process with the synthetic-weights fallback:
`--mesh-dir` / `--mesh-resolution` / `--mesh-format` of `generate_point_ddpm.py` and `complete_point_ddpm.py`.  The files read back as closed
meshes (empty ones are allowed: two-step noise clouds promise nothing more), and the arrays the scripts store are what they store without the
flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _check_meshes(mesh_dir, ext, count):
    from shapegen_amd.utils import load_mesh, mesh_is_closed
    assert sorted(os.listdir(mesh_dir)) == [f"sample_{i}.{ext}" for i in range(count)]
    for i in range(count):
        mesh = load_mesh(os.path.join(mesh_dir, f"sample_{i}.{ext}"))
        v, f = mesh.vertices.numpy(), mesh.faces.numpy()
        assert v.ndim == 2 and v.shape[1] == 3 and f.ndim == 2 and f.shape[1] == 3 and mesh_is_closed(mesh)
        assert f.size == 0 or (f.min() >= 0 and f.max() < v.shape[0] and np.isfinite(v).all())


def test_generate_point_ddpm_writes_meshes(tmp_path):
    base = [os.path.join(ROOT, "generate_point_ddpm.py"), "--num-samples", "2", "--num-points", "256", "--steps", "2"]
    _run(base + ["--out", str(tmp_path / "plain")], str(tmp_path))
    plain = np.load(tmp_path / "plain" / "generated.npz")
    _run(base + ["--out", str(tmp_path / "m"), "--mesh-dir", str(tmp_path / "mesh"), "--mesh-resolution", "16"], str(tmp_path))
    z = np.load(tmp_path / "m" / "generated.npz")
    assert sorted(z.files) == sorted(plain.files) == ["sampler", "samples", "steps"]
    for key in plain.files:
        assert np.array_equal(z[key], plain[key]), key
    assert sorted(os.listdir(tmp_path / "m")) == ["generated.npz"]
    _check_meshes(tmp_path / "mesh", "obj", 2)
    log = open(tmp_path / "test" / "logs" / "point_ddpm_generate.log").read()
    assert "mesh 0:" in log and "mesh 1:" in log and "enclosed nodes" in log


def test_complete_point_ddpm_writes_meshes(tmp_path):
    base = [os.path.join(ROOT, "complete_point_ddpm.py"), "--num-samples", "2", "--num-points", "128", "--steps", "12", "--resample", "2", "--jump", "4"]
    _run(base + ["--out", str(tmp_path / "plain")], str(tmp_path))
    plain = np.load(tmp_path / "plain" / "completions.npz")
    _run(base + ["--out", str(tmp_path / "m"), "--mesh-dir", str(tmp_path / "mesh"), "--mesh-resolution", "16", "--mesh-format", "ply"], str(tmp_path))
    z = np.load(tmp_path / "m" / "completions.npz")
    assert sorted(z.files) == sorted(plain.files) == ["completion", "counts", "metrics", "partial"]
    for key in plain.files:
        assert np.array_equal(z[key], plain[key], equal_nan=True), key
    _check_meshes(tmp_path / "mesh", "ply", 2)
    log = open(tmp_path / "test" / "logs" / "point_ddpm_complete.log").read()
    assert "mesh 0:" in log and "mesh 1:" in log
