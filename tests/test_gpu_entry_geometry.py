"""The cloud-geometry flags of the entry points end to end on one GPU, each in a child process with the synthetic-weights fallback:
`--remove-outliers` / `--ply-dir` of `generate_point_ddpm.py` and `complete_point_ddpm.py`, and `render_shapes.py` on a PLY cloud.  Without
the flags the scripts write what they wrote before, under the same names and shapes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_statement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _check_plys(ply_dir, clouds, counts):
    """`sample_{i}.ply` holds the first counts[i] rows of cloud i, bit for bit, and a unit normal for each."""
    from shapegen_amd.utils import load_point_cloud
    assert sorted(os.listdir(ply_dir)) == [f"sample_{i}.ply" for i in range(len(counts))]
    for i, n in enumerate(counts):
        points, normals = load_point_cloud(os.path.join(ply_dir, f"sample_{i}.ply"))
        assert points.shape == (n, 3) and np.array_equal(points.numpy(), clouds[i, :n])
        assert normals is not None and normals.shape == (n, 3)
        assert bool(((normals.double().norm(dim=1) - 1).abs() <= 4 * 2.0 ** -24).all())


def test_generate_point_ddpm_outliers_and_ply(tmp_path):
    base = [os.path.join(ROOT, "generate_point_ddpm.py"), "--num-samples", "2", "--num-points", "256", "--steps", "2"]
    _run(base + ["--out", str(tmp_path / "plain")], str(tmp_path))
    plain = np.load(tmp_path / "plain" / "generated.npz")
    assert sorted(plain.files) == ["sampler", "samples", "steps"] and plain["samples"].shape == (2, 256, 3)
    assert sorted(os.listdir(tmp_path / "plain")) == ["generated.npz"]
    _run(base + ["--out", str(tmp_path / "o"), "--remove-outliers", "--outlier-k", "8", "--outlier-ratio", "1.0", "--ply-dir", str(tmp_path / "ply")],
         str(tmp_path))
    z = np.load(tmp_path / "o" / "generated.npz")
    assert sorted(z.files) == ["filtered", "filtered_counts", "sampler", "samples", "steps"]
    assert np.array_equal(z["samples"], plain["samples"])                     # the samples themselves are untouched
    counts = z["filtered_counts"]
    assert z["filtered"].shape == (2, 256, 3) and counts.shape == (2,) and ((0 < counts) & (counts < 256)).all()
    for i, n in enumerate(counts):
        assert not z["filtered"][i, n:].any()
        rows = {r.tobytes() for r in z["samples"][i]}
        assert all(r.tobytes() in rows for r in z["filtered"][i, :n])          # every kept row is a row of the sample
    _check_plys(tmp_path / "ply", z["filtered"], counts.tolist())
    log = open(tmp_path / "test" / "logs" / "point_ddpm_generate.log").read()
    assert "outlier removal (k 8, ratio 1.0) kept" in log
    # --ply-dir alone: the whole clouds
    _run(base + ["--out", str(tmp_path / "w"), "--ply-dir", str(tmp_path / "whole")], str(tmp_path))
    _check_plys(tmp_path / "whole", plain["samples"], [256, 256])


def test_complete_point_ddpm_outliers_and_ply(tmp_path):
    _run([os.path.join(ROOT, "complete_point_ddpm.py"), "--num-samples", "2", "--num-points", "128", "--steps", "12", "--resample", "2", "--jump", "4",
          "--out", str(tmp_path / "o"), "--remove-outliers", "--outlier-ratio", "1.0", "--ply-dir", str(tmp_path / "ply")], str(tmp_path))
    z = np.load(tmp_path / "o" / "completions.npz")
    assert sorted(z.files) == ["completion", "counts", "filtered", "filtered_counts", "metrics", "partial"]
    assert z["partial"].shape == z["completion"].shape == z["filtered"].shape == (2, 128, 3) and z["metrics"].shape == (2, 3)
    counts = z["filtered_counts"]
    assert ((0 < counts) & (counts < 128)).all()
    _check_plys(tmp_path / "ply", z["filtered"], counts.tolist())


def test_render_shapes_draws_a_ply_cloud(tmp_path):
    from shapegen_amd.utils import save_point_cloud
    g = torch.Generator().manual_seed(0)
    pts = torch.rand(200, 3, generator=g) * 1.6 - 0.8
    save_point_cloud(str(tmp_path / "cloud.ply"), pts, torch.nn.functional.normalize(pts, dim=1))
    out = _run([os.path.join(ROOT, "render_shapes.py"), str(tmp_path / "cloud.ply"), "--views", "2", "--size", "40", "--radius", "2", "--out",
                str(tmp_path / "p")], str(tmp_path))
    assert "wrote 1 PNG" in out and os.listdir(tmp_path / "p") == ["cloud_cloud_0.png"]
    with open(tmp_path / "p" / "cloud_cloud_0.png", "rb") as src:
        im = S.decode_png(src.read())
    assert im.shape == (40, 80, 3) and (im == 255).all(axis=-1).any() and (im != 255).any()
