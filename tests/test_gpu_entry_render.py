"""The picture-writing entry points end to end on one GPU, each in a child process: `render_shapes.py` on a tiny `.npz`, and
`generate_point_ddpm.py --png-dir` with the synthetic-weights fallback.  The PNGs are decoded with zlib alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

import render_statement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _png(path):
    with open(path, "rb") as src:
        return S.decode_png(src.read())


def test_render_shapes_script(tmp_path):
    g = np.random.default_rng(0)
    grid = np.zeros((2, 1, 8, 8, 8), np.float32)
    grid[:, 0, 2:6, 2:6, 2:6] = 1.0
    np.savez(tmp_path / "tiny.npz", generated=g.uniform(-0.8, 0.8, (3, 64, 3)).astype(np.float32), metrics=np.zeros((3, 3), np.float32), vox=grid)
    out = _run([os.path.join(ROOT, "render_shapes.py"), str(tmp_path / "tiny.npz"), "--views", "2", "--size", "40", "--radius", "2", "--out",
                str(tmp_path / "p")], str(tmp_path))
    assert "wrote 5 PNG" in out and sorted(os.listdir(tmp_path / "p")) == [f"tiny_generated_{i}.png" for i in range(3)] + ["tiny_vox_0.png", "tiny_vox_1.png"]
    for name in os.listdir(tmp_path / "p"):
        im = _png(tmp_path / "p" / name)
        assert im.shape == (40, 80, 3) and (im == 255).all(axis=-1).any() and (im != 255).any(), name       # two views side by side, drawn on white
    _run([os.path.join(ROOT, "render_shapes.py"), str(tmp_path / "tiny.npz"), "--size", "32", "--grid", "2", "--arrays", "generated", "--out",
          str(tmp_path / "g")], str(tmp_path))
    assert os.listdir(tmp_path / "g") == ["tiny_generated.png"] and _png(tmp_path / "g" / "tiny_generated.png").shape == (64, 64, 3)


def test_generate_point_ddpm_png_dir(tmp_path):
    _run([os.path.join(ROOT, "generate_point_ddpm.py"), "--num-samples", "2", "--num-points", "256", "--steps", "2", "--out", str(tmp_path / "o"),
          "--png-dir", str(tmp_path / "png")], str(tmp_path))
    assert np.load(tmp_path / "o" / "generated.npz")["samples"].shape == (2, 256, 3)
    assert sorted(os.listdir(tmp_path / "png")) == ["sample_0_2d.png", "sample_0_3d.png", "sample_1_2d.png", "sample_1_3d.png"]
    for i in range(2):
        assert _png(tmp_path / "png" / f"sample_{i}_3d.png").shape == (256, 256, 3)
        assert _png(tmp_path / "png" / f"sample_{i}_2d.png").shape == (256, 768, 3)
