"""`evaluate_meshes.py` end to end on one GPU, in a child process: two directories of small `.obj` cubes paired by stem."""
import json
import os
import subprocess
import sys

import pytest

import mesh_in_statement as MS
from mesh_data_statement import write_obj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_evaluate_meshes_script(tmp_path):
    gen, ref = tmp_path / "gen", tmp_path / "ref"
    gen.mkdir()
    ref.mkdir()
    same = MS.cube((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    write_obj(gen / "same.obj", same)
    write_obj(ref / "same.obj", same)
    write_obj(gen / "shifted.obj", MS.cube((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)))
    write_obj(ref / "shifted.obj", MS.cube((-0.25, -0.5, -0.5), (0.75, 0.5, 0.5)))
    write_obj(gen / "nested.obj", MS.cube((-0.75, -0.75, -0.75), (0.75, 0.75, 0.75)))
    write_obj(ref / "nested.obj", MS.cube((-0.25, -0.25, -0.25), (0.25, 0.25, 0.25)))
    write_obj(gen / "lonely.obj", same)                                      # no partner in ref
    out = _run([os.path.join(ROOT, "evaluate_meshes.py"), str(gen), str(ref), "--num-points", "4000", "--resolution", "16", "--batch", "2",
                "--out", str(tmp_path / "scores" / "eval.json")], str(tmp_path))
    assert "unpaired, skipped: lonely" in out and "3 pair(s)" in out
    with open(tmp_path / "scores" / "eval.json") as f:
        got = json.load(f)
    cols = got["columns"]
    assert cols[:10] == ["ACC", "COMP", "CHAMFER_L1", "ACC2", "COMP2", "CHAMFER_L2", "HAUSDORFF", "NC_A", "NC_B", "NC"]
    assert cols[10:] == [f"{k}@{t}" for t in ("0.02", "0.04", "0.1") for k in ("PRECISION", "RECALL", "FSCORE")] + ["IOU"]
    assert got["stems"] == ["nested", "same", "shifted"] and got["unpaired"] == ["lonely"]
    assert len(got["rows"]) == 3 and all(len(r) == len(cols) for r in got["rows"])
    row = {s: dict(zip(cols, r)) for s, r in zip(got["stems"], got["rows"])}
    assert row["same"]["IOU"] == 1.0 and row["same"]["FSCORE@0.1"] == 1.0 and row["same"]["NC"] > 0.8
    assert 0.0 < row["shifted"]["IOU"] < 1.0 and row["shifted"]["FSCORE@0.1"] < 1.0 and row["shifted"]["HAUSDORFF"] >= 0.25
    assert 0.0 < row["nested"]["IOU"] < row["shifted"]["IOU"] and row["nested"]["FSCORE@0.1"] == 0.0
    for name in cols:
        assert name in out
    # two single files are a pair whatever they are called
    out = _run([os.path.join(ROOT, "evaluate_meshes.py"), str(gen / "lonely.obj"), str(ref / "same.obj"), "--num-points", "500", "--resolution",
                "0", "--thresholds", "0.3", "--normalize"], str(tmp_path))
    assert "1 pair(s)" in out and "FSCORE@0.3" in out and "IOU" in out and "(1 of 1 NaN)" in out
