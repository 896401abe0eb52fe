"""`process_meshes.py` with the simplification flags, run once as a script on two small files: the files read back within the face budget,
closed if they went in closed, and the report carries the grid resolution the bisection chose; and `generate_mesh_ldm.py` with a grid
resolution against the same run without one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_ops_statement as S
import mesh_simplify_cases as C
import mesh_simplify_statement as Q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(script, *args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + [str(a) for a in args], cwd=str(cwd), env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_generate_mesh_ldm_with_a_grid_resolution(tmp_path):
    """One run (the script's cost is building the model): a 6^3 grid leaves at most 216 vertices a mesh where surface nets at 32^3 write
    thousands, every one a mean of decoded vertices and so inside their cube, every face with three different vertices."""
    from shapegen_amd import utils
    run("generate_mesh_ldm.py", "--num-samples", 2, "--steps", 2, "--format", "ply", "--out", tmp_path / "m", "--simplify-resolution", 6,
        "--placement", "mean", cwd=tmp_path)
    for i in range(2):
        got = utils.load_mesh(str(tmp_path / "m" / f"mesh_{i}.ply"))
        v, f = got.vertices.numpy(), got.faces.numpy()
        assert 0 < v.shape[0] <= 216 and f.shape[0] > 0 and f.min() >= 0 and f.max() < v.shape[0]
        assert np.isfinite(v).all() and np.abs(v).max() <= 1.0 + 2.0 / 31.0          # the [-1, 1] cube and one voxel pitch round it
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()


def test_process_meshes_script_with_a_face_budget(tmp_path):
    from shapegen_amd import utils
    src, budget = tmp_path / "in", 120
    for name, ext in (("mixed", ".obj"), ("icosphere_642", ".ply")):
        v, f = C.case(name)
        utils.save_mesh(str(src / (name + ext)), (torch.from_numpy(v.copy()), torch.from_numpy(f.copy())))
    r = run("process_meshes.py", src, tmp_path / "out", "--target-faces", budget, "--keep-largest", "--smooth", 2, "--normals", "--format", "ply",
            "--report", tmp_path / "report.json", cwd=tmp_path)
    report = json.load(open(tmp_path / "report.json"))
    assert sorted(report) == ["icosphere_642", "mixed"]
    for name in report:
        v, f = utils.load_mesh(str(src / (name + (".obj" if name == "mixed" else ".ply"))))      # the bits the script read
        v, f = v.numpy(), f.numpy()
        kv, kf = S.compact(v, f, S.keep_flags(v.shape[0], f, keep_largest=True))
        want = Q.simplify(kv, kf, target_faces=budget)
        back = utils.load_mesh(str(tmp_path / "out" / (name + ".ply")))
        assert report[name]["resolution"] == want["resolution"] and f"grid {want['resolution']}^3" in r.stdout
        assert np.array_equal(back.faces.numpy(), want["faces"]) and back.faces.shape[0] <= budget
        assert np.array_equal(back.vertices.numpy().view(np.uint32), S.smooth(want["vertices"], want["faces"], 2, 0.5, -0.53).view(np.uint32))
        assert S.measures(kv, kf)["closed"] == 1 and S.measures(back.vertices.numpy(), back.faces.numpy())["closed"] == 1
        assert report[name]["after"]["closed"] == 1 and report[name]["after"]["faces"] == back.faces.shape[0]
        pts, nrm = utils.load_point_cloud(str(tmp_path / "out" / (name + ".ply")))
        assert nrm.shape == back.vertices.shape
    assert report["mixed"]["resolution"] == 1024 and report["mixed"]["after"]["faces"] == 12     # the cube is within the budget as it is
