"""The entry points of mesh processing, each run once as a script: `process_meshes.py` on two small files with every flag, and
`generate_mesh_ldm.py` with and without its processing flags."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_ops_cases as C
import mesh_ops_statement as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(script, *args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + [str(a) for a in args], cwd=str(cwd), env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_process_meshes_script_with_every_flag(tmp_path):
    from shapegen_amd import utils
    src = tmp_path / "in"
    for name, ext in (("mixed", ".obj"), ("two_tetrahedra", ".ply")):
        v, f = C.case(name)
        utils.save_mesh(str(src / (name + ext)), (torch.from_numpy(v.copy()), torch.from_numpy(f.copy())))
    run("process_meshes.py", src, tmp_path / "out", "--smooth", 3, "--lambda", 0.5, "--mu", -0.53, "--pin-boundary", "--keep-largest",
        "--normals", "--format", "ply", "--report", tmp_path / "r" / "report.json", cwd=tmp_path)
    report = json.load(open(tmp_path / "r" / "report.json"))
    assert sorted(report) == ["mixed", "two_tetrahedra"]
    for name, first in (("mixed", 1), ("two_tetrahedra", 0)):
        v, f = C.case(name)
        # obj text holds 9 significant digits: the vertices read back are the case's bits
        kv, kf = S.compact(v, f, S.keep_flags(v.shape[0], f, keep_largest=True))
        want = S.smooth(kv, kf, 3, 0.5, -0.53, pin_boundary=True)
        back = utils.load_mesh(str(tmp_path / "out" / (name + ".ply")))
        assert np.array_equal(back.vertices.numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(back.faces.numpy(), kf)
        pts, nrm = utils.load_point_cloud(str(tmp_path / "out" / (name + ".ply")))
        assert np.array_equal(nrm.numpy().view(np.uint32), S.vertex_normals(want, kf).view(np.uint32))
        before, after = report[name]["before"], report[name]["after"]
        wb, wa = S.measures(v, f), S.measures(want, kf)
        for k in ("vertices", "edges", "faces", "boundary_edges", "irregular_edges", "components", "euler", "closed"):
            assert before[k] == wb[k] and after[k] == wa[k], (name, k)
        assert after["components"] == 1 and after["closed"] == 1 and before["components"] == (3 if name == "mixed" else 2)
        assert abs(after["volume"] - wa["volume"]) <= 1e-10 * wa["abs_volume"] and len(after["centroid"]) == 3
    # a single file, the other component rule, plain Laplacian smoothing, written by OUT's extension
    run("process_meshes.py", src / "mixed.obj", tmp_path / "one.obj", "--min-component-faces", 5, "--smooth", 1, "--mu", 0, cwd=tmp_path)
    v, f = C.case("mixed")
    kv, kf = S.compact(v, f, S.keep_flags(v.shape[0], f, min_faces=5))
    back = utils.load_mesh(str(tmp_path / "one.obj"))
    assert np.array_equal(back.vertices.numpy().view(np.uint32), S.smooth(kv, kf, 1, 0.5, 0.0).view(np.uint32))
    assert np.array_equal(back.faces.numpy(), kf) and "vn " not in open(tmp_path / "one.obj").read()


def test_generate_mesh_ldm_with_and_without_the_processing_flags(tmp_path):
    """Without the flags the script writes what it wrote before it had them: two such runs give the same files, with no normals in
    them; with the flags every mesh is one component, smoothed, and carries normals."""
    from shapegen_amd import utils
    base = ("--num-samples", 2, "--steps", 2, "--format", "obj")
    run("generate_mesh_ldm.py", *base, "--out", tmp_path / "a", cwd=tmp_path)
    run("generate_mesh_ldm.py", *base, "--out", tmp_path / "b", cwd=tmp_path)
    run("generate_mesh_ldm.py", *base, "--out", tmp_path / "c", "--smooth", 2, "--keep-largest", "--normals", cwd=tmp_path)
    for i in range(2):
        plain = open(tmp_path / "a" / f"mesh_{i}.obj", "rb").read()
        assert plain == open(tmp_path / "b" / f"mesh_{i}.obj", "rb").read() and b"vn " not in plain and b"//" not in plain
        raw = utils.load_mesh(str(tmp_path / "a" / f"mesh_{i}.obj"))
        v, f = raw.vertices.numpy(), raw.faces.numpy()
        kv, kf = S.compact(v, f, S.keep_flags(v.shape[0], f, keep_largest=True))
        want = S.smooth(kv, kf, 2, 0.5, -0.53)
        text = open(tmp_path / "c" / f"mesh_{i}.obj").read()
        done = utils.load_mesh(str(tmp_path / "c" / f"mesh_{i}.obj"))
        assert np.array_equal(done.vertices.numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(done.faces.numpy(), kf)
        assert text.count("\nvn ") == kv.shape[0] and (kv.shape[0] == 0 or S.components(kv.shape[0], kf)[1] == 1)
