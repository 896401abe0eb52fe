"""The surface-nets statement (tests/mesh_statement.py) pinned against cases that can be checked by hand, the mesh file writer read back by a
parser written here, and the host side of the pcd_mesh_* entry points.  No GPU."""
import ctypes as C
import math
import struct

import numpy as np
import pytest
import torch

import mesh_statement as S


def test_single_voxel_is_a_cube_of_a_third():
    """One occupied voxel in a 3^3 grid at threshold 0.5: every crossing sits half way, a corner cell's vertex is the mean of three of them:
    8 vertices at 1 +- 1/6 on every axis, 6 quads = 12 triangles, a cube of edge 1/3."""
    v = np.zeros((3, 3, 3))
    v[1, 1, 1] = 1.0
    vi, f = S.surface_nets_index(v, 0.5)
    assert vi.shape == (8, 3) and f.shape == (12, 3) and f.dtype == np.int32
    want = np.array([[1 + sz / 6, 1 + sy / 6, 1 + sx / 6] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)])
    np.testing.assert_allclose(vi, want, rtol=0, atol=1e-15)           # row-major (cz, cy, cx) order of the cells
    inv = S.mesh_invariants(vi, f)
    assert inv["closed"] and inv["chi"] == 2 and inv["max_edge_use"] == 2 and (inv["V"], inv["E"], inv["F"]) == (8, 18, 12)
    # index rows are (fz, fy, fx): an orientation-reversing relabelling of [x, y, z], so outward normals give -volume here and +volume in output rows
    assert inv["volume"] == pytest.approx(-1.0 / 27.0, abs=1e-15)
    out, _ = S.surface_nets(v, 0.5)
    assert S.mesh_invariants(out, f)["volume"] == pytest.approx(1.0 / 27.0, abs=1e-15)      # 2 / (n - 1) = 1: output units = index units
    np.testing.assert_allclose(out, want[:, ::-1] - 1.0, rtol=0, atol=1e-15)


def test_lattice_sphere_is_a_closed_manifold_of_the_right_volume():
    g = S.lattice_sphere()
    assert g.shape == (12, 12, 12) and g.dtype == np.float32
    vi, f = S.surface_nets_index(g, S.THR)
    inv = S.mesh_invariants(vi[:, ::-1], f)                              # [x, y, z] order: outward normals, positive volume
    assert inv["closed"] and inv["chi"] == 2 and inv["max_edge_use"] == 2
    assert 3 * inv["F"] == 2 * inv["E"]                                  # every edge on exactly two triangles
    ball = 4.0 / 3.0 * math.pi * 4.403 ** 3
    assert inv["volume"] > 0 and abs(inv["volume"] - ball) < 0.10 * ball, (inv["volume"], ball)
    nv, nq = S.capacities(g.shape)
    assert inv["V"] <= nv and inv["F"] <= 2 * nq


def test_two_voxels_touching_along_an_edge():
    v = np.zeros((4, 4, 4))
    v[1, 1, 1] = v[1, 2, 2] = 1.0
    vi, f = S.surface_nets_index(S.lattice(v), S.THR)
    inv = S.mesh_invariants(vi[:, ::-1], f)
    assert inv["closed"] and inv["max_edge_use"] == 4 and inv["volume"] > 0


def test_checkerboard_counts_stay_within_the_capacities():
    g = S.checkerboard((4, 4, 4))
    vi, f = S.surface_nets_index(g, S.THR)
    nv, nq = S.capacities(g.shape)
    assert (nv, nq) == (125, 240)
    assert vi.shape[0] == 121 and f.shape[0] == 2 * 192                  # the four empty corner cells; 144 interior edges + 48 to the padding
    inv = S.mesh_invariants(vi[:, ::-1], f)
    assert inv["closed"] and inv["volume"] > 0


def test_full_grid_is_the_box_half_a_voxel_larger():
    v = np.ones((3, 4, 5))
    vi, f = S.surface_nets_index(v, 0.5)
    for axis, n in enumerate(v.shape):
        assert vi[:, axis].min() == -0.5 and vi[:, axis].max() == n - 0.5
    inv = S.mesh_invariants(vi[:, ::-1], f)
    assert inv["closed"] and inv["chi"] == 2 and inv["max_edge_use"] == 2
    assert 2 * 3 * 4 < inv["volume"] < 3 * 4 * 5                         # inside the box (edges and corners are cut), outside the box a voxel smaller
    out, _ = S.surface_nets(v, 0.5)                                      # half a pitch outside [-1, 1]
    np.testing.assert_allclose(out.max(axis=0), [1 + 0.5 * 2 / 4, 1 + 0.5 * 2 / 3, 1 + 0.5 * 2 / 2], rtol=0, atol=1e-15)


def test_lattice_builder_refuses_inputs_that_could_blur_a_comparison():
    with pytest.raises(AssertionError):
        S.lattice(np.full((2, 2, 2), 0.3))                               # no multiple of 1/64
    with pytest.raises(AssertionError):
        S.lattice(np.full((2, 2, 2), 0.5), thr=0.5)                      # on the threshold
    with pytest.raises(AssertionError):
        S.lattice(np.full((2, 2, 2), 0.5), thr=0.3)                      # threshold not exact in fp32
    assert S.lattice_random((3, 5, 9), 0).shape == (3, 5, 9)


# ------------------------------------------------------------------ files
def _read_obj(path):
    v, f = [], []
    for line in open(path):
        tok = line.split()
        if tok and tok[0] == "v":
            v.append([float(t) for t in tok[1:4]])
        elif tok and tok[0] == "f":
            f.append([int(t.split("/")[0]) - 1 for t in tok[1:4]])
    return np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elems = [l.split() for l in lines if l.startswith("element")]
    assert [e[1] for e in elems] == ["vertex", "face"]
    props = [l for l in lines if l.startswith("property")]
    assert props == ["property float x", "property float y", "property float z", "property list uchar int vertex_indices"]
    nv, nf = int(elems[0][2]), int(elems[1][2])
    v = np.frombuffer(body[:12 * nv], dtype="<f4").reshape(nv, 3)
    f, at = [], 12 * nv
    for _ in range(nf):
        assert body[at] == 3
        f.append(struct.unpack_from("<3i", body, at + 1))
        at += 13
    assert at == len(body)
    return v, np.asarray(f, np.int64).reshape(-1, 3)


def test_save_mesh_round_trip(tmp_path):
    from shapegen_amd.utils import Mesh, mesh_is_closed, save_mesh
    v = np.zeros((3, 3, 3))
    v[1, 1, 1] = 1.0
    out, f = S.surface_nets(v, 0.5)
    mesh = Mesh(torch.from_numpy(out.astype(np.float32)), torch.from_numpy(f))
    assert mesh.faces.dtype == torch.int32 and mesh_is_closed(mesh)
    assert not mesh_is_closed(Mesh(mesh.vertices, mesh.faces[:-1]))
    save_mesh(str(tmp_path / "a" / "cube.obj"), mesh)
    save_mesh(str(tmp_path / "cube.ply"), mesh)
    vo, fo = _read_obj(tmp_path / "a" / "cube.obj")
    vp, fp = _read_ply(tmp_path / "cube.ply")
    assert np.array_equal(fo, f) and np.array_equal(fp, f)
    assert vp.dtype == np.float32 and np.array_equal(vp.view(np.uint32), mesh.vertices.numpy().view(np.uint32))
    assert np.array_equal(vo.astype(np.float32), mesh.vertices.numpy())          # 9 significant digits carry a float32
    first = open(tmp_path / "a" / "cube.obj").read().split("\n")
    assert first[1].startswith("v ") and min(int(t) for l in first if l.startswith("f ") for t in l.split()[1:]) == 1
    empty = Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    save_mesh(str(tmp_path / "empty.ply"), empty)
    assert _read_ply(tmp_path / "empty.ply")[0].shape == (0, 3) and mesh_is_closed(empty)
    with pytest.raises(ValueError):
        save_mesh(str(tmp_path / "cube.stl"), mesh)


# ------------------------------------------------------------------ the C ABI without a device
def test_mesh_entry_points_without_gpu():
    from shapegen_amd import _lib
    lib = _lib.load()
    assert lib.pcd_mesh_workspace_bytes(7, 32, 32, 32) == 7 * 33 ** 3 * 4
    assert lib.pcd_mesh_workspace_bytes(2, 3, 5, 9) == 2 * 4 * 6 * 10 * 4
    assert lib.pcd_mesh_workspace_bytes(0, 32, 32, 32) == 0 and lib.pcd_mesh_workspace_bytes(1, 1, 32, 32) == 0
    p = 64                                                               # never dereferenced: the checks come before any device work
    assert lib.pcd_mesh_count(None, 1, 8, 8, 8, 0.5, p, p, None) == -1 and b"bad argument" in lib.pcd_last_error()
    assert lib.pcd_mesh_count(p, 1, 8, 8, 8, 0.5, None, p, None) == -1
    assert lib.pcd_mesh_count(p, 1, 8, 8, 8, 0.5, p, None, None) == -1
    assert lib.pcd_mesh_count(p, 1, 8, 8, 8, 0.0, p, p, None) == -1
    assert lib.pcd_mesh_count(p, 1, 8, 8, 8, -0.5, p, p, None) == -1
    assert lib.pcd_mesh_count(p, 1, 8, 8, 8, float("inf"), p, p, None) == -1
    assert lib.pcd_mesh_count(p, 1, 8, 8, 8, float("nan"), p, p, None) == -1
    assert lib.pcd_mesh_count(p, 1, 1, 8, 8, 0.5, p, p, None) == -1
    assert lib.pcd_mesh_count(p, 0, 8, 8, 8, 0.5, p, p, None) == -1
    assert lib.pcd_mesh_emit(p, 1, 8, 8, 8, 0.5, p, p, p, None, None) == -1
    assert lib.pcd_mesh_emit(p, 1, 8, 8, 1, 0.5, p, p, p, p, None) == -1
    assert lib.pcd_mesh_emit(p, 1, 8, 8, 8, 0.0, p, p, p, p, None) == -1
    assert lib.pcd_mesh_config(2) == -1 and lib.pcd_mesh_config(1) == 0


def test_python_surface_refuses_cpu_tensors_and_unknown_outputs():
    from shapegen_amd.utils import voxel_tensor_to_meshes
    with pytest.raises(RuntimeError):
        voxel_tensor_to_meshes(torch.zeros(1, 1, 4, 4, 4))
    from shapegen_amd.diffusion import LatentDiffusion
    bare = object.__new__(LatentDiffusion)                               # no weights: the value is checked before the module is touched
    for name in ("sample", "sample2", "sample3", "sample_dpm"):
        with pytest.raises(ValueError, match="output must be 'points' or 'mesh'"):
            getattr(bare, name)(1, output="voxels")
