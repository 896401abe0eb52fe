"""Mesh input on the GPU (csrc/mesh_in.hip through `utils.meshes_to_voxel_tensor` and `utils.sample_mesh_points`) against the float64 statement
(tests/mesh_in_statement.py), the round trip with the surface-nets kernel, repeatability, the refusals and the preprocessing script.

Exact lattice: R = 8, bounds (0, 7) (index = coordinate, inv_pitch exactly 1), vertices multiples of 1/2 in [-1, 8]: every product and sum of the
predicates fits 24 bits (differences 6, products 12, normal 13, plane dot 21), so fp32 decides every tie as float64 does and nothing is left out.
Round trip: every surface-nets quad is pierced once by the grid edge it is dual to and by no other grid line, and for binary fields its vertices lie
at least 1/24 of a pitch inside the four cells round that edge, five orders above the fp32 coordinate rounding: interior(mesh(g)) == g exactly.
Conditioned random triangles (surface only): voxels whose statement margin is below 1e-4 -- a thousand times the fp32 rounding of a predicate
whose terms are below 2^11 in index units -- are left out, at most 1 % of a mesh's voxels (the share itself is asserted on the CPU, in
test_mesh_in_statement_cpu.py).  Sampling: face indices equal the statement's except within 1e-5 x total of a running-sum boundary (the device's
sums are fp32; expected share 2e-5 F <= 0.5 %, at most 2 % may be left out); points and normals within 1e-5 absolute (coordinates below 2, about
six roundings; a wrong vertex moves a point by 1e-2 or more).

The statements run once per module and are left unchanged."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_in_statement as S
import mesh_statement as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FILLS = ("surface", "interior", "solid")
MARGIN = 1e-4
SQUARE = (np.asarray([(1.5, 1.5, 2.5), (2.5, 1.5, 2.5), (2.5, 2.5, 2.5), (1.5, 2.5, 2.5)]), np.asarray([(0, 1, 2), (0, 2, 3)], np.int32))
THROUGH = (np.asarray([(0.0, 0.0, 3.0), (6.0, 0.0, 3.0), (0.0, 6.0, 3.0)]), np.asarray([(0, 1, 2)], np.int32))


def dev(mesh):
    from shapegen_amd.utils import Mesh
    v, f = mesh
    return Mesh(torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda())


def voxelize(meshes, r, fill, bounds=(-1.0, 1.0)):
    from shapegen_amd.utils import meshes_to_voxel_tensor
    out = meshes_to_voxel_tensor([dev(m) for m in meshes], r, fill=fill, bounds=bounds)
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == (len(meshes), 1, r, r, r)
    assert bool(((out == 0) | (out == 1)).all())
    return out[:, 0].cpu().numpy() > 0.5


# ------------------------------------------------------------------ 1. the exact lattice
def lattice_meshes():
    return [SQUARE, THROUGH, S.cube(1.5, 4.5), S.merge(S.cube(1.5, 4.5), S.cube(2.5, 5.5)), S.cube(1.5, 4.5, inside_out=True), S.lattice_triangles(40, 0)]


@pytest.fixture(scope="module")
def lattice_reference():
    out = []
    for v, f in lattice_meshes():
        assert np.array_equal(np.round(v * 2.0), v * 2.0) and v.min() >= -1.0 and v.max() <= 8.0
        surface, interior = S.voxelize_surface(v, f, 8), S.voxelize_interior(v, f, 8)
        out.append({"surface": surface, "interior": interior, "solid": surface | interior})
    return out


@pytest.mark.parametrize("fill", FILLS)
def test_lattice_meshes_equal_the_statement_voxel_for_voxel(lattice_reference, fill):
    got = voxelize(lattice_meshes(), 8, fill, bounds=(0.0, 7.0))
    for i, want in enumerate(lattice_reference):
        print(f"{fill}[{i}]: device {int(got[i].sum())} statement {int(want[fill].sum())} differ {int((got[i] != want[fill]).sum())}")
        assert np.array_equal(got[i], want[fill]), (fill, i, np.argwhere(got[i] != want[fill])[:8].tolist())
    assert int(lattice_reference[0]["surface"].sum()) == 18 and int(lattice_reference[1]["interior"].sum()) == 63      # the cases worked by hand
    assert int(lattice_reference[5]["surface"].sum()) > 100


def chunked_lattice_mesh():
    """1025 small triangles on the lattice of halves: one more than a chunk of 1024.  The first 1024 stay below index 6; the last one lies alone
    at z = 6.5 over the nodes (6, 6), so surface and interior both change if the chunk that holds only this triangle is lost."""
    g = np.random.default_rng(7)
    v = g.integers(0, 10, size=(1024, 1, 3)) / 2.0 + g.integers(-1, 3, size=(1024, 3, 3)) / 2.0
    v = np.concatenate([v, np.asarray([[(5.5, 5.5, 6.5), (7.0, 5.5, 6.5), (5.5, 7.0, 6.5)]])]).reshape(-1, 3)
    return v, np.arange(3 * 1025, dtype=np.int32).reshape(-1, 3)


def test_a_lattice_mesh_of_1025_triangles_equals_the_statement():
    v, f = chunked_lattice_mesh()
    assert np.array_equal(np.round(v * 2.0), v * 2.0) and v.min() >= -1.0 and v.max() <= 8.0
    want = {"surface": S.voxelize_surface_vec(v, f, 8)[0], "interior": S.voxelize_interior_vec(v, f, 8)[0]}
    want["solid"] = want["surface"] | want["interior"]
    assert v[:-3].max() <= 5.5 and np.argwhere(want["surface"]).max() == 7         # index 7 is reached by the last triangle alone
    assert (want["interior"] != S.voxelize_interior_vec(v, f[:1024], 8)[0]).sum() >= 4
    for fill in FILLS:
        got = voxelize([(v, f)], 8, fill, bounds=(0.0, 7.0))[0]
        print(f"{fill}: device {int(got.sum())} statement {int(want[fill].sum())} differ {int((got != want[fill]).sum())}")
        assert np.array_equal(got, want[fill]), (fill, np.argwhere(got != want[fill])[:8].tolist())
    assert 0 < int(want["solid"].sum()) < 512


# ------------------------------------------------------------------ 2. round trip with the surface-nets kernel
def r5_grids():
    """Small shapes in 5^3 whose meshes have at most 256 faces (the sampler's inputs too)."""
    one = np.zeros((5, 5, 5), np.float32)
    one[2, 1, 3] = 1
    block = np.zeros((5, 5, 5), np.float32)
    block[0:2, 3:5, 1:3] = 1
    plus = np.zeros((5, 5, 5), np.float32)
    plus[2, 2, 1:4] = plus[2, 1:4, 2] = plus[1:4, 2, 2] = 1
    ell = np.zeros((5, 5, 5), np.float32)
    ell[4, 0:4, 0] = ell[4, 0, 0:3] = ell[1:5, 0, 0] = 1
    return [one, block, plus, ell]


def binary_grids(name):
    if name == "r32":
        n = 32
        zz, yy, xx = np.meshgrid(*[np.arange(n)] * 3, indexing="ij")
        corners = np.zeros((n, n, n), np.float32)
        corners[0, 0, 0] = corners[n - 1, n - 1, n - 1] = corners[0, n - 1, 0] = 1
        sphere = ((zz - 15.3) ** 2 + (yy - 15.6) ** 2 + (xx - 15.9) ** 2 <= 11.2 ** 2).astype(np.float32)
        rnd = (np.random.default_rng(0).random((n, n, n)) < 0.5).astype(np.float32)
        return [M.checkerboard((n, n, n)), np.zeros((n, n, n), np.float32), np.ones((n, n, n), np.float32), corners, rnd, sphere]
    if name == "r2":
        return [np.ones((2, 2, 2), np.float32), (np.random.default_rng(2).random((2, 2, 2)) < 0.5).astype(np.float32), np.zeros((2, 2, 2), np.float32),
                M.checkerboard((2, 2, 2))]
    if name == "r5":
        return r5_grids() + [(np.random.default_rng(5).random((5, 5, 5)) < 0.5).astype(np.float32), np.ones((5, 5, 5), np.float32)]
    n = int(name[1:])                                              # above 32 the accumulators live in the workspace, not in LDS
    zz, yy, xx = np.meshgrid(*[np.arange(n)] * 3, indexing="ij")
    sphere = ((zz - n * 0.48) ** 2 + (yy - n * 0.5) ** 2 + (xx - n * 0.53) ** 2 <= (n * 0.36) ** 2).astype(np.float32)
    return [sphere, (np.random.default_rng(n).random((n, n, n)) < 0.3).astype(np.float32)]


def device_meshes(grids):
    from shapegen_amd.utils import voxel_tensor_to_meshes
    return voxel_tensor_to_meshes(torch.from_numpy(np.stack(grids)[:, None]).cuda(), 0.5)


@pytest.mark.parametrize("name", ["r32", "r2", "r5", "r33", "r64"])
def test_round_trip_with_the_surface_nets_kernel(name):
    from shapegen_amd.utils import meshes_to_voxel_tensor
    grids = binary_grids(name)
    r = grids[0].shape[0]
    meshes = device_meshes(grids)
    want = np.stack(grids) > 0.5
    got = {fill: meshes_to_voxel_tensor(meshes, r, fill=fill)[:, 0].cpu().numpy() > 0.5 for fill in FILLS}
    for i in range(len(grids)):
        print(f"{name}[{i}]: occupied {int(want[i].sum())} F {meshes[i].faces.shape[0]} interior differs {int((got['interior'][i] != want[i]).sum())} "
              f"surface {int(got['surface'][i].sum())} solid {int(got['solid'][i].sum())}")
        assert np.array_equal(got["interior"][i], want[i]), (name, i)
        assert bool((got["solid"][i] >= want[i]).all()) and np.array_equal(got["solid"][i], got["surface"][i] | got["interior"][i]), (name, i)
        assert bool(got["surface"][i].any()) == bool(want[i].any()), (name, i)


# ------------------------------------------------------------------ 3. conditioned random triangles
@pytest.fixture(scope="module")
def conditioned():
    meshes = [S.conditioned_triangles(300, seed) for seed in range(4)]
    return meshes, [S.voxelize_surface_vec(S.index_coords(v, 32), f, 32) for v, f in meshes]


def test_conditioned_random_triangles_match_outside_the_margin(conditioned):
    meshes, ref = conditioned
    got = voxelize(meshes, 32, "surface")
    for i, (want, margin) in enumerate(ref):
        keep = margin >= MARGIN
        left_out = 1.0 - float(keep.mean())
        wrong = int(((got[i] != want) & keep).sum())
        print(f"mesh {i}: statement {int(want.sum())} device {int(got[i].sum())} left out {left_out:.5f} wrong among the kept {wrong} among all {int((got[i] != want).sum())}")
        assert int(got[i].sum()) > 0 and int(want.sum()) > 0
        assert left_out <= 0.01
        assert wrong == 0


# ------------------------------------------------------------------ 4. sampling
def sampler_meshes():
    """The surface-nets meshes of the small 5^3 shapes and a unit cube: host float32 arrays, at most 256 faces each."""
    out = [(m.vertices.cpu().numpy(), m.faces.cpu().numpy()) for m in device_meshes(r5_grids())]
    v, f = S.cube(-0.5, 0.5)
    out.append((v.astype(np.float32), f))
    assert all(0 < f.shape[0] <= 256 for _, f in out)
    return out


def test_sampling_with_injected_uniforms_matches_the_statement():
    from shapegen_amd.utils import sample_mesh_points
    meshes = sampler_meshes()
    n = 4096
    u = torch.rand(len(meshes), n, 3, generator=torch.Generator().manual_seed(7))
    assert float(u.max()) < 1.0
    points, normals, index = sample_mesh_points([dev(m) for m in meshes], n, return_normals=True, return_faces=True, uniforms=u.cuda())
    assert tuple(points.shape) == (len(meshes), n, 3) and tuple(normals.shape) == (len(meshes), n, 3) and tuple(index.shape) == (len(meshes), n)
    assert points.dtype == torch.float32 and normals.dtype == torch.float32 and index.dtype == torch.int32
    points, normals, index, u = points.cpu().numpy().astype(np.float64), normals.cpu().numpy().astype(np.float64), index.cpu().numpy(), u.numpy()
    for i, (v, f) in enumerate(meshes):
        want_index, _ = S.sample_points(v, f, u[i])
        run = S.running_areas(v, f)
        target = u[i, :, 0].astype(np.float64) * run[-1]
        near = np.abs(target[:, None] - run[None, :]).min(axis=1) < 1e-5 * run[-1]
        assert index[i].min() >= 0 and index[i].max() < f.shape[0]
        wrong = int(((index[i] != want_index) & ~near).sum())
        want_points, want_normals = S.points_on(v, f, index[i], u[i])
        dp, dn = float(np.abs(points[i] - want_points).max()), float(np.abs(normals[i] - want_normals).max())
        unit = float(np.abs(np.linalg.norm(normals[i], axis=1) - 1.0).max())
        print(f"mesh {i}: F {f.shape[0]} left out {near.mean():.5f} wrong faces {wrong} (all {int((index[i] != want_index).sum())}) max |dp| {dp:.2e} |dn| {dn:.2e} "
              f"| |n| - 1 | {unit:.2e}")
        assert float(near.mean()) <= 0.02
        assert wrong == 0
        assert dp <= 1e-5 and dn <= 1e-5 and unit <= 1e-5


def _on_face_residual(v, f, index, points):
    """Distance of each point from its reported triangle's plane, and how far its barycentric coordinates leave [0, 1] (float64)."""
    t = np.asarray(v, np.float64)[np.asarray(f, np.int64)[index]]
    a, e0, e1 = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    d = points - a
    g00, g01, g11 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1)
    b0, b1 = (d * e0).sum(1), (d * e1).sum(1)
    det = g00 * g11 - g01 * g01
    s, w = (g11 * b0 - g01 * b1) / det, (g00 * b1 - g01 * b0) / det
    off = np.linalg.norm(d - s[:, None] * e0 - w[:, None] * e1, axis=1)
    outside = np.maximum.reduce([-s, -w, s + w - 1.0, np.zeros_like(s)])
    return float(off.max()), float(outside.max())


def test_sampling_with_philox_is_repeatable_independent_and_on_the_surface():
    from shapegen_amd.utils import sample_mesh_points
    meshes = sampler_meshes()
    device = [dev(m) for m in meshes]
    n = 2048
    p1, n1, i1 = sample_mesh_points(device, n, seed=11, return_normals=True, return_faces=True)
    p2, n2, i2 = sample_mesh_points(device, n, seed=11, return_normals=True, return_faces=True)
    assert torch.equal(p1, p2) and torch.equal(n1, n2) and torch.equal(i1, i2)
    p3 = sample_mesh_points(device, n, seed=12)
    assert torch.is_tensor(p3) and not torch.equal(p1, p3) and float((p1 != p3).float().mean()) > 0.9
    for k, m in enumerate(device):                                          # each mesh of the batch gets the bits it gets alone
        pa, na, ia = sample_mesh_points([m], n, seed=11, return_normals=True, return_faces=True)
        assert torch.equal(pa[0], p1[k]) and torch.equal(na[0], n1[k]) and torch.equal(ia[0], i1[k]), k
    for k, (v, f) in enumerate(meshes):
        off, outside = _on_face_residual(v, f, i1[k].cpu().numpy(), p1[k].cpu().numpy().astype(np.float64))
        print(f"mesh {k}: off the plane {off:.2e}, outside the triangle {outside:.2e}")
        assert off <= 1e-5 and outside <= 1e-5
    torch.manual_seed(3)                                                     # seed=None draws from the global generator
    a = sample_mesh_points(device, 64)
    b = sample_mesh_points(device, 64)
    torch.manual_seed(3)
    c = sample_mesh_points(device, 64)
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_sampling_is_uniform_by_area_on_the_cube():
    from shapegen_amd.utils import sample_mesh_points
    v, f = S.cube(-0.5, 0.5)
    n = 49152
    _, index = sample_mesh_points([dev((v, f))], n, seed=5, return_faces=True)
    counts = np.bincount(index[0].cpu().numpy(), minlength=12)
    print("per face:", counts.tolist())
    assert counts.shape == (12,) and int(counts.sum()) == n
    assert np.abs(counts - 4096).max() <= 5 * 61                            # binomial(49152, 1/12): sigma = 61


def test_a_mesh_of_zero_area_returns_its_first_vertex():
    from shapegen_amd.utils import sample_mesh_points
    v = np.asarray([(9.0, 9.0, 9.0), (1.0, 2.0, 3.0), (1.0, 2.0, 3.0), (1.0, 2.0, 3.0), (4.0, 4.0, 4.0)], np.float32)
    f = np.asarray([(1, 2, 3), (3, 3, 3)], np.int32)
    cube = S.cube(-0.5, 0.5)
    p, nrm, idx = sample_mesh_points([dev(cube), dev((v, f))], 100, seed=1, return_normals=True, return_faces=True)
    assert torch.equal(p[1].cpu(), torch.tensor([1.0, 2.0, 3.0]).expand(100, 3))
    assert not bool(nrm[1].any()) and not bool(idx[1].any())
    assert float(p[0].abs().max()) <= 0.5 + 1e-6 and bool(idx[0].any())          # a convex combination of coordinates +-0.5 in fp32: a few ulp at most


# ------------------------------------------------------------------ 5. repeatability, independence of the batch, the workspace
def raw_voxelize(meshes, r, fill, garbage):
    """The entry point itself, with a workspace of the caller's pre-filled with `garbage` bytes."""
    from shapegen_amd import _lib
    from shapegen_amd.utils import MESH_FILLS, _pack_meshes
    lib = _lib.load()
    verts, faces, offsets, rows = _pack_meshes([dev(m) for m in meshes], "test")
    b = len(meshes)
    size = lib.pcd_mesh_voxelize_workspace_bytes(b, r)
    assert size > 0
    ws = torch.full((size,), garbage, dtype=torch.uint8, device="cuda")
    vox = torch.full((b, 1, r, r, r), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.pcd_mesh_voxelize(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, r, -1.0, (r - 1) / 2.0, MESH_FILLS[fill],
                                     ws.data_ptr(), vox.data_ptr(), _lib.stream_ptr()), "mesh_voxelize")
    return vox


@pytest.mark.parametrize("r", [32, 40])
def test_repeatable_independent_of_the_batch_and_of_the_workspace(conditioned, r):
    from shapegen_amd.utils import meshes_to_voxel_tensor
    meshes = conditioned[0] + [(m.vertices.cpu().numpy(), m.faces.cpu().numpy()) for m in device_meshes(binary_grids("r5")[:3])]
    meshes.append((np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32)))                  # a mesh without faces: an empty grid
    device = [dev(m) for m in meshes]
    for fill in FILLS:
        first = meshes_to_voxel_tensor(device, r, fill=fill)
        assert torch.equal(first, meshes_to_voxel_tensor(device, r, fill=fill))
        order = [5, 2, 7, 0, 6, 3, 1, 4]
        assert torch.equal(meshes_to_voxel_tensor([device[k] for k in order], r, fill=fill), first[order])
        assert torch.equal(meshes_to_voxel_tensor([device[3]], r, fill=fill), first[3:4])
        assert torch.equal(raw_voxelize(meshes, r, fill, 0x5A), first) and torch.equal(raw_voxelize(meshes, r, fill, 0xFF), first)
        assert not bool(first[7].any()) and bool(first[0].any())


# ------------------------------------------------------------------ 6. refusals, the extreme resolutions
def test_bad_arguments_raise():
    from shapegen_amd.utils import Mesh, meshes_to_voxel_tensor, sample_mesh_points
    cube = S.cube(-0.5, 0.5)
    host = Mesh(torch.from_numpy(cube[0].astype(np.float32)), torch.from_numpy(cube[1]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshes_to_voxel_tensor([host])
    with pytest.raises(RuntimeError, match="no CPU path"):
        sample_mesh_points([host], 16)
    d = dev(cube)
    for kw in (dict(fill="shell"), dict(fill=None), dict(bounds=(1.0, 1.0)), dict(bounds=(1.0, -1.0)), dict(bounds=(0.0, float("inf"))),
               dict(resolution=1), dict(resolution=65), dict(resolution=0), dict(resolution=31.5)):
        with pytest.raises(ValueError):
            meshes_to_voxel_tensor([d], **kw)
    empty = Mesh(d.vertices, d.faces[:0])
    with pytest.raises(ValueError, match="mesh 1 "):
        sample_mesh_points([d, empty, d], 16)
    with pytest.raises(ValueError):
        sample_mesh_points([d], 0)
    assert tuple(meshes_to_voxel_tensor([(d.vertices, d.faces)], 4).shape) == (1, 1, 4, 4, 4)         # a plain (vertices, faces) pair


@pytest.mark.parametrize("r", [2, 64])
def test_the_extreme_resolutions_run_and_match_the_statement(r):
    v, f = S.merge(S.cube(-0.61, 0.43), S.cube((0.3, 0.2, 0.1), (1.2, 1.3, 1.4)))                    # the second box leaves the grid round its last node
    v = v.astype(np.float32)
    p = S.index_coords(v, r)
    (surface, ms), (interior, mi) = S.voxelize_surface_vec(p, f, r), S.voxelize_interior_vec(p, f, r)
    for fill, want, margin in (("surface", surface, ms), ("interior", interior, mi)):
        got = voxelize([(v, f)], r, fill)[0]
        keep = margin >= MARGIN
        print(f"R {r} {fill}: statement {int(want.sum())} device {int(got.sum())} left out {1.0 - keep.mean():.5f} wrong {int(((got != want) & keep).sum())}")
        assert int(want.sum()) > 0 and float(keep.mean()) >= 0.99 and not bool(((got != want) & keep).any())


# ------------------------------------------------------------------ 7. the entry script
def test_preprocess_meshes_script(tmp_path):
    from shapegen_amd.data import DeviceVoxelDataModule, PointCloudDataset
    from shapegen_amd.utils import Mesh, load_mesh, meshes_to_voxel_tensor, normalize_mesh, sample_mesh_points, save_mesh
    src, out, pts = tmp_path / "meshes", tmp_path / "grids", tmp_path / "clouds"
    os.makedirs(src)
    zz, yy, xx = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    blob = (((zz - 14) / 9.0) ** 2 + ((yy - 17) / 6.0) ** 2 + ((xx - 15) / 12.0) ** 2 <= 1).astype(np.float32)
    shapes = {"1a_x_y_z_02691156_0": S.cube((-2.0, -1.0, -0.5), (2.0, 1.0, 0.5)),           # extents x > y > z: the asymmetric one
              "1a_x_y_z_03001627_1": tuple(t.cpu().numpy() for t in device_meshes([blob])[0]),
              "1a_x_y_z_03001627_2": S.merge(S.cube(-0.5, 0.25), S.cube(0.0, 0.5))}
    for stem, (v, f) in shapes.items():
        save_mesh(str(src / (stem + ".obj")), (torch.from_numpy(np.asarray(v, np.float32)), torch.from_numpy(np.asarray(f, np.int32))))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "preprocess_meshes.py"), str(src), str(out), "--points-dir", str(pts), "--num-points", "256",
                        "--batch", "2", "--seed", "9"], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == sorted(os.listdir(pts)) == sorted(s + ".npz" for s in shapes)
    margin = 2.0 / 31.0
    normalised = {s: normalize_mesh(load_mesh(str(src / (s + ".obj"))), margin) for s in shapes}
    want = {s: meshes_to_voxel_tensor([Mesh(m.vertices.cuda(), m.faces.cuda())], 32)[0].cpu() for s, m in normalised.items()}
    # the host dataset reads the grids
    ds = PointCloudDataset(str(out), input_mode="voxels", output_mode="voxels", jitter=False, return_labels=True)
    assert len(ds) == 3 and ds.categories == ["airplane", "chair"]          # the file name, and with it the synset-id field, is kept
    for i, name in enumerate(ds.file_list):
        grid, _ = ds[i]
        raw = np.load(str(out / name))["data"]
        assert raw.dtype == np.uint8 and raw.shape == (32, 32, 32)
        assert tuple(grid.shape) == (1, 32, 32, 32) and torch.equal(grid, want[name[:-4]]) and int(grid.sum()) > 100, name
    # the device module reads them
    dm = DeviceVoxelDataModule(data_dir=str(out), output_mode="voxels", augmentations=False, batch_size=3)
    dm.setup()
    batch = dm.batch(torch.arange(3, dtype=torch.int32, device="cuda"), seed=0, offset=0)
    for i, name in enumerate(dm.file_list):
        assert torch.equal(batch[i].cpu(), want[name[:-4]]), name
    # the documented axes: in the clouds the datasets make from a grid, column 0 is the mesh's z, column 1 its y, column 2 its x
    box = PointCloudDataset.voxel_to_point_cloud(want["1a_x_y_z_02691156_0"][0].numpy())
    span = box.max(axis=0) - box.min(axis=0)
    v = normalised["1a_x_y_z_02691156_0"].vertices.numpy()
    assert np.allclose(v.max(axis=0), [1 - margin, (1 - margin) / 2, (1 - margin) / 4], atol=1e-6)
    assert span.tolist() == [7, 15, 29], span                               # the box spans 29, 14.5 and 7.25 pitches round the centre 15.5: nodes 1 .. 30 in x, 8 .. 23 in y, 12 .. 19 in z
    # the clouds load as point-cloud files, are the sampler's output for the mesh alone, and keep the mesh's own [x, y, z] columns
    dp = PointCloudDataset(str(pts), num_points=256, input_mode="point_clouds", output_mode="point_clouds", normalize=False, jitter=False)
    assert len(dp) == 3
    for i, name in enumerate(dp.file_list):
        cloud = dp[i]
        m = normalised[name[:-4]]
        alone = sample_mesh_points([Mesh(m.vertices.cuda(), m.faces.cuda())], 256, seed=9)[0].cpu()
        assert tuple(cloud.shape) == (256, 3) and cloud.dtype == torch.float32 and torch.equal(cloud, alone), name
    cloud = torch.from_numpy(np.load(str(pts / "1a_x_y_z_02691156_0.npz"))["data"])
    ext = cloud.abs().max(dim=0).values
    assert 0.8 < float(ext[0]) <= 1 - margin + 1e-6 and 0.4 < float(ext[1]) <= (1 - margin) / 2 + 1e-6 and float(ext[2]) <= (1 - margin) / 4 + 1e-6
