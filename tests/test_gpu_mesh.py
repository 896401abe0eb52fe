"""Mesh output on the GPU (csrc/mesh.hip through `utils.voxel_tensor_to_meshes`): index arrays equal to the float64 statement
(tests/mesh_statement.py) and vertices within the fp32 bound on lattice inputs, in both forms of the kernels (grid staged in LDS, grid read
through the cache); the invariants of the device meshes; repeatability and independence of the batch; the overlay with the point conversion;
`output="mesh"` of the latent samplers; the entry script.

Inputs are lattice fields (multiples of 1/64, threshold 51/128): fp32 and float64 put every node on the same side and the crossing parameter is
one correctly rounded division, so nothing is masked or left out.  Vertex bound 2e-5 absolute in output coordinates: t is exact to 1 ulp and
about 16 fp32 roundings at index magnitude <= 34 give <= 3e-5 index units, times the pitch 2 / 31 = 2e-6; the bound is ten times that, and a dropped
or misplaced crossing moves a vertex by 1e-3 or more.  The awkward extents keep the bound: their pitch is up to 2 (extent 2), but their indices
stay below 10, where 16 roundings are under 8e-6 index units.

The statement runs once per grid for the whole module (about 2 s of host loops for the seven 32^3 grids) and is left unchanged."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_statement as S
from helpers import latent_sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

N = 32
VERTEX_TOL = 2e-5
NAMES = ("empty", "full", "corner_0", "corner_31", "sphere", "random", "checkerboard")


def _grids():
    shape = (N, N, N)
    return [S.lattice(np.zeros(shape)), S.lattice(np.ones(shape)), S.single_voxel(shape, (0, 0, 0)), S.single_voxel(shape, (N - 1,) * 3),
            S.lattice_sphere(N, (15.3, 15.6, 15.9), 11.2), S.lattice_random(shape, 0), S.checkerboard(shape)]


def _awkward():
    a = (3, 5, 9)
    sphere = np.round(np.clip(0.5 + (1.6 - np.sqrt(sum((g - c) ** 2 for g, c in zip(np.meshgrid(*map(np.arange, a), indexing="ij"),
                                                                                     (1.2, 2.3, 4.4))))) / 2.0, 0, 1) * 64.0) / 64.0
    b = (2, 2, 2)
    return {a: [S.lattice_random(a, 1), S.checkerboard(a), S.lattice(sphere), S.lattice(np.ones(a))],
            b: [S.lattice_random(b, 2), S.lattice(np.ones(b)), S.single_voxel(b, (1, 0, 1)), S.lattice(np.zeros(b)), S.checkerboard(b)]}


_cache = {}


def reference(key, grids):
    """Statement meshes and their invariants of a list of grids, computed once and left unchanged."""
    if key not in _cache:
        out = []
        for g in grids:
            v, f = S.surface_nets(g, S.THR)
            out.append((v, f, S.mesh_invariants(v, f)))
        _cache[key] = out
    return _cache[key]


def batch_of(grids):
    return torch.from_numpy(np.stack(grids)[:, None]).cuda()


def meshes_of(grids, staged=1):
    from shapegen_amd import _lib
    from shapegen_amd.utils import voxel_tensor_to_meshes
    lib = _lib.load()
    assert lib.pcd_mesh_config(staged) == 0
    try:
        return voxel_tensor_to_meshes(batch_of(grids), threshold=S.THR)
    finally:
        assert lib.pcd_mesh_config(1) == 0


@pytest.fixture(scope="module")
def seven():
    grids = _grids()
    return grids, reference("seven", grids), meshes_of(grids)


def _compare(meshes, ref, tol, what):
    assert len(meshes) == len(ref)
    for i, (m, (v, f, _)) in enumerate(zip(meshes, ref)):
        assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32 and m.vertices.is_cuda and m.faces.is_cuda
        assert tuple(m.vertices.shape) == v.shape and tuple(m.faces.shape) == f.shape, (what, i, m.vertices.shape, v.shape, m.faces.shape, f.shape)
        assert torch.equal(m.faces.cpu(), torch.from_numpy(f)), (what, i)
        err = float(np.abs(m.vertices.cpu().numpy().astype(np.float64) - v).max()) if v.size else 0.0
        print(f"{what}[{i}]: V {v.shape[0]} F {f.shape[0]} max |dv| {err:.3e} (bound {tol:.1e})")
        assert err <= tol, (what, i, err)


# ------------------------------------------------------------------ 1. parity with the statement
@pytest.mark.parametrize("staged", [1, 0], ids=["lds", "global"])
def test_seven_grids_match_the_statement(seven, staged):
    grids, ref, staged_meshes = seven
    meshes = staged_meshes if staged else meshes_of(grids, staged=0)
    _compare(meshes, ref, VERTEX_TOL, "seven")
    assert ref[0][0].shape == (0, 3) and ref[0][1].shape == (0, 3)                    # the empty grid: (0, 3) and (0, 3)
    nv, nq = S.capacities((N, N, N))
    assert ref[6][2]["V"] == nv - 4 and ref[6][2]["F"] == 2 * (nq - 3 * N * N)         # checkerboard: all but four corner cells; half the border edges
    if not staged:                                                                     # the two forms give the same bits
        for a, b in zip(meshes, staged_meshes):
            assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)


@pytest.mark.parametrize("staged", [1, 0], ids=["lds", "global"])
@pytest.mark.parametrize("shape", [(3, 5, 9), (2, 2, 2)], ids=["3x5x9", "2x2x2"])
def test_awkward_extents_match_the_statement(shape, staged):
    """Extents that are no multiple of a wave and fewer cells than one pass of the workgroup (240 and 27 of 1024)."""
    grids = _awkward()[shape]
    _compare(meshes_of(grids, staged), reference(shape, grids), VERTEX_TOL, str(shape))


# ------------------------------------------------------------------ 2. invariants of the device output
def test_device_meshes_are_closed_with_the_statement_volume(seven):
    _, ref, meshes = seven
    for name, m, (_, _, want) in zip(NAMES, meshes, ref):
        got = S.mesh_invariants(m.vertices.cpu().numpy(), m.faces.cpu().numpy())
        print(name, got)
        assert got["closed"] and want["closed"]
        assert {k: got[k] for k in ("V", "F", "E", "chi", "max_edge_use")} == {k: want[k] for k in ("V", "F", "E", "chi", "max_edge_use")}
        if name == "empty":                                        # no surface: nothing to have a volume
            assert got["V"] == got["F"] == 0
            continue
        assert got["volume"] > 0 and abs(got["volume"] - want["volume"]) <= 1e-4 * want["volume"], (name, got["volume"], want["volume"])
    assert ref[4][2]["chi"] == 2 and ref[4][2]["max_edge_use"] == 2 and ref[1][2]["chi"] == 2          # sphere and full box: manifold spheres


# ------------------------------------------------------------------ 3. repeatability, batch independence
def test_repeatable_and_independent_of_the_batch(seven):
    grids, _, meshes = seven
    again = meshes_of(grids)
    for a, b in zip(meshes, again):
        assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)
    for i, g in enumerate(grids):
        alone = meshes_of([g])[0]
        assert torch.equal(alone.vertices, meshes[i].vertices) and torch.equal(alone.faces, meshes[i].faces), NAMES[i]


# ------------------------------------------------------------------ 4. overlay with the point conversion
def test_point_cloud_lies_inside_the_mesh_bounding_box(seven):
    from shapegen_amd.utils import voxel_tensor_to_point_clouds
    grids, _, meshes = seven
    g = grids[4]                                                   # the sphere: off-centre on every axis by a different amount
    pts = voxel_tensor_to_point_clouds(batch_of([g]), threshold=S.THR)[0]
    assert pts.shape[0] == int((g > S.THR).sum()) > 1000
    lo, hi = meshes[4].vertices.min(dim=0).values, meshes[4].vertices.max(dim=0).values
    assert bool((pts >= lo).all()) and bool((pts <= hi).all())
    pitch = 2.0 / (N - 1)                                          # and the box hugs the cloud: less than a pitch away on every side
    assert bool((pts.min(dim=0).values - lo < pitch).all()) and bool((hi - pts.max(dim=0).values < pitch).all())


def test_bad_arguments_raise():
    from shapegen_amd.utils import voxel_tensor_to_meshes
    x = batch_of([S.checkerboard((4, 4, 4))])
    for thr in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="mesh_count"):
            voxel_tensor_to_meshes(x, threshold=thr)
    with pytest.raises(RuntimeError):
        voxel_tensor_to_meshes(x[:, :, :1], threshold=0.5)


# ------------------------------------------------------------------ 5. through the model
@pytest.fixture(scope="module")
def ldm():
    from shapegen_amd.diffusion import LatentDiffusion
    from shapegen_amd.vae import VAE3DLarge
    m = LatentDiffusion(VAE3DLarge())
    m.load_state_dict(latent_sd(), strict=True)
    return m.to("cuda").eval()


def _same(meshes, want):
    assert len(meshes) == len(want) == 4
    for a, b in zip(meshes, want):
        assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)


def test_samplers_return_the_meshes_of_their_decoded_grids(ldm):
    from shapegen_amd.utils import Mesh, voxel_tensor_to_meshes
    z_T = torch.randn(4, 256, generator=torch.Generator().manual_seed(5)).cuda()
    thr = 0.4
    meshes, z_0 = ldm.sample(4, num_steps=2, threshold=thr, z_T=z_T, output="mesh", return_latent=True)
    assert all(isinstance(m, Mesh) for m in meshes) and tuple(z_0.shape) == (4, 256)
    grids = ldm.vae.decode(z_0)
    _same(meshes, voxel_tensor_to_meshes(grids, threshold=thr))
    print("sample: (V, F) per shape", [(m.vertices.shape[0], m.faces.shape[0]) for m in meshes], "occupied", (grids > thr).sum(dim=(1, 2, 3, 4)).tolist())
    only = ldm.sample(4, num_steps=2, threshold=thr, z_T=z_T, output="mesh")
    _same(only, meshes)
    points = ldm.sample(4, num_steps=2, threshold=thr, z_T=z_T)                       # the default is still the point list
    assert all(torch.is_tensor(p) and p.shape[1] == 3 for p in points)
    meshes, z_0 = ldm.sample_dpm(4, num_steps=2, threshold=thr, z_T=z_T, output="mesh", return_latent=True)
    _same(meshes, voxel_tensor_to_meshes(ldm.vae.decode(z_0), threshold=thr))
    for call in (lambda: ldm.sample(4, num_steps=2, z_T=z_T, output="voxels"), lambda: ldm.sample_dpm(4, num_steps=2, z_T=z_T, output="Mesh"),
                 lambda: ldm.sample2(4, num_steps=2, z_T=z_T, output=None), lambda: ldm.sample3(4, num_steps=2, output="")):
        with pytest.raises(ValueError, match="output must be"):
            call()


# ------------------------------------------------------------------ 6. the entry script
def test_generate_mesh_ldm_script(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_mesh_ldm.py"), "--num-samples", "2", "--steps", "2", "--format", "obj",
                        "--out", str(tmp_path / "o")], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    log = open(tmp_path / "test" / "logs" / "mesh_ldm_generate.log").read()
    lines = re.findall(r"mesh (\d+): (\d+) vertices, (\d+) triangles, closed (True|False) -> (\S+)", log)
    assert [int(l[0]) for l in lines] == [0, 1]
    for i, nv, nf, closed, path in lines:
        assert os.path.samefile(path if os.path.isabs(path) else tmp_path / path, tmp_path / "o" / f"mesh_{i}.obj") and closed == "True"
        rows = [l.split() for l in open(tmp_path / "o" / f"mesh_{i}.obj") if l[:2] in ("v ", "f ")]
        v = [r for r in rows if r[0] == "v"]
        f = np.asarray([[int(t) for t in r[1:]] for r in rows if r[0] == "f"], np.int64).reshape(-1, 3)
        assert len(v) == int(nv) and f.shape[0] == int(nf)
        assert all(np.isfinite(float(t)) for r in v for t in r[1:])
        assert f.size == 0 or (f.min() >= 1 and f.max() <= len(v))
