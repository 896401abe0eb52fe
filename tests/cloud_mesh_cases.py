"""Inputs shared by the cloud-to-mesh tests (tests/test_cloud_mesh_statement_cpu.py, tests/test_gpu_cloud_mesh.py): shell masks for the fill,
outside masks for the depth, clouds for the shell, and the surfaces of the end-to-end and condition tests, with the statements of
tests/cloud_mesh_statement.py computed once per case and shared.

Launch shapes as built (csrc/cloud_mesh.hip).  Shell + fill: one workgroup of 1024 threads per cloud, a thread owns the rows (z, y) = tid,
tid + 1024, ... of R^2 <= 4096; a row is one 64-bit word, so R = 31 / 32 / 33 sit on both sides of the word's 32-bit half and 63 / 64 at the full
word (the mask of the bits at and past R; shifts by R - 1 and R).  The shell takes one point per wave, 16 waves: clouds of 0, 1, 255, 256, 257 and
1300 points end below, at and past a round of the waves.  Depth: grid (R, P) with 256 threads, lane = x, 4 rows at a time."""
import functools

import numpy as np
import torch

import cloud_mesh_statement as S
import geometry_cases as GC

FILL_RESOLUTIONS = (8, 31, 32, 33, 63, 64)
MAZE_R = 33
MAZE_PATH = 512         # free nodes of the serpentine maze = the length of its only free path


def box(R, lo, hi, hollow=True):
    """The nodes of the cube [lo, hi]^3, its interior free if hollow (walls one node thick)."""
    m = np.zeros((R, R, R), bool)
    m[lo:hi + 1, lo:hi + 1, lo:hi + 1] = True
    if hollow:
        m[lo + 1:hi, lo + 1:hi, lo + 1:hi] = False
    return m


def corridor(R):
    """All shell but one corridor: in from the grid's face at x = 0 along the row (z, y) = (R / 2, R / 2) to x = R - 2, over to the row y + 1
    there, and back along it to x = 1: the fill has to run the length of a word towards the high end and then towards the low end."""
    m = np.ones((R, R, R), bool)
    z = y = R // 2
    m[z, y, 0:R - 1] = False
    m[z, y + 1, 1:R - 1] = False
    return m


def maze(R=MAZE_R):
    """A serpentine wall maze in the y-z plane at x = R / 2, everything else shell: the lines z = 1, 3, .., R - 2 run over y = 1 .. R - 2, joined
    at alternating ends through z = 2, 4, .., and the line z = 1 opens to the face z = 0 at y = 1.  Every step of the path is a step to another
    word, so a sweep of the fill gains about one node: 16 * 31 + 15 + 1 = 512 nodes for R = 33."""
    m = np.ones((R, R, R), bool)
    x = R // 2
    m[0, 1, x] = False
    for n, z in enumerate(range(1, R - 1, 2)):
        m[z, 1:R - 1, x] = False
        if z + 2 < R - 1:
            m[z + 1, R - 2 if n % 2 == 0 else 1, x] = False
    return m


@functools.lru_cache(maxsize=None)
def fill_masks(R):
    """name -> shell mask bool [R][R][R]"""
    rng = np.random.default_rng(4100 + R)
    holed = box(R, 2, R - 3)
    holed[2, R // 2, R // 2] = False
    out = {"empty": np.zeros((R, R, R), bool), "full": np.ones((R, R, R), bool), "hollow": box(R, 2, R - 3), "holed": holed,
           "border": box(R, 0, R // 2), "random_0.3": rng.random((R, R, R)) < 0.3, "random_0.6": rng.random((R, R, R)) < 0.6,
           "corridor": corridor(R)}
    if R == MAZE_R:
        out["maze"] = maze(R)
    return out


@functools.lru_cache(maxsize=None)
def fill_statements(R):
    """name -> (outside bool [R][R][R], info)"""
    out = {}
    for name, m in fill_masks(R).items():
        o = S.outside_bfs(m)
        out[name] = (o, S.counts(m, o))
    return out


@functools.lru_cache(maxsize=None)
def depth_masks(R):
    """name -> outside mask: a single outside node in a full grid (the largest distances), none at all (only the layer round the grid), and the
    outsides of the hollow box and the sparser random mask."""
    single = np.zeros((R, R, R), bool)
    single[0, 0, 0] = True
    fills = fill_statements(R)
    return {"single": single, "none": np.zeros((R, R, R), bool), "hollow": fills["hollow"][0], "random_0.3": fills["random_0.3"][0]}


@functools.lru_cache(maxsize=None)
def depth_statements(R):
    return {name: S.depth2(m) for name, m in depth_masks(R).items()}


# ------------------------------------------------------------------ clouds for the shell
SHELL_RESOLUTIONS = (8, 33, 64)
SHELL_SIZES = (0, 1, 255, 256, 257, 1300)


@functools.lru_cache(maxsize=None)
def shell_clouds():
    """[(points (n, 3), count, radius)]: the sizes at the edges of a round of waves with two radii, a cloud cut by its count, one with a NaN and
    an infinite row, one that reaches far outside the bounds."""
    out = [(GC.uniform(n, 5000 + n), n, 0.2 if i % 2 else 0.31) for i, n in enumerate(SHELL_SIZES)]
    out.append((GC.uniform(300, 5301), 120, 0.2))
    out.append((GC.non_finite(200, 5302), 200, 0.31))
    out.append((GC.uniform(400, 5303) * 3.0, 400, 0.2))
    return out


def lattice_cloud():
    """Points on nodes of the R = 33 grid over (-1, 1), pitch 1/16, and r = 3/16: every d2 is a multiple of 1/256 and exact, r * r = 9/256 is
    reached exactly at the offsets (3, 0, 0) and (2, 2, 1), so the comparison's <= decides nodes."""
    g = torch.Generator().manual_seed(5400)
    return torch.randint(-12, 13, (60, 3), generator=g).float() / 16, 33, (-1.0, 1.0), 3.0 / 16.0


# ------------------------------------------------------------------ surfaces
def two_spheres():
    a, _ = GC.sphere(1024, 9201, 0.45)
    b, _ = GC.sphere(1024, 9202, 0.35)
    return torch.cat([a + torch.tensor([-0.5, 0.0, 0.0]), b + torch.tensor([0.55, 0.0, 0.0])])


def ellipsoid(n, seed, axes):
    """Area-weighted samples of the ellipsoid with the semi-axes `axes` about the origin (rejection from the sphere's directions)."""
    g = np.random.default_rng(seed)
    a = np.asarray(axes, np.float64)
    x = g.normal(size=(8 * n, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    w = np.sqrt(((x * np.array([a[1] * a[2], a[0] * a[2], a[0] * a[1]])) ** 2).sum(axis=1))
    keep = g.random(8 * n) < w / w.max()
    assert keep.sum() >= n
    return torch.from_numpy((x[keep][:n] * a).astype(np.float32))


@functools.lru_cache(maxsize=None)
def surface(name):
    if name == "sphere":
        return GC.sphere(2048, 9100)[0]
    if name == "torus":
        return GC.torus(2048, 9101)[0]
    if name == "two_spheres":
        return two_spheres()
    if name == "flat":
        return ellipsoid(2048, 9103, (0.8, 0.5, 0.01))
    raise KeyError(name)


# end to end against the statement at R = 32 with explicit radii
# (the clamp at R = 32 is 2 h = 0.161: the radii lie above it, and 2 r = 0.34 bridges the 0.25 between the two spheres -- one body, as the
# limits say; the statement says the same)
E2E = (("sphere", 0.2), ("torus", 0.17), ("two_spheres", 0.17))


@functools.lru_cache(maxsize=None)
def e2e_statement(name, radius_):
    return S.cloud_to_mesh(surface(name).numpy(), 32, radius_, do_project=False)


# the conditions: (surface, R, inset) with the spacing radius at scale 1.5, k = 8, bounds +-1.25.  The two spheres stand 0.25 apart: at R = 32
# the clamp 2 h = 0.161 makes 2 r wider than that and bridges them, so their case runs at R = 64 (r = 0.105).
CONDITIONS = (("sphere", 32, 0.0), ("sphere", 64, 0.0), ("torus", 32, 0.0), ("two_spheres", 64, 0.0), ("flat", 64, 0.5), ("flat", 64, -1.0))
CHI = {"sphere": 2, "torus": 0, "two_spheres": 4, "flat": 2}
SPHERE_BAND = 0.02          # every projected vertex of the sphere lies within this of radius 0.8
FLIP_SHARE = 0.01           # the projection turns at most this share of the sphere's triangles over


def check_conditions(name, R, inset, vertices, projected, faces, info):
    """The conditions of one case on a mesh, whoever made it; `info` = (shell, enclosed, border).  Returns the figures it looked at."""
    import mesh_statement as M
    inv = M.mesh_invariants(vertices, faces)
    out = dict(V=inv["V"], F=inv["F"], chi=inv["chi"], closed=inv["closed"], max_edge_use=inv["max_edge_use"], info=tuple(info))
    if name == "flat" and inset == 0.5:
        assert inv["V"] == 0 and inv["F"] == 0, out
        return out
    assert inv["closed"] and inv["chi"] == CHI[name] and inv["V"] > 0, out
    assert M.mesh_invariants(projected, faces)["closed"]
    if name == "sphere":
        assert inv["max_edge_use"] <= 4 and info[1] > 0 and info[2] == 0, out
        rad = np.linalg.norm(np.asarray(projected, np.float64), axis=1)
        out["radial"] = float(np.abs(rad - GC.SPHERE_RADIUS).max())
        out["flipped"] = S.flipped_share(vertices, projected, faces)
        assert out["radial"] <= SPHERE_BAND and out["flipped"] <= FLIP_SHARE, out
    return out
