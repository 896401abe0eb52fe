"""The meshes the mesh-processing tests run on: the smallest shapes at which each kernel of csrc/mesh_ops.hip can go wrong.  Every case is
(vertices (V, 3) float32, faces (F, 3) int32) in numpy; `CASES` builds each once."""
import functools

import numpy as np

import mesh_statement as MS


def _mesh(v, f):
    return np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)


def tetrahedron(shift=(0.0, 0.0, 0.0), scale=1.0):
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * scale + np.asarray(shift)
    return _mesh(v, [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])              # outward


def octahedron():
    v = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    return _mesh(v, [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def cube(shift=(0.0, 0.0, 0.0)):
    """Half-extent 1, 12 outward triangles: volume 8, area 24."""
    v = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64) + np.asarray(shift)
    f = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]
    return _mesh(v, f)


def grid_patch(n=5):
    """An open n x n patch of vertices with a gentle bump: it has a boundary."""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i / (n - 1.0), j / (n - 1.0), 0.1 * np.sin(1.7 * i + 0.3) * np.cos(1.1 * j)], axis=-1).reshape(-1, 3)
    f = []
    for r in range(n - 1):
        for c in range(n - 1):
            q = r * n + c
            f += [[q, q + 1, q + n + 1], [q, q + n + 1, q + n]]
    return _mesh(v, f)


def cube_flipped():
    """The cube with the winding of one triangle reversed: not closed, irregular edges, no boundary."""
    v, f = cube()
    f = f.copy()
    f[3] = f[3][[0, 2, 1]]
    return v, f


def non_manifold():
    """Three triangles on one edge (0, 1)."""
    v = [[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -0.5, 0.8], [0.5, -0.5, -0.8]]
    return _mesh(v, [[0, 1, 2], [1, 0, 3], [0, 1, 4]])


def pole_fan(n=70):
    """A closed fan of n triangles round vertex 0, whose row is longer than a wave."""
    t = 2.0 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(t), np.sin(t), 0.05 * np.cos(3.0 * t)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.4]], rim])
    f = [[0, 1 + i, 1 + (i + 1) % n] for i in range(n)]
    return _mesh(v, f)


def two_tetrahedra():
    """Two disjoint tetrahedra with equal face counts: the tie of the `largest` rule."""
    (va, fa), (vb, fb) = tetrahedron((3.0, 0.0, 0.0), 0.5), tetrahedron((-3.0, 0.5, 0.0), 0.7)
    return _mesh(np.concatenate([va, vb]), np.concatenate([fa, fb + 4]))


def mixed():
    """An unreferenced vertex (row 0), a cube (rows 1..8) and two disjoint tetrahedra with equal face counts (rows 9..12, 13..16)."""
    (vc, fc), (vt, ft) = cube(), two_tetrahedra()
    return _mesh(np.concatenate([[[9.0, 9.0, 9.0]], vc, vt]), np.concatenate([fc + 1, ft + 9]))


def bad_indices():
    """The open patch with faces that are not valid: an index past the vertices, a negative one, a repeated one."""
    v, f = grid_patch(4)
    extra = [[0, 1, 16], [-1, 2, 3], [5, 5, 6], [7, 8, 7], [2, 2, 2]]
    return _mesh(v, np.concatenate([f[:5], extra, f[5:]]))


def empty():
    return _mesh(np.zeros((0, 3)), np.zeros((0, 3)))


def icosphere(level, jitter_seed=None):
    """10 * 4**level + 2 vertices on the unit sphere, optionally with a seeded radial jitter of up to 5 %."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1], [-p, 0, -1],
         [-p, 0, 1]]
    v = [np.asarray(q, np.float64) / np.linalg.norm(q) for q in v]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4],
         [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(level):
        mid, g = {}, []

        def middle(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                q = v[a] + v[b]
                v.append(q / np.linalg.norm(q))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            g += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = g
    v = np.asarray(v)
    if jitter_seed is not None:
        v = v * (1.0 + 0.05 * np.random.default_rng(jitter_seed).uniform(-1.0, 1.0, (v.shape[0], 1)))
    return _mesh(v, f)


def surface_nets_sphere():
    v, f = MS.surface_nets(MS.lattice_sphere(), MS.THR)
    return _mesh(v, f)


BUILDERS = dict(tetrahedron=tetrahedron, octahedron=octahedron, cube=cube, grid_patch=grid_patch, cube_flipped=cube_flipped,
                non_manifold=non_manifold, pole_fan=pole_fan, two_tetrahedra=two_tetrahedra, mixed=mixed, bad_indices=bad_indices, empty=empty,
                icosphere_642=functools.partial(icosphere, 3, 7), icosphere_10242=functools.partial(icosphere, 5), nets_sphere=surface_nets_sphere)
SMALL = tuple(k for k in BUILDERS if k != "icosphere_10242")
CLOSED_GENUS_0 = ("tetrahedron", "octahedron", "cube", "icosphere_642", "icosphere_10242", "nets_sphere")
# the empty mesh first, in the middle and last, sizes mixed from 5 to 10 242 vertices
MIXED_BATCH = ("empty", "cube", "icosphere_10242", "pole_fan", "empty", "mixed", "icosphere_642", "bad_indices", "nets_sphere", "empty")


@functools.lru_cache(maxsize=None)
def case(name):
    v, f = BUILDERS[name]()
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f
