"""The meshes the simplification tests add to tests/mesh_ops_cases.py (reused unchanged through `case`): the smallest shapes at which the
kernels of csrc/mesh_simplify.hip can go wrong.  `case(name)` serves both sets."""
import functools

import numpy as np

import mesh_ops_cases as C


def doubled_cube():
    """The cube with its first two faces listed twice (at the end): 14 faces, 12 after `deduplicate`."""
    v, f = C.cube()
    return C._mesh(v, np.concatenate([f, f[:2]]))


def thin_plate(n=9, gap=0.01):
    """Two n x n sheets `gap` apart with side walls, closed, outward: the sheets fall into the same cells below R of about 1 / gap."""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    flat = np.stack([i / (n - 1.0), j / (n - 1.0), np.zeros_like(i, float)], axis=-1).reshape(-1, 3)
    top = flat + [0.0, 0.0, gap]
    f = []
    for r in range(n - 1):
        for c in range(n - 1):
            q = r * n + c
            f += [[q, q + n + 1, q + 1], [q, q + n, q + n + 1]]                                  # bottom, facing -z
            f += [[n * n + q, n * n + q + 1, n * n + q + n + 1], [n * n + q, n * n + q + n + 1, n * n + q + n]]   # top, facing +z
    ring = [c for c in range(n)] + [r * n + n - 1 for r in range(1, n)] + [(n - 1) * n + c for c in range(n - 2, -1, -1)] + \
           [r * n for r in range(n - 2, 0, -1)]                                                  # the boundary, counter-clockwise from above
    for a, b in zip(ring, ring[1:] + ring[:1]):
        f += [[a, b, n * n + b], [a, n * n + b, n * n + a]]
    return C._mesh(np.concatenate([flat, top]), f)


def flat_patch(n=5):
    """An open n x n patch in the plane z = 0: every quadric is singular, the regulariser decides."""
    v, f = C.grid_patch(n)
    v = v.copy()
    v[:, 2] = 0.0
    return v, f


def coincident():
    """Every referenced vertex at one point (the faces have no area): ext = 0, one cluster.  Vertex 0 is unreferenced and elsewhere."""
    v = [[5.0, 5.0, 5.0]] + [[0.25, -1.5, 3.0]] * 4
    return C._mesh(v, [[1, 2, 3], [1, 3, 4], [2, 4, 3]])


def non_finite():
    """The cube with a NaN and an infinity in referenced vertices."""
    v, f = C.cube()
    v = v.copy()
    v[3, 1] = np.nan
    v[6, 0] = np.inf
    return v, f


def non_finite_unreferenced():
    """The cube and three unreferenced vertices that are not finite: they must not touch the box."""
    v, f = C.cube()
    extra = np.array([[np.nan, 0, 0], [np.inf, -np.inf, 0], [0, 0, -np.inf]], np.float32)
    return C._mesh(np.concatenate([extra[:1], v, extra[1:]]), f + 1)


BUILDERS = dict(doubled_cube=doubled_cube, thin_plate=thin_plate, flat_patch=flat_patch, coincident=coincident, non_finite=non_finite,
                non_finite_unreferenced=non_finite_unreferenced)
NEW = tuple(BUILDERS)
CLOSED = C.CLOSED_GENUS_0 + ("thin_plate",)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in C.BUILDERS:
        return C.case(name)
    v, f = BUILDERS[name]()
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f
