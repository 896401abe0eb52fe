"""The literal float64 statement of the surface-nets definition (DESIGN.md "Mesh output"; include/pcd_hip.h pcd_mesh_*), with plain loops, for
small grids only; the invariants of a triangle mesh; and the lattice inputs on which fp32 and float64 classify every node alike.

Definition.  v[D][H][W], a node is inside iff v > thr (0 < thr).  The field is surrounded by one layer of nodes of value 0: padded node index
p = i + 1, padded extents D + 2, H + 2, W + 2.  Cell (cz, cy, cx), 0 <= cz <= D and likewise, has the padded nodes (cz + a, cy + b, cx + c),
a, b, c in {0, 1}; it is active iff its corners are not all on one side, and then owns one vertex: the arithmetic mean of the crossing points
A + t (B - A), t = (thr - v_A) / (v_B - v_A), of those of its 12 edges whose ends differ in side, in index coordinates of the unpadded grid
(padded - 1).  Vertices are numbered in row-major (cz, cy, cx) order of the active cells.  Faces: scan the padded nodes in row-major order and at
each the axes z, y, x; where the edge to the +1 neighbour along the axis exists and its ends differ in side, emit the quad of the four cells that
share it -- with (u, w) the two axes that follow the edge's axis cyclically, the node's own index offset by (du, dw) = (-1, -1), (0, -1), (0, 0),
(-1, 0), reversed when the node itself is inside -- as the triangles (q0, q1, q2), (q0, q2, q3).  Vertices leave as rows [x, y, z], the reverse of
the index order (z, y, x) in which the rule is written: with the reversal on the inside node the signed volume sum v0 . (v1 x v2) / 6 of the rows
that leave is positive (normals point outward); in (fz, fy, fx) index rows, a mirror image, it is the negative of that."""
import itertools

import numpy as np

THR = 51.0 / 128.0          # between the lattice values 25/64 and 26/64, 1/128 from each


CORNERS = list(itertools.product((0, 1), repeat=3))                                  # corner k = (a, b, c), k = 4 a + 2 b + c
EDGES = [(axis, CORNERS.index(A), CORNERS.index(tuple(A[k] + (k == axis) for k in range(3))))
         for axis in range(3) for A in CORNERS if A[axis] == 0]                      # the 12 edges of a cell: (axis, low corner, high corner)


def surface_nets_index(v, thr):
    """-> (vertices (V, 3) float64 as (fz, fy, fx) in index coordinates of the unpadded grid, faces (F, 3) int32)."""
    v = np.asarray(v, dtype=np.float64)
    assert v.ndim == 3 and thr > 0
    D, H, W = v.shape
    padded = np.zeros((D + 2, H + 2, W + 2), np.float64)
    padded[1:-1, 1:-1, 1:-1] = v
    p = padded.tolist()                                                               # nested lists of python floats (float64): plain indexing below
    inside = (padded > thr).tolist()
    number = [[[-1] * (W + 1) for _ in range(H + 1)] for _ in range(D + 1)]
    verts = []
    for cz in range(D + 1):
        for cy in range(H + 1):
            for cx in range(W + 1):
                side = [inside[cz + a][cy + b][cx + c] for a, b, c in CORNERS]
                if all(side) or not any(side):
                    continue
                total, n = [0.0, 0.0, 0.0], 0
                for axis, ka, kb in EDGES:
                    if side[ka] == side[kb]:
                        continue
                    A, B = CORNERS[ka], CORNERS[kb]
                    va, vb = p[cz + A[0]][cy + A[1]][cx + A[2]], p[cz + B[0]][cy + B[1]][cx + B[2]]
                    t = (thr - va) / (vb - va)
                    cell = (cz, cy, cx)
                    for k in range(3):
                        total[k] += cell[k] + A[k] + t * (B[k] - A[k]) - 1.0           # A + t (B - A), padded - 1
                    n += 1
                number[cz][cy][cx] = len(verts)
                verts.append([total[0] / n, total[1] / n, total[2] / n])
    faces = []
    ext = (D + 2, H + 2, W + 2)
    for z in range(D + 2):
        for y in range(H + 2):
            for x in range(W + 2):
                node = (z, y, x)
                for axis in range(3):
                    if node[axis] + 1 >= ext[axis]:
                        continue
                    nb = [z, y, x]
                    nb[axis] += 1
                    if inside[z][y][x] == inside[nb[0]][nb[1]][nb[2]]:
                        continue
                    u, w = (axis + 1) % 3, (axis + 2) % 3
                    quad = []
                    for du, dw in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
                        cell = [z, y, x]
                        cell[u] += du
                        cell[w] += dw
                        assert all(0 <= cell[k] <= ext[k] - 2 for k in range(3)), "a cell round a crossing edge always exists"
                        n = number[cell[0]][cell[1]][cell[2]]
                        assert n >= 0, "a cell round a crossing edge is always active"
                        quad.append(n)
                    if inside[z][y][x]:
                        quad.reverse()
                    faces.append((quad[0], quad[1], quad[2]))
                    faces.append((quad[0], quad[2], quad[3]))
    return (np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3))


def to_output(verts_index, shape):
    """(fz, fy, fx) index rows -> [x, y, z] = [2 fx / (W - 1) - 1, 2 fy / (H - 1) - 1, 2 fz / (D - 1) - 1], the map of voxel_tensor_to_point_clouds."""
    D, H, W = shape
    vi = np.asarray(verts_index, np.float64).reshape(-1, 3)
    return np.stack([2.0 * vi[:, 2] / (W - 1) - 1.0, 2.0 * vi[:, 1] / (H - 1) - 1.0, 2.0 * vi[:, 0] / (D - 1) - 1.0], axis=1)


def surface_nets(v, thr):
    """-> (vertices (V, 3) float64 rows [x, y, z] in output coordinates, faces (F, 3) int32)."""
    vi, f = surface_nets_index(v, thr)
    return to_output(vi, np.asarray(v).shape), f


def capacities(shape):
    """(most vertices, most quads) a grid of this shape can have."""
    D, H, W = shape
    return (D + 1) * (H + 1) * (W + 1), (W + 1) * H * D + (H + 1) * D * W + (D + 1) * H * W


def mesh_invariants(vertices, faces):
    """V, F, E (undirected edges), chi = V - E + F, closed (every directed edge occurs as often as its reverse: closed and consistently
    oriented), max_edge_use (most triangles on one undirected edge) and the signed volume sum v0 . (v1 x v2) / 6."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    assert f.size == 0 or (f.min() >= 0 and f.max() < v.shape[0]), "a face indexes outside the vertex list"
    n = max(v.shape[0], 1)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                                  # the directed edges (a, b) of every triangle
    closed = bool(np.array_equal(np.sort(a * n + b), np.sort(b * n + a)))              # the multiset of edges equals that of their reverses
    use = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_counts=True)[1]
    t = v[f]
    volume = float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)
    return dict(V=int(v.shape[0]), F=int(f.shape[0]), E=int(use.size), chi=int(v.shape[0]) - int(use.size) + int(f.shape[0]),
                closed=closed, max_edge_use=int(use.max()) if use.size else 0, volume=volume)


# ------------------------------------------------------------------ lattice inputs
def lattice(values, thr=THR):
    """float32 grid of `values`, after asserting what makes the fp32 kernel and this float64 statement comparable without conditioning: every value
    a multiple of 1/64 in [0, 1] and none within 1/128 of the threshold (so both precisions classify every node alike), and every crossing edge
    of the padded field with |v_B - v_A| >= 1/64 (thr - v_A and v_B - v_A are exact in fp32: t is one correctly rounded division).  A violated
    precondition is an error of the test that built the input."""
    v = np.asarray(values, np.float64)
    assert v.ndim == 3 and min(v.shape) > 1
    assert np.array_equal(np.round(v * 64.0), v * 64.0) and v.min() >= 0.0 and v.max() <= 1.0, "values must be multiples of 1/64 in [0, 1]"
    assert float(np.float32(thr)) == thr and thr > 0.0, "the threshold must be positive and exact in fp32"
    assert np.abs(v - thr).min() >= 1.0 / 128.0 and thr >= 1.0 / 128.0, "a value (or the padding's 0) lies within 1/128 of the threshold"
    p = np.zeros(tuple(n + 2 for n in v.shape))
    p[1:-1, 1:-1, 1:-1] = v
    inside = p > thr
    for axis in range(3):
        a, b = np.moveaxis(p, axis, 0)[:-1], np.moveaxis(p, axis, 0)[1:]
        cross = np.moveaxis(inside, axis, 0)[:-1] != np.moveaxis(inside, axis, 0)[1:]
        assert not cross.any() or np.abs(b - a)[cross].min() >= 1.0 / 64.0, "a crossing edge is shorter than 1/64 in value"
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def lattice_sphere(n=12, centre=(5.3, 5.6, 5.9), radius=4.2):
    """clip(0.5 + (radius - r) / 2, 0, 1) rounded to 1/64, r the distance from `centre` (z, y, x); its THR level set is the sphere of radius
    radius + 2 (0.5 - THR) = radius + 0.203125."""
    zz, yy, xx = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    r = np.sqrt((zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2)
    return lattice(np.round(np.clip(0.5 + (radius - r) / 2.0, 0.0, 1.0) * 64.0) / 64.0)


def lattice_random(shape, seed):
    """Uniform multiples of 1/64 in [0, 1]: many cells whose inside corners are not connected (the ambiguous ones)."""
    return lattice(np.random.default_rng(seed).integers(0, 65, size=shape) / 64.0)


def checkerboard(shape):
    """1 where z + y + x is even: every interior edge crosses -- the most active cells and the most faces a grid can have."""
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return lattice(((zz + yy + xx) % 2 == 0).astype(np.float64))


def single_voxel(shape, at):
    v = np.zeros(shape)
    v[tuple(at)] = 1.0
    return lattice(v)
