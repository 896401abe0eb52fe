"""The literal float64 statement of the mesh-input definitions (DESIGN.md "Mesh input"; include/pcd_hip.h pcd_mesh_voxelize,
pcd_mesh_sample_points): plain loops over (triangle, voxel) and (triangle, column) for small grids, a vectorised form of the same arithmetic
for R = 32, the per-voxel margins that say how far a voxel's decision is from flipping, and the sampler.

Coordinates.  Everything here works on index coordinates p = (v - lo) * inv_pitch, rows [x, y, z] (`index_coords`); node (z, y, x) of the
[z][y][x] grid sits at p = (x, y, z).

Surface.  Node on iff some triangle meets the closed cube of side 1 centred on it.  With a, b, c the triangle's vertices relative to the node, 13 axes:
  box normal k                 projections a_k, b_k, c_k, radius 1/2
  triangle normal n = u x v    (u = b - a, v = c - a) projection n . a (the same for all three vertices), radius (|n_x| + |n_y| + |n_z|) / 2
  e x X, e x Y, e x Z          for e = b - a, c - b, a - c: projections e_z q_y - e_y q_z, e_x q_z - e_z q_x, e_y q_x - e_x q_y of q = a, b, c;
                               radius (|e_z| + |e_y|) / 2, (|e_x| + |e_z|) / 2, (|e_y| + |e_x|) / 2
An axis separates iff min projection > radius or max projection < -radius; the triangle meets the cube iff no axis separates (touching counts).
The slack of an axis is min(radius - min, max + radius) (negative: the gap by which it separates); divided by the sum of the absolute values of
the terms that enter it (the `scale`: for a box normal |vertex coordinate| + |node coordinate| + 1/2, for the others the absolute products of
the worst vertex plus the radius) it is the axis's normalised slack; an axis whose scale is 0 (a zero axis) never separates and is left out.
The signed margin of (triangle, node) is the least normalised slack (>= 0: they meet); of a node, the greatest signed margin over the
triangles: >= 0 iff the node is on, and |.| is how far, relative to the numbers compared, the decision is from flipping.

Interior.  For node (z, y, x) and a triangle with n_z = u_x v_y - u_y v_x != 0: a, b, c relative to (x, y); b and c swapped when n_z < 0; edge
functions E(p, q) = p_x q_y - p_y q_x for (a, b), (b, c), (c, a); the point is covered iff every E > 0, or E = 0 on an edge with d_y < 0, or
d_y = 0 and d_x > 0 (d = q - p).  A covering triangle counts sign(n_z) iff sign(n_z) g > 0, g = (n_x a_x + n_y a_y) + n_z (a_z - z) with a
relative to (x, y) -- the plane's height over the point is strictly above the node.  Node on iff the sum is not 0.
"""
import numpy as np

INF = float("inf")


def index_coords(vertices, resolution, bounds=(-1.0, 1.0)):
    """float64 rows [x, y, z] of index coordinates, with the fp32 inv_pitch the entry point is handed."""
    lo, hi = float(bounds[0]), float(bounds[1])
    inv_pitch = float(np.float32((resolution - 1) / (hi - lo)))
    return (np.asarray(vertices, np.float64).reshape(-1, 3) - lo) * inv_pitch


# ------------------------------------------------------------------ plain loops
def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def tri_cube_axes(A, B, C, node):
    """The 13 axes of triangle (A, B, C) against the unit cube centred on `node` (all [x, y, z] python floats):
    list of (min projection, max projection, radius, scale)."""
    a, b, c = ([q[k] - node[k] for k in range(3)] for q in (A, B, C))
    out = []
    for k in range(3):
        out.append((min(a[k], b[k], c[k]), max(a[k], b[k], c[k]), 0.5, max(abs(A[k]), abs(B[k]), abs(C[k])) + abs(node[k]) + 0.5))
    u, v = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
    n = _cross(u, v)
    d = (n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]
    rn = 0.5 * ((abs(n[0]) + abs(n[1])) + abs(n[2]))
    out.append((d, d, rn, abs(n[0] * a[0]) + abs(n[1] * a[1]) + abs(n[2] * a[2]) + rn))
    for e in (u, [c[k] - b[k] for k in range(3)], [a[k] - c[k] for k in range(3)]):
        for i, j in ((1, 2), (2, 0), (0, 1)):                       # e x X: e_z q_y - e_y q_z, and cyclically
            p = [e[j] * q[i] - e[i] * q[j] for q in (a, b, c)]
            rad = 0.5 * (abs(e[j]) + abs(e[i]))
            out.append((min(p), max(p), rad, max(abs(e[j] * q[i]) + abs(e[i] * q[j]) for q in (a, b, c)) + rad))
    return out


def tri_cube_signed_margin(A, B, C, node):
    m = INF
    for lo, hi, rad, scale in tri_cube_axes(A, B, C, node):
        if scale > 0.0:
            m = min(m, min(rad - lo, hi + rad) / scale)
    return m


def tri_meets_cube(A, B, C, node):
    return all(not (lo > rad or hi < -rad) for lo, hi, rad, _ in tri_cube_axes(A, B, C, node))


def _triangles(p, faces):
    p = np.asarray(p, np.float64).reshape(-1, 3).tolist()
    return [(p[i], p[j], p[k]) for i, j, k in np.asarray(faces, np.int64).reshape(-1, 3).tolist()]


def voxelize_surface(p, faces, R):
    """bool [z][y][x]: plain loops over (triangle, voxel)."""
    out = np.zeros((R, R, R), bool)
    for A, B, C in _triangles(p, faces):
        for z in range(R):
            for y in range(R):
                for x in range(R):
                    if not out[z, y, x] and tri_meets_cube(A, B, C, (float(x), float(y), float(z))):
                        out[z, y, x] = True
    return out


def _edge_covers(p, q):
    e = p[0] * q[1] - p[1] * q[0]
    dx, dy = q[0] - p[0], q[1] - p[1]
    return e > 0.0 or (e == 0.0 and (dy < 0.0 or (dy == 0.0 and dx > 0.0)))


def winding(p, faces, R):
    """int [z][y][x]: plain loops over (triangle, column), then the nodes of the column."""
    out = np.zeros((R, R, R), np.int64)
    for A, B, C in _triangles(p, faces):
        u, v = [B[k] - A[k] for k in range(3)], [C[k] - A[k] for k in range(3)]
        n = _cross(u, v)
        if n[2] == 0.0:
            continue
        s = 1 if n[2] > 0.0 else -1
        for y in range(R):
            for x in range(R):
                a, b, c = ((q[0] - x, q[1] - y) for q in (A, B, C))
                if s < 0:
                    b, c = c, b
                if not (_edge_covers(a, b) and _edge_covers(b, c) and _edge_covers(c, a)):
                    continue
                t0 = n[0] * (A[0] - x) + n[1] * (A[1] - y)
                for z in range(R):
                    if s * (t0 + n[2] * (A[2] - z)) > 0.0:
                        out[z, y, x] += s
    return out


def voxelize_interior(p, faces, R):
    return winding(p, faces, R) != 0


def voxelize_solid(p, faces, R):
    return voxelize_surface(p, faces, R) | voxelize_interior(p, faces, R)


# ------------------------------------------------------------------ vectorised form, with margins
def _nodes(R):
    z, y, x = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    return np.stack([x, y, z], axis=-1).astype(np.float64)                  # [z][y][x][(x, y, z)]


def _norm_slack(lo, hi, rad, scale):
    slack = np.minimum(rad - lo, hi + rad)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0.0, slack / np.where(scale > 0.0, scale, 1.0), INF)


def tri_cube_signed_margin_vec(A, B, C, nodes):
    """`tri_cube_signed_margin` for an array of nodes (..., 3)."""
    A, B, C = (np.asarray(q, np.float64) for q in (A, B, C))
    a, b, c = A - nodes, B - nodes, C - nodes
    m = np.full(nodes.shape[:-1], INF)
    for k in range(3):
        m = np.minimum(m, _norm_slack(np.minimum(np.minimum(a[..., k], b[..., k]), c[..., k]), np.maximum(np.maximum(a[..., k], b[..., k]), c[..., k]),
                                      0.5, max(abs(A[k]), abs(B[k]), abs(C[k])) + np.abs(nodes[..., k]) + 0.5))
    u, v = b - a, c - a
    n = np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                  u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)
    d = (n[..., 0] * a[..., 0] + n[..., 1] * a[..., 1]) + n[..., 2] * a[..., 2]
    rn = 0.5 * ((np.abs(n[..., 0]) + np.abs(n[..., 1])) + np.abs(n[..., 2]))
    m = np.minimum(m, _norm_slack(d, d, rn, np.abs(n[..., 0] * a[..., 0]) + np.abs(n[..., 1] * a[..., 1]) + np.abs(n[..., 2] * a[..., 2]) + rn))
    for e in (u, c - b, a - c):
        for i, j in ((1, 2), (2, 0), (0, 1)):
            p = [e[..., j] * q[..., i] - e[..., i] * q[..., j] for q in (a, b, c)]
            rad = 0.5 * (np.abs(e[..., j]) + np.abs(e[..., i]))
            scale = np.maximum.reduce([np.abs(e[..., j] * q[..., i]) + np.abs(e[..., i] * q[..., j]) for q in (a, b, c)]) + rad
            m = np.minimum(m, _norm_slack(np.minimum.reduce(p), np.maximum.reduce(p), rad, scale))
    return m


def surface_signed_margin(p, faces, R):
    """float [z][y][x]: the greatest signed margin over the triangles; >= 0 iff the node is on.  A triangle is evaluated on the nodes within 2 of
    its bounding box; further out a box normal separates it by a gap of at least 3/2 and it cannot decide a margin below 1e-2 (-inf is left)."""
    nodes = _nodes(R)
    best = np.full((R, R, R), -INF)
    for A, B, C in _triangles(p, faces):
        q = np.asarray([A, B, C])
        lo = np.clip(np.floor(q.min(axis=0)).astype(int) - 2, 0, R)
        hi = np.clip(np.ceil(q.max(axis=0)).astype(int) + 3, 0, R)
        if np.any(hi <= lo):
            continue
        box = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
        best[box] = np.maximum(best[box], tri_cube_signed_margin_vec(A, B, C, nodes[box]))
    return best


def voxelize_surface_vec(p, faces, R):
    """-> (bool [z][y][x], margin [z][y][x])"""
    s = surface_signed_margin(p, faces, R)
    return s >= 0.0, np.abs(s)


def winding_vec(p, faces, R):
    """-> (int [z][y][x], margin [z][y][x]): the margin of a node is the least, over the triangles with n_z != 0, of the margin of the conjunction
    (edge, edge, edge, plane): all true -> the least normalised magnitude of the four, otherwise the greatest among the false ones."""
    nodes = _nodes(R)
    X, Y, Z = nodes[0, :, :, 0], nodes[0, :, :, 1], np.arange(R, dtype=np.float64)[:, None, None]
    out = np.zeros((R, R, R), np.int64)
    margin = np.full((R, R, R), INF)
    for A, B, C in _triangles(p, faces):
        u, v = [B[k] - A[k] for k in range(3)], [C[k] - A[k] for k in range(3)]
        n = _cross(u, v)
        if n[2] == 0.0:
            continue
        s = 1 if n[2] > 0.0 else -1
        a, b, c = ((q[0] - X, q[1] - Y) for q in (A, B, C))
        if s < 0:
            b, c = c, b
        truth, size = [], []
        for (px, py), (qx, qy) in ((a, b), (b, c), (c, a)):
            e = px * qy - py * qx
            dx, dy = qx - px, qy - py
            truth.append(np.broadcast_to(((e > 0.0) | ((e == 0.0) & ((dy < 0.0) | ((dy == 0.0) & (dx > 0.0)))))[None], (R, R, R)))
            size.append(np.broadcast_to((np.abs(e) / (np.abs(px * qy) + np.abs(py * qx) + 1e-300))[None], (R, R, R)))
        t0 = n[0] * a[0] + n[1] * a[1]
        g = t0[None] + n[2] * (A[2] - Z)
        truth.append(s * g > 0.0)
        size.append(np.abs(g) / (np.abs(n[0] * a[0]) + np.abs(n[1] * a[1]) + np.abs(n[2] * A[2]) + np.abs(n[2] * Z) + 1e-300))
        truth, size = np.stack(truth), np.stack(size)
        counts = truth.all(axis=0)
        out += s * counts
        margin = np.minimum(margin, np.where(counts, size.min(axis=0), np.where(truth, -INF, size).max(axis=0)))
    return out, margin


def voxelize_interior_vec(p, faces, R):
    w, m = winding_vec(p, faces, R)
    return w != 0, m


# ------------------------------------------------------------------ sampling
def running_areas(vertices, faces):
    """float64 inclusive running sum of the triangle areas |e0 x e1| / 2, in face order."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = v[np.asarray(faces, np.int64).reshape(-1, 3)]
    return np.cumsum(0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1))


def points_on(vertices, faces, index, u):
    """The points (1 - s) A + s (1 - u2) B + s u2 C, s = sqrt(u1), on the faces `index`, and those faces' unit normals (zero for zero area)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = v[np.asarray(faces, np.int64).reshape(-1, 3)[np.asarray(index, np.int64)]]
    u = np.asarray(u, np.float64).reshape(-1, 3)
    s = np.sqrt(u[:, 1])[:, None]
    w = u[:, 2][:, None]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return (1.0 - s) * t[:, 0] + s * (1.0 - w) * t[:, 1] + s * w * t[:, 2], np.where(length > 0.0, n / np.where(length > 0.0, length, 1.0), 0.0)


def sample_points(vertices, faces, u):
    """u (N, 3) in [0, 1) -> (face index (N,), points (N, 3)): the first face whose running sum exceeds u0 * total; a mesh of total area 0 puts
    every point on the first vertex of its first face."""
    run = running_areas(vertices, faces)
    u = np.asarray(u, np.float64).reshape(-1, 3)
    if run[-1] <= 0.0:
        v = np.asarray(vertices, np.float64).reshape(-1, 3)
        return np.zeros(len(u), np.int64), np.repeat(v[np.asarray(faces).reshape(-1, 3)[0, 0]][None], len(u), axis=0)
    index = np.minimum(np.searchsorted(run, u[:, 0] * run[-1], side="right"), len(run) - 1)
    return index, points_on(vertices, faces, index, u)[0]


# ------------------------------------------------------------------ hand-worked and random inputs
CUBE_FACES = np.asarray([(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (2, 3, 7), (2, 7, 6), (1, 2, 6), (1, 6, 5),
                         (0, 4, 7), (0, 7, 3)], np.int32)


def cube(lo, hi, inside_out=False):
    """Closed box [lo, hi]^3 (scalars or 3-vectors), 8 vertices rows [x, y, z], 12 triangles with outward normals (inward when inside_out)."""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (3,)), np.broadcast_to(np.asarray(hi, np.float64), (3,))
    v = np.asarray([(lo[0], lo[1], lo[2]), (hi[0], lo[1], lo[2]), (hi[0], hi[1], lo[2]), (lo[0], hi[1], lo[2]),
                    (lo[0], lo[1], hi[2]), (hi[0], lo[1], hi[2]), (hi[0], hi[1], hi[2]), (lo[0], hi[1], hi[2])])
    f = CUBE_FACES[:, ::-1].copy() if inside_out else CUBE_FACES.copy()
    return v, f


def merge(*meshes):
    """One mesh from several: vertices stacked, faces re-based."""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float64).reshape(-1, 3))
        fs.append(np.asarray(f, np.int32).reshape(-1, 3) + base)
        base += vs[-1].shape[0]
    return np.concatenate(vs), np.concatenate(fs)


def lattice_triangles(count, seed):
    """`count` random triangles with vertices on multiples of 1/2 in [-1, 8]: with R = 8 and bounds (0, 7) (index = coordinate) every product and
    sum of the predicates is exact in fp32 -- differences 6 bits, products 12, normal 13, plane dot 21."""
    g = np.random.default_rng(seed)
    v = g.integers(-2, 17, size=(3 * count, 3)) / 2.0
    return v, np.arange(3 * count, dtype=np.int32).reshape(-1, 3)


def conditioned_triangles(count, seed, R=32):
    """`count` random float32 triangles inside [-1, 1]^3 with edges of 2 to 10 voxel pitches (not closed): a first vertex anywhere, the other two at
    a distance of 2 .. 10 pitches from it in random directions, each redrawn until it lies inside the cube."""
    g = np.random.default_rng(seed)
    pitch = 2.0 / (R - 1)
    verts = np.zeros((count, 3, 3))
    for t in range(count):
        verts[t, 0] = g.uniform(-0.9, 0.9, 3)
        for k in (1, 2):
            while True:
                d = g.normal(size=3)
                q = verts[t, 0] + d / np.linalg.norm(d) * g.uniform(2.0, 7.0) * pitch
                if np.abs(q).max() <= 1.0 and (k == 1 or 2.0 * pitch <= np.linalg.norm(q - verts[t, 1]) <= 10.0 * pitch):
                    verts[t, k] = q
                    break
    return verts.reshape(-1, 3).astype(np.float32), np.arange(3 * count, dtype=np.int32).reshape(-1, 3)
