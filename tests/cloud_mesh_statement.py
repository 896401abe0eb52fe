"""The statement of the cloud-to-mesh definition (DESIGN.md "Cloud to mesh"; include/pcd_hip.h pcd_cloud_spacing .. pcd_project_to_cloud) in plain
numpy: fp64 where a value is real, fp32-mirrored where a classification depends on it -- the node coordinates lo + (float)i * h, the squared
distance (dx dx + dy dy) + dz dz, the product r * r and the field expression are evaluated in numpy float32, operation by operation, which
rounds as the kernels do (no contraction).

Grids are bool / int arrays [z][y][x]; `words` packs a bool grid into the kernels' layout, one uint64 per row (z, y), bit x = node x.

Pieces: shell by brute force, outside by breadth-first search from the layer round the grid, D2 by brute-force separable minima over the padded
grid, the field, surface nets through tests/mesh_statement.py, the projection by numpy.linalg.eigh."""
import numpy as np
import torch

import geometry_statement as G
import mesh_statement as M

F32 = np.float32
BOUNDS = (-1.25, 1.25)


def pitch(R, lo=BOUNDS[0], hi=BOUNDS[1]):
    """h = (hi - lo) / (R - 1) in double, rounded to fp32 once"""
    return F32((float(hi) - float(lo)) / (R - 1))


def nodes(R, lo, h):
    """c_i = lo + (float)i * h: the product rounded, then the sum"""
    return F32(lo) + np.arange(R, dtype=F32) * F32(h)


def clamp(r, h, inset):
    """max(r, (2 - inset) * h) in fp32 as written; a NaN r takes the clamp value"""
    floor_r = (F32(2.0) - F32(inset)) * F32(h)
    r = F32(r)
    return floor_r if not r == r or r < floor_r else r


def spacing(points, k=8):
    """The mean over the points that have k valid neighbours of the fp32 root of the k-th neighbour's d2 (the fp32 arithmetic of pcd_knn, the point
    itself left out), summed in double -> (float64 mean, count); (0, 0) without such a point."""
    x = torch.as_tensor(np.asarray(points, F32))
    if x.shape[0] == 0:
        return 0.0, 0
    d2 = G.knn(x, x, k, True)[0][:, k - 1].numpy()
    ok = ~np.isnan(d2)
    if not ok.any():
        return 0.0, 0
    return float(np.sqrt(d2[ok].astype(F32)).astype(np.float64).sum() / ok.sum()), int(ok.sum())


def radius(points, h, radius=None, scale=1.5, inset=0.0):
    """The radius the cloud is closed with, fp32."""
    if radius is None:
        s, have = spacing(points)
        radius = F32(scale) * F32(s) if have else F32(0.0)
    return clamp(radius, h, inset)


def shell_full(points, R, lo, h, r):
    """Brute force over every (point, node) pair: node (z, y, x) is shell iff some finite point has (dx dx + dy dy) + dz dz <= r * r."""
    c = nodes(R, lo, h)
    r2 = F32(r) * F32(r)
    out = np.zeros((R, R, R), bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in np.asarray(points, F32).reshape(-1, 3):
            if not np.isfinite(p).all():
                continue
            dx, dy, dz = c - p[0], c - p[1], c - p[2]
            d2 = (dx * dx)[None, None, :] + (dy * dy)[None, :, None] + (dz * dz)[:, None, None]      # left to right: (dx dx + dy dy) + dz dz
            out |= d2 <= r2
    return out


def shell(points, R, lo, h, r):
    """The same predicate on the same fp32 values, evaluated only on the nodes of a box round each point that is two nodes wider on every side
    than r / h in double: outside it |dx| > r + h on some axis, far beyond any fp32 rounding of the predicate (test_cloud_mesh_statement_cpu
    checks it against `shell_full`)."""
    c = nodes(R, lo, h)
    r2 = F32(r) * F32(r)
    out = np.zeros((R, R, R), bool)
    reach = float(r) / float(h) + 2.0
    if not np.isfinite(reach):
        return shell_full(points, R, lo, h, r)
    for p in np.asarray(points, F32).reshape(-1, 3):
        if not np.isfinite(p).all():
            continue
        f = (p.astype(np.float64) - float(lo)) / float(h)
        a = np.clip(np.floor(f - reach), 0, R).astype(int)
        b = np.clip(np.ceil(f + reach), -1, R - 1).astype(int) + 1
        if (a >= b).any():
            continue
        dx, dy, dz = c[a[0]:b[0]] - p[0], c[a[1]:b[1]] - p[1], c[a[2]:b[2]] - p[2]
        d2 = (dx * dx)[None, None, :] + (dy * dy)[None, :, None] + (dz * dz)[:, None, None]
        out[a[2]:b[2], a[1]:b[1], a[0]:b[0]] |= d2 <= r2
    return out


def outside_bfs(shell_mask):
    """Free = not shell.  Outside = the free nodes 6-connected through free nodes to the layer of free nodes round the grid: breadth-first search
    over the padded grid, level by level, from the whole layer at once (level n + 1 = the free, unseen 6-neighbours of level n)."""
    R = shell_mask.shape[0]
    n = R + 2
    free = np.ones((n, n, n), bool)
    free[1:-1, 1:-1, 1:-1] = ~np.asarray(shell_mask, bool)
    seen = np.ones((n, n, n), bool)
    seen[1:-1, 1:-1, 1:-1] = False
    frontier = seen.copy()
    while frontier.any():
        near = np.zeros_like(frontier)
        near[1:] |= frontier[:-1]
        near[:-1] |= frontier[1:]
        near[:, 1:] |= frontier[:, :-1]
        near[:, :-1] |= frontier[:, 1:]
        near[:, :, 1:] |= frontier[:, :, :-1]
        near[:, :, :-1] |= frontier[:, :, 1:]
        frontier = near & free & ~seen
        seen |= frontier
    return seen[1:-1, 1:-1, 1:-1].copy()


def depth2(outside_mask):
    """D2 int32: the squared Euclidean distance in pitches to the nearest outside node, the layer round the grid counting as outside; separable,
    min_j (g[j] + (i - j)^2) per axis by brute force over the padded grid."""
    R = outside_mask.shape[0]
    n = R + 2
    big = 4 * n * n
    g = np.zeros((n, n, n), np.int64)
    g[1:-1, 1:-1, 1:-1] = np.where(np.asarray(outside_mask, bool), 0, big)
    i = np.arange(n)
    sq = (i[:, None] - i[None, :]) ** 2                                     # [i][j]
    for axis in (2, 1, 0):
        g = np.moveaxis(g, axis, -1)
        g = (g[..., None, :] + sq).min(axis=-1)
        g = np.moveaxis(g, -1, axis)
    return g[1:-1, 1:-1, 1:-1].astype(np.int32)


def field(d2, h, r, inset):
    """v = 0 where D2 = 0, elsewhere 1.0f + ((sqrtf((float)D2) * h - r) - inset * h), every operation in fp32"""
    root = np.sqrt(d2.astype(F32))
    v = F32(1.0) + ((root * F32(h) - F32(r)) - F32(inset) * F32(h))
    return np.where(d2 == 0, F32(0.0), v).astype(F32)


def counts(shell_mask, outside_mask):
    """info = (shell nodes, enclosed nodes, shell nodes on the six faces of the grid)"""
    s = np.asarray(shell_mask, bool)
    inner = s.copy()
    inner[1:-1, 1:-1, 1:-1] = False
    return int(s.sum()), int((~s & ~np.asarray(outside_mask, bool)).sum()), int(inner.sum())


def words(mask):
    """bool [R][R][R] -> uint64 [R][R], bit x of word [z][y] = mask[z][y][x]"""
    m = np.asarray(mask, bool)
    return (m.astype(np.uint64) << np.arange(m.shape[2], dtype=np.uint64)).sum(axis=2, dtype=np.uint64)


def unwords(w, R):
    w = np.asarray(w).view(np.uint64).reshape(-1, R, R)
    return ((w[..., None] >> np.arange(R, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def nets(v, lo=BOUNDS[0], hi=BOUNDS[1]):
    """Surface nets at threshold 1 -> vertices (V, 3) float64 mapped from the nets' [-1, 1] to the bounds, faces (F, 3) int32."""
    verts, faces = M.surface_nets(np.asarray(v, np.float64), 1.0)
    return verts * ((hi - lo) / 2.0) + (lo + hi) / 2.0, faces


def project(verts, points, index):
    """verts (V, 3) fp32, points (n, 3) fp32, index (V, k) -> (projected (V, 3) float64, gap (V,) = (l1 - l0) / l2, NaN where the vertex stayed).
    The neighbours are the entries 0 <= index < n; fewer than 3: the vertex stays."""
    v = np.asarray(verts, F32).astype(np.float64)
    pts = np.asarray(points, F32).astype(np.float64)
    out, gap = v.copy(), np.full(v.shape[0], np.nan)
    for i in range(v.shape[0]):
        idx = np.asarray(index[i])
        idx = idx[(idx >= 0) & (idx < pts.shape[0])]
        if idx.size < 3:
            continue
        nb = pts[idx]
        c = nb.mean(axis=0)
        q = nb - c
        w, vec = np.linalg.eigh(q.T @ q)
        n = vec[:, 0]
        out[i] = v[i] - ((v[i] - c) @ n) * n
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
    return out, gap


def knn_index(verts, points, k):
    """The neighbour lists of the vertices in the cloud, in the fp32 arithmetic of pcd_knn."""
    if len(verts) == 0:
        return np.zeros((0, k), np.int32)
    return G.knn(torch.as_tensor(np.asarray(verts, F32)), torch.as_tensor(np.asarray(points, F32)), k, False)[1].numpy()


def cloud_to_mesh(points, R, radius_=None, scale=1.5, inset=0.0, bounds=BOUNDS, do_project=True, k=8, want_mesh=True):
    """The whole definition for one cloud -> dict(radius, shell, outside, d2, v, info, vertices (fp64, unprojected), faces, projected, gap)."""
    lo, hi = bounds
    h = pitch(R, lo, hi)
    pts = np.asarray(points, F32).reshape(-1, 3)
    r = radius(pts, h, radius_, scale, inset)
    s = shell(pts, R, F32(lo), h, r)
    o = outside_bfs(s)
    d2 = depth2(o)
    v = field(d2, h, r, inset)
    out = dict(radius=r, shell=s, outside=o, d2=d2, v=v, info=counts(s, o))
    if want_mesh:
        out["vertices"], out["faces"] = nets(v, lo, hi)
        if do_project:
            v32 = out["vertices"].astype(F32)
            out["projected"], out["gap"] = project(v32, pts, knn_index(v32, pts, k))
    return out


def flipped_share(before, after, faces):
    """The share of triangles whose normal after the projection points against the one before."""
    if len(faces) == 0:
        return 0.0
    def normal(v):
        t = np.asarray(v, np.float64)[np.asarray(faces, np.int64)]
        return np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return float(((normal(before) * normal(after)).sum(axis=1) < 0).mean())
