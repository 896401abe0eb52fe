"""The definitions of DESIGN.md "Mesh processing" in numpy, written from that text (not from the kernels): valid faces, vertex rings,
Taubin smoothing, vertex normals, connected components, compaction and measures of one mesh (vertices (V, 3), faces (F, 3)).

Smoothing and normals come in two forms: `dtype=np.float32` mirrors the stated fp32 evaluation, every operation one numpy float32
operation in the stated order; `dtype=np.float64` is the same formula in double."""
import numpy as np

REFERENCED, BOUNDARY, IRREGULAR = 1, 2, 4


def valid_faces(nv, faces):
    """mask (F,): all three indices are rows of the mesh and pairwise different."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < nv)).all(axis=1)
    return inside & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def adjacency(nv, faces):
    """-> dict: nbr_start (V + 1,), nbr_index (E,), nbr_counts (E, 2) = (out, in) per entry, rows ascending in the neighbour; inc_start
    (V + 1,), inc_faces in ascending face order; flags (V,)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(nv, f)
    fv = f[ok]
    a, b = fv.reshape(-1), fv[:, [1, 2, 0]].reshape(-1)                      # the directed edges a -> b of the valid faces
    # an entry (vertex, neighbour): `out` counts the edges vertex -> neighbour, `in` the edges neighbour -> vertex
    key = np.concatenate([a * max(nv, 1) + b, b * max(nv, 1) + a])
    is_out = np.concatenate([np.ones(a.size, bool), np.zeros(a.size, bool)])
    uniq, inverse = np.unique(key, return_inverse=True)
    out = np.bincount(inverse[is_out], minlength=uniq.size)
    inn = np.bincount(inverse[~is_out], minlength=uniq.size)
    owner, nbr = uniq // max(nv, 1), uniq % max(nv, 1)
    nbr_start = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=nv))]).astype(np.int64)
    corner_vertex = fv.reshape(-1)
    corner_face = np.repeat(np.nonzero(ok)[0], 3)
    order = np.lexsort((corner_face, corner_vertex))
    inc_start = np.concatenate([[0], np.cumsum(np.bincount(corner_vertex, minlength=nv))]).astype(np.int64)
    flags = np.zeros(nv, np.int32)
    flags[np.unique(corner_vertex)] |= REFERENCED
    flags[np.unique(owner[out + inn == 1])] |= BOUNDARY
    flags[np.unique(owner[(out != 1) | (inn != 1)])] |= IRREGULAR
    return dict(nbr_start=nbr_start, nbr_index=nbr.astype(np.int32), nbr_counts=np.stack([out, inn], axis=1).astype(np.int32),
                inc_start=inc_start, inc_faces=corner_face[order].astype(np.int32), flags=flags)


def _padded(start, index):
    """rows -> (V, widest) index table and the row lengths."""
    n = np.diff(start)
    table = np.zeros((n.size, max(int(n.max()) if n.size else 0, 1)), np.int64)
    for k in range(table.shape[1]):
        has = n > k
        table[has, k] = index[start[:-1][has] + k]
    return table, n


def smooth(vertices, faces, iterations, lam, mu, pin_boundary=False, dtype=np.float32):
    """`iterations` rounds of a lam step then (mu != 0) a mu step.  Per step and component: s = +0; s = s + x[u] over the row in ascending u;
    m = s / n; x' = x + f (m - x); all vertices read the old positions.  Empty rows, and with `pin_boundary` boundary vertices, keep theirs."""
    x = np.array(vertices, dtype).reshape(-1, 3)
    adj = adjacency(x.shape[0], faces)
    table, n = _padded(adj["nbr_start"], adj["nbr_index"])
    moves = n > 0
    if pin_boundary:
        moves &= (adj["flags"] & BOUNDARY) == 0
    factors = [dtype(lam)] + ([dtype(mu)] if mu != 0 else [])
    nf = n.astype(dtype)
    for _ in range(int(iterations)):
        for f in factors:
            s = np.zeros_like(x)
            for k in range(table.shape[1]):
                has = n > k
                s[has] = s[has] + x[table[has, k]]
            new = x.copy()
            m = s[moves] / nf[moves, None]
            new[moves] = x[moves] + f * (m - x[moves])
            x = new
    assert x.dtype == dtype
    return x


def vertex_normals(vertices, faces, dtype=np.float32):
    """Per vertex, over its incident valid faces in ascending order: n = n + (e1 x e2), e1 = b - a, e2 = c - a, every product rounded before
    its subtraction, from +0; len = sqrt((nx nx + ny ny) + nz nz); n / len, zeros where len is 0 or the vertex is unreferenced."""
    x = np.array(vertices, dtype).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    adj = adjacency(x.shape[0], f)
    table, n = _padded(adj["inc_start"], adj["inc_faces"])
    fs = np.clip(f, 0, max(x.shape[0] - 1, 0))                               # invalid faces are never in a row
    e1, e2 = (x[fs[:, 1]] - x[fs[:, 0]], x[fs[:, 2]] - x[fs[:, 0]]) if x.shape[0] else (np.zeros((0, 3), dtype),) * 2
    cross = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    s = np.zeros_like(x)
    for k in range(table.shape[1]):
        has = n > k
        s[has] = s[has] + cross[table[has, k]]
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    out = np.zeros_like(x)
    ok = (n > 0) & (length != 0)
    out[ok] = s[ok] / length[ok, None]
    assert out.dtype == dtype
    return out


def components(nv, faces):
    """-> labels (V,) int32 (the least vertex index of the component, -1 unreferenced), the number of components, and sizes (V,) int32: at a
    label root the valid faces of its component, 0 elsewhere.  By repeated minimum over the faces until nothing changes."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fv = f[valid_faces(nv, f)]
    label = np.full(nv, nv, np.int64)
    label[np.unique(fv)] = np.unique(fv)
    for _ in range(nv + 1):
        low = label[fv].min(axis=1) if fv.size else np.zeros(0, np.int64)
        new = label.copy()
        for k in range(3):
            np.minimum.at(new, fv[:, k], low)
        new = np.where(new < nv, new[np.minimum(new, nv - 1)], new) if nv else new     # one pointer jump
        if np.array_equal(new, label):
            break
        label = new
    labels = np.where(label < nv, label, -1).astype(np.int32)
    sizes = np.bincount(labels[fv[:, 0]], minlength=nv).astype(np.int32) if fv.size else np.zeros(nv, np.int32)
    return labels, int((labels == np.arange(nv)).sum()), sizes


def keep_flags(nv, faces, min_faces=None, keep_largest=False):
    """The keep flag of every vertex under one of the two rules; unreferenced vertices are never kept."""
    labels, _, sizes = components(nv, faces)
    roots = np.nonzero(labels == np.arange(nv))[0]
    if keep_largest:
        if roots.size == 0:
            return np.zeros(nv, bool)
        best = roots[np.lexsort((roots, -sizes[roots]))[0]]                 # most faces, then the smaller label
        return labels == best
    return (labels >= 0) & (sizes[np.maximum(labels, 0)] >= min_faces)


def compact(vertices, faces, keep):
    """The kept vertices in order; in order the valid faces whose three vertices are all kept, renumbered."""
    v = np.asarray(vertices).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = np.asarray(keep) != 0
    new = np.cumsum(keep) - 1
    fv = f[valid_faces(v.shape[0], f)]
    fv = fv[keep[fv].all(axis=1)] if fv.size else fv
    return v[keep], new[fv].astype(np.int32).reshape(-1, 3)


def measures(vertices, faces):
    """float64 area, volume, centroid and sum |term| of each (for the tolerance), and the integer measures."""
    x = np.asarray(vertices, np.float64).reshape(-1, 3)
    nv = x.shape[0]
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fv = f[valid_faces(nv, f)]
    a, b, c = (x[fv[:, k]] for k in range(3)) if fv.size else (np.zeros((0, 3)),) * 3
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1) / 2.0
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)) / 6.0
    moment = area[:, None] * (a + b + c) / 3.0
    adj = adjacency(nv, f)
    out, inn = adj["nbr_counts"][:, 0], adj["nbr_counts"][:, 1]
    owner = np.repeat(np.arange(nv), np.diff(adj["nbr_start"]))
    once = adj["nbr_index"] > owner
    refd, edges, nfaces = int((adj["flags"] & REFERENCED != 0).sum()), int(out.size // 2), int(fv.shape[0])
    return dict(area=float(area.sum()), volume=float(vol.sum()),
                centroid=moment.sum(axis=0) / area.sum() if area.sum() > 0 else np.zeros(3),
                abs_area=float(area.sum()), abs_volume=float(np.abs(vol).sum()), abs_moment=np.abs(moment).sum(axis=0),
                vertices=refd, edges=edges, faces=nfaces, boundary_edges=int(((out + inn == 1) & once).sum()),
                irregular_edges=int((((out != 1) | (inn != 1)) & once).sum()), components=components(nv, f)[1],
                euler=refd - edges + nfaces, closed=int(np.array_equal(out, inn)))
