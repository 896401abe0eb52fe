"""The definitions of DESIGN.md "Mesh simplification" in numpy, written from that text (not from the kernels): the grid in fp32, clusters
and faces in integers, positions in fp64 with every operation one numpy operation in the stated order.  Every ordered sum is `np.add.at`
over indices in the stated order (it adds one element after the other; `np.sum` adds pairwise and is not the statement)."""
import numpy as np

from mesh_ops_statement import valid_faces

MAX_R = 1024
F32 = np.float32


def _faces(vertices, faces):
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return v, f, valid_faces(v.shape[0], f)


def box(vertices, faces):
    """-> lo (3,) fp32, ext fp32 and the referenced mask.  lo / hi start at +inf / -inf and take x where x < lo / x > hi (false for NaN);
    ext starts at -inf and takes hi - lo where that is larger."""
    v, f, ok = _faces(vertices, faces)
    ref = np.zeros(v.shape[0], bool)
    ref[f[ok].reshape(-1)] = True
    lo, hi = np.full(3, np.inf, F32), np.full(3, -np.inf, F32)
    with np.errstate(all="ignore"):
        if ref.any():
            lo = np.fmin(lo, np.fmin.reduce(v[ref], axis=0))                 # fmin / fmax skip NaN; the order cannot matter
            hi = np.fmax(hi, np.fmax.reduce(v[ref], axis=0))
        ext = F32(-np.inf)
        for d in (hi - lo).astype(F32):
            if d > ext:
                ext = d
    return lo, F32(ext), ref


def grid(vertices, faces, resolution=None, cell_size=None):
    """-> lo, h (fp32), R, referenced mask"""
    lo, ext, ref = box(vertices, faces)
    with np.errstate(all="ignore"):
        if cell_size is not None:
            h = F32(cell_size)
            e = F32(ext / h)
            r = 1 if not np.isfinite(ext) else (MAX_R if e >= F32(MAX_R - 1) else int(np.floor(e)) + 1)
        else:
            r = int(resolution)
            h = F32(ext / F32(r))
            if ext == 0 or not np.isfinite(ext):
                h = F32(1)
    return lo, h, r, ref


def cell_keys(vertices, lo, h, r):
    """cell coordinates (V, 3) and keys (V,) of every vertex"""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = ((v - lo).astype(F32) / h).astype(F32)
        inside = (q >= 0) & (q < F32(r))
        c = np.where(inside, np.floor(np.where(inside, q, 0)), np.where(q >= F32(r), r - 1, 0)).astype(np.int64)   # !(q >= 0): 0, NaN too
    return c, (c[:, 2] * r + c[:, 1]) * r + c[:, 0]


def clusters(vertices, faces, resolution=None, cell_size=None):
    """-> dict: map (V,) int32 (cluster number, -1 unreferenced), roots (K,) vertex indices ascending, cells (K, 3) of the roots, lo, h, R"""
    v, f, ok = _faces(vertices, faces)
    lo, h, r, ref = grid(v, f, resolution, cell_size)
    c, key = cell_keys(v, lo, h, r)
    idx = np.nonzero(ref)[0]
    uniq, first, inv = np.unique(key[idx], return_index=True, return_inverse=True)
    roots = idx[first]                                                       # the least vertex index of every key
    order = np.argsort(roots, kind="stable")
    number = np.empty(uniq.size, np.int64)
    number[order] = np.arange(uniq.size)
    cmap = np.full(v.shape[0], -1, np.int32)
    cmap[idx] = number[inv.reshape(-1)]
    roots = roots[order]
    return dict(map=cmap, roots=roots, cells=c[roots], lo=lo, h=h, R=r)


def map_faces(nv, faces, cmap, deduplicate=False):
    """-> (kept face indices, mapped faces int32): valid faces in order, those with two equal numbers dropped; with `deduplicate` only the
    first of every oriented triple up to rotation."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    idx = np.nonzero(valid_faces(nv, f))[0]
    g = cmap[f[idx]].astype(np.int64).reshape(-1, 3)
    keep = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    idx, g = idx[keep], g[keep]
    if deduplicate and idx.size:
        s = np.argmin(g, axis=1)
        rot = np.stack([g[np.arange(g.shape[0]), (s + k) % 3] for k in range(3)], axis=1)
        _, first = np.unique(rot, axis=0, return_index=True)
        first = np.sort(first)
        idx, g = idx[first], g[first]
    return idx, g.astype(np.int32).reshape(-1, 3)


def face_quadrics(vertices, faces):
    """(F, 9) fp64 = A00 A01 A02 A11 A12 A22 b0 b1 b2 per face; zeros for invalid faces and faces without area"""
    v, f, ok = _faces(vertices, faces)
    q = np.zeros((f.shape[0], 9), np.float64)
    x = v.astype(np.float64)
    fv = f[ok]
    with np.errstate(all="ignore"):
        a, b, c = (x[fv[:, k]] for k in range(3)) if fv.size else (np.zeros((0, 3)),) * 3
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ux, uy, uz, w = nx / length, ny / length, nz / length, 0.5 * length
        d = (ux * a[:, 0] + uy * a[:, 1]) + uz * a[:, 2]
        wx, wy, wz, wd = w * ux, w * uy, w * uz, w * d
        rows = np.stack([wx * ux, wx * uy, wx * uz, wy * uy, wy * uz, wz * uz, wd * ux, wd * uy, wd * uz], axis=1)
    rows[length == 0] = 0.0                                                  # contributes nothing (adding +0 changes no sum that starts at +0)
    q[ok] = rows
    return q


def positions(vertices, faces, cl, placement="quadric"):
    """(K, 3) fp32 cluster vertices and, for the tests, the fp64 pieces: mean, regularised A', b', the solution and whether it was taken."""
    v, f, ok = _faces(vertices, faces)
    k = cl["roots"].size
    x = v.astype(np.float64)
    vq = np.zeros((v.shape[0], 9), np.float64)
    fq = face_quadrics(v, f)
    fidx = np.nonzero(ok)[0]
    np.add.at(vq, f[fidx].reshape(-1), np.repeat(fq[fidx], 3, axis=0))       # per vertex: ascending face order
    members = np.nonzero(cl["map"] >= 0)[0]                                  # ascending vertex order
    cm = cl["map"][members]
    s, cq, count = np.zeros((k, 3)), np.zeros((k, 9)), np.zeros(k)
    with np.errstate(all="ignore"):
        np.add.at(s, cm, x[members])
        np.add.at(cq, cm, vq[members])
        np.add.at(count, cm, 1.0)
        mean = s / count[:, None]
        out = mean.copy()
        info = dict(mean=mean, taken=np.zeros(k, bool))
        if placement == "quadric":
            t = (cq[:, 0] + cq[:, 3]) + cq[:, 5]
            reg = 1e-3 * t
            a00, a01, a02, a11, a12, a22 = cq[:, 0] + reg, cq[:, 1], cq[:, 2], cq[:, 3] + reg, cq[:, 4], cq[:, 5] + reg
            b0, b1, b2 = cq[:, 6] + reg * mean[:, 0], cq[:, 7] + reg * mean[:, 1], cq[:, 8] + reg * mean[:, 2]
            c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
            c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
            det = (a00 * c00 + a01 * c01) + a02 * c02
            p = np.stack([((c00 * b0 + c01 * b1) + c02 * b2) / det, ((c01 * b0 + c11 * b1) + c12 * b2) / det,
                          ((c02 * b0 + c12 * b1) + c22 * b2) / det], axis=1)
            lo, h, cells = cl["lo"].astype(np.float64), np.float64(cl["h"]), cl["cells"].astype(np.float64)
            low, high = lo + (cells - 0.5) * h, lo + (cells + 1.5) * h
            take = (t > 0) & (np.isfinite(p) & (p >= low) & (p <= high)).all(axis=1)
            out[take] = p[take]
            info.update(taken=take, solution=p, A=np.stack([a00, a01, a02, a01, a11, a12, a02, a12, a22], axis=1).reshape(-1, 3, 3),
                        b=np.stack([b0, b1, b2], axis=1))
        return out.astype(F32), info


def surviving(vertices, faces, r, deduplicate=False):
    cl = clusters(vertices, faces, resolution=r)
    return map_faces(np.asarray(vertices).reshape(-1, 3).shape[0], faces, cl["map"], deduplicate)[0].size


def bisect(vertices, faces, target, deduplicate=False):
    """lo = 1, hi = 1025; ten rounds: mid = (lo + hi) // 2, lo = mid if the surviving faces at mid are <= target, else hi = mid; -> lo"""
    lo, hi = 1, MAX_R + 1
    for _ in range(10):
        mid = (lo + hi) // 2
        if surviving(vertices, faces, mid, deduplicate) <= max(int(target), 0):
            lo = mid
        else:
            hi = mid
    return lo


def simplify(vertices, faces, resolution=None, cell_size=None, target_faces=None, placement="quadric", deduplicate=False):
    """-> dict: vertices (K, 3) fp32, faces (F', 3) int32, map (V,) int32, resolution int, info (the fp64 pieces of `positions`)"""
    assert sum(a is not None for a in (resolution, cell_size, target_faces)) == 1
    v, f, _ = _faces(vertices, faces)
    if target_faces is not None:
        resolution = bisect(v, f, target_faces, deduplicate)
    cl = clusters(v, f, resolution, cell_size)
    pos, info = positions(v, f, cl, placement)
    _, nf = map_faces(v.shape[0], f, cl["map"], deduplicate)
    return dict(vertices=pos, faces=nf, map=cl["map"], resolution=cl["R"], info=info)
