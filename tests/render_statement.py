"""The literal statement of the renderer's definition (DESIGN.md "Render"; include/pcd_hip.h pcd_render_points, pcd_render_meshes) in numpy:
float64 by default, `dtype=np.float32` runs the same formulas in fp32 on the CPU.  One loop over the primitives, every pixel of the image (cut
to the primitive's bounding box widened by PAD pixels, outside which it decides nothing and no margin below PAD - 1).

View.  q = ((m0 px + m1 py) + m2 pz) + t per row of the 3 x 4 view; pixel (i, j) has its centre at (j + 1/2, i + 1/2).  A primitive with a
projected coordinate that is not finite is skipped.

Points.  (dx, dy) = c - (qx, qy); covered iff dx dx + dy dy <= r r; depth qz; L = max(0, ((dx lx + dy ly) + nz lz) / r), nz = -sqrt(r r - d2).
The coverage margin is |sqrt(d2) - r|.

Triangles.  u = q1 - q0, v = q2 - q0, n = u x v; n_z = 0 draws nothing.  Edge (P, Q) with third vertex R: A = the lexicographically smaller
(x, y) of P, Q, d = B - A; e(c) = d_x (c_y - A_y) - d_y (c_x - A_x), w = e(R), s = sign(w) (w = 0 draws nothing); inward normal s (-d_y, d_x);
inside iff s e > 0, or e = 0 and (nx > 0, or nx = 0 and ny > 0).  Depth z0 - (n_x (c_x - x0) + n_y (c_y - y0)) / n_z, not covered where that is
not finite; L = |(n_x lx + n_y ly) + n_z lz| / |n|.  The coverage margin is the distance |e| / |d| to the edge lines: inside, the least of the
three; outside, the greatest among the edges that exclude the pixel (all of them have to flip).

Visibility.  The least (depth, index) pair among the covering primitives.  rgb = floor(min(max((255 color) (ambient + (1 - ambient) L), 0), 255)
+ 1/2); background: id -1, depth +inf, round(255 background).

Margins per pixel: `cover_margin`, the least coverage margin over all primitives (how far, in pixels, the nearest boundary that could flip a
coverage decision is), and `depth_gap`, second-nearest minus nearest covering depth (inf with fewer than two).
"""
import numpy as np

INF = float("inf")
PAD = 3
DEFAULT_LIGHT = np.asarray([-0.4, -0.6, -0.7]) / np.linalg.norm([-0.4, -0.6, -0.7])
DEFAULT_COLOR = (0.27, 0.51, 0.71)


def project(view, p, dtype=np.float64):
    """rows [x, y, z] of view space for world rows p, in `dtype`, in the device's order of operations."""
    m = np.asarray(view, np.float32).reshape(3, 4).astype(dtype)
    p = np.asarray(p, np.float32).reshape(-1, 3).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((m[k, 0] * p[:, 0] + m[k, 1] * p[:, 1]) + m[k, 2] * p[:, 2]) + m[k, 3] for k in range(3)], axis=1)


class _Buffers:
    def __init__(self, height, width, dtype):
        self.h, self.w, self.dtype = height, width, dtype
        self.ids = np.full((height, width), -1, np.int64)
        self.depth = np.full((height, width), INF, dtype)
        self.second = np.full((height, width), INF, dtype)
        self.shade = np.zeros((height, width), dtype)
        self.cover_margin = np.full((height, width), INF)

    def box(self, lo_x, hi_x, lo_y, hi_y):
        """slices of the pixels whose centres may lie within PAD of [lo, hi], and their centre coordinates"""
        x0 = int(np.clip(np.floor(lo_x - 0.5) - PAD, 0, self.w)); x1 = int(np.clip(np.ceil(hi_x - 0.5) + PAD + 1, 0, self.w))
        y0 = int(np.clip(np.floor(lo_y - 0.5) - PAD, 0, self.h)); y1 = int(np.clip(np.ceil(hi_y - 0.5) + PAD + 1, 0, self.h))
        if x1 <= x0 or y1 <= y0:
            return None
        cx = (np.arange(x0, x1) + 0.5).astype(self.dtype)[None, :]
        cy = (np.arange(y0, y1) + 0.5).astype(self.dtype)[:, None]
        return (slice(y0, y1), slice(x0, x1)), cx, cy

    def take(self, at, index, cover, depth, shade, margin):
        depth = np.broadcast_to(depth, cover.shape)
        best, ids = self.depth[at], self.ids[at]
        wins = cover & ((depth < best) | ((depth == best) & ((index < ids) | (ids < 0))))
        self.second[at] = np.where(wins, best, np.where(cover, np.minimum(self.second[at], depth), self.second[at]))
        self.depth[at] = np.where(wins, depth, best)
        self.ids[at] = np.where(wins, index, ids)
        self.shade[at] = np.where(wins, shade, self.shade[at])
        self.cover_margin[at] = np.minimum(self.cover_margin[at], margin)

    def finish(self, color, ambient, background):
        t = self.dtype
        col = np.asarray(DEFAULT_COLOR if color is None else color, np.float32).astype(t)
        amb = t(np.float32(ambient))
        shade = amb + (t(1) - amb) * self.shade
        v = (t(255) * col)[None, None, :] * shade[:, :, None]
        rgb = np.floor(np.minimum(np.maximum(v, t(0)), t(255)) + t(0.5)).astype(np.uint8)
        bg = np.floor(np.clip(t(255) * np.asarray(background, np.float32).astype(t), t(0), t(255)) + t(0.5)).astype(np.uint8)
        rgb[self.ids < 0] = bg
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isfinite(self.second), self.second.astype(np.float64) - self.depth.astype(np.float64), INF)
        return dict(ids=self.ids.astype(np.int32), depth=self.depth, rgb=rgb, cover_margin=self.cover_margin, depth_gap=gap)


def _light(light, dtype):
    return (DEFAULT_LIGHT if light is None else np.asarray(light, np.float64)).astype(np.float32).astype(dtype)


def render_points(points, view, height, width, radius, color=None, light=None, ambient=0.3, background=(1.0, 1.0, 1.0), dtype=np.float64):
    t = dtype
    out = _Buffers(height, width, t)
    q = project(view, points, t)
    l = _light(light, t)
    r = t(np.float32(radius))
    r2 = r * r
    for k in range(q.shape[0]):
        if not np.isfinite(q[k]).all():
            continue
        box = out.box(q[k, 0] - r, q[k, 0] + r, q[k, 1] - r, q[k, 1] + r)
        if box is None:
            continue
        at, cx, cy = box
        dx, dy = cx - q[k, 0], cy - q[k, 1]
        d2 = dx * dx + dy * dy
        cover = d2 <= r2
        nz = -np.sqrt(np.maximum(r2 - d2, t(0)))
        shade = np.maximum(((dx * l[0] + dy * l[1]) + nz * l[2]) / r, t(0))
        out.take(at, k, cover, q[k, 2], shade, np.abs(np.sqrt(d2.astype(np.float64)) - float(r)))
    return out.finish(color, ambient, background)


def _edge(P, Q, R, cx, cy, t):
    """-> (inside, distance to the edge line), or None for w = 0"""
    if Q[0] < P[0] or (Q[0] == P[0] and Q[1] < P[1]):
        P, Q = Q, P
    dx, dy = Q[0] - P[0], Q[1] - P[1]
    w = dx * (R[1] - P[1]) - dy * (R[0] - P[0])
    if w == 0:
        return None
    s = t(1) if w > 0 else t(-1)
    nx, ny = s * -dy, s * dx
    tie = bool(nx > 0 or (nx == 0 and ny > 0))
    e = dx * (cy - P[1]) - dy * (cx - P[0])
    inside = (s * e > 0) | ((e == 0) & tie)
    return inside, np.abs(e.astype(np.float64)) / np.hypot(float(dx), float(dy))


def render_mesh(vertices, faces, view, height, width, color=None, light=None, ambient=0.3, background=(1.0, 1.0, 1.0), dtype=np.float64):
    t = dtype
    out = _Buffers(height, width, t)
    q = project(view, vertices, t)
    l = _light(light, t)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    for k, (i0, i1, i2) in enumerate(faces.tolist()):
        if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= q.shape[0]:
            continue
        a, b, c = q[i0], q[i1], q[i2]
        if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()):
            continue
        u, v = b - a, c - a
        nx, ny, nz = u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]
        if nz == 0 or nz != nz:
            continue
        box = out.box(min(a[0], b[0], c[0]), max(a[0], b[0], c[0]), min(a[1], b[1], c[1]), max(a[1], b[1], c[1]))
        if box is None:
            continue
        at, cx, cy = box
        edges = [_edge(a, b, c, cx, cy, t), _edge(b, c, a, cx, cy, t), _edge(c, a, b, cx, cy, t)]
        if any(e is None for e in edges):
            continue
        inside = np.stack([np.broadcast_to(e[0], (cy.shape[0], cx.shape[1])) for e in edges])
        dist = np.stack([np.broadcast_to(e[1], (cy.shape[0], cx.shape[1])) for e in edges])
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            depth = a[2] - (nx * (cx - a[0]) + ny * (cy - a[1])) / nz
            length = np.sqrt((nx * nx + ny * ny) + nz * nz)
            shade = np.abs((nx * l[0] + ny * l[1]) + nz * l[2]) / length
        cover = inside.all(axis=0)
        margin = np.where(cover, dist.min(axis=0), np.where(inside, -INF, dist).max(axis=0))
        out.take(at, k, cover & np.isfinite(depth), depth, shade, margin)
    return out.finish(color, ambient, background)


def comparable(result, margin=1e-3):
    """pixels whose winner cannot flip under perturbations below `margin` pixels, and the share of the covered pixels that are left out"""
    keep = (result["cover_margin"] >= margin) & (result["depth_gap"] >= margin)
    covered = result["ids"] >= 0
    share = float((covered & ~keep).sum()) / max(int(covered.sum()), 1)
    return keep, share


# ------------------------------------------------------------------ inputs of the tests
def front_view(scale, height, width):
    """x right, y down, z away, `scale` pixels per unit, the origin at the image centre: exact in fp32 for lattice coordinates"""
    return np.asarray([[scale, 0, 0, width / 2.0], [0, scale, 0, height / 2.0], [0, 0, scale, 0]], np.float32)


def lattice_mesh():
    """Multiples of 1/16 under front_view(8, 48, 64): projected coordinates are multiples of 1/2 below 64, every product fits 24 bits.
    Faces: 0 a right triangle with its legs through pixel centres, 1 - 2 a quad as two triangles (diagonal through pixel centres), 3 zero area,
    4 an index out of range, 5 a NaN vertex, 6 - 7 two coplanar overlapping triangles at constant depth, 8 a triangle partly outside."""
    v = np.asarray([
        (-3.4375, -2.4375, 1.0), (-1.4375, -2.4375, 1.0), (-3.4375, -0.4375, 1.0),                     # 0: centres at k + 1/2 px = (k + 1/2) / 8
        (-0.9375, -2.4375, 2.0), (1.0625, -2.4375, 2.0), (1.0625, -0.4375, 3.0), (-0.9375, -0.4375, 3.0),   # 1, 2
        (1.5, -2.0, 1.0), (2.0, -1.5, 1.0), (2.5, -1.0, 1.0),                                          # 3: collinear
        (np.nan, 0.0, 0.0),                                                                            # 5
        (-3.5, 0.5, 2.0), (-0.5, 0.5, 2.0), (-3.5, 2.5, 2.0), (-2.5, 0.0625, 2.0), (0.5, 1.0, 2.0), (-2.5, 2.9375, 2.0),   # 6, 7
        (2.5, 1.5, 0.5), (5.5, 2.0, 1.5), (3.0, 4.5, 1.0),                                             # 8: past the right and bottom borders
    ], np.float32)
    f = np.asarray([(0, 1, 2), (3, 4, 5), (3, 5, 6), (7, 8, 9), (0, 1, 20), (0, 10, 2), (11, 12, 13), (14, 15, 16), (17, 18, 19)], np.int32)
    return v, f


def lattice_points():
    """Under front_view(8, 48, 64): centres on pixel centres, on pixel corners and half way, overlapping at different depths, one partly outside
    the image, one wholly outside, one NaN."""
    return np.asarray([(-2.4375, -1.4375, 1.0), (-2.0, -1.5, 0.5), (0.0625, 0.0625, 2.0), (0.3125, 0.0625, 2.0), (0.1875, 0.25, 1.0),
                       (3.9375, 2.9375, 1.0), (-4.0, -3.0, 1.0), (9.0, 0.0, 1.0), (np.nan, 0.0, 1.0), (0.0625, 0.0625, 2.0)], np.float32)


def fan(azim, elev, count=8, seed=3):
    """`count` triangles round a shared vertex, the rim closed, facing the eye of orbit_view(azim, elev): the rim runs once round the hub in the
    image plane (angles sorted, each gap below pi) with some relief in depth, so the projected triangles tile a star-shaped polygon without overlap.
    -> (vertices, faces)"""
    g = np.random.default_rng(seed)
    a, e = np.deg2rad(azim), np.deg2rad(elev)
    right = np.asarray([-np.sin(a), np.cos(a), 0.0])
    up = np.asarray([-np.cos(a) * np.sin(e), -np.sin(a) * np.sin(e), np.cos(e)])
    toward = np.asarray([np.cos(a) * np.cos(e), np.sin(a) * np.cos(e), np.sin(e)])
    ang = (np.arange(count) + g.uniform(0.1, 0.9, count)) * (2.0 * np.pi / count)
    rad = g.uniform(0.5, 0.85, count)
    rim = (rad * np.cos(ang))[:, None] * right + (rad * np.sin(ang))[:, None] * up + g.uniform(-0.3, 0.3, count)[:, None] * toward
    hub = 0.05 * right - 0.03 * up + 0.1 * toward
    v = np.concatenate([hub[None], rim]).astype(np.float32)
    f = np.asarray([(0, 1 + i, 1 + (i + 1) % count) for i in range(count)], np.int32)
    return v, f


def random_triangles(count, seed, extent=None):
    """`count` separate triangles in [-1, 1]^3; with `extent`, small ones: a centre in [-0.8, 0.8]^3 and corners within `extent` of it"""
    g = np.random.default_rng(seed)
    if extent is None:
        v = g.uniform(-1.0, 1.0, (count, 3, 3))
    else:
        v = g.uniform(-0.8, 0.8, (count, 1, 3)) + g.uniform(-extent, extent, (count, 3, 3))
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * count, dtype=np.int32).reshape(-1, 3)


def random_points(count, seed):
    return np.random.default_rng(seed).uniform(-0.9, 0.9, (count, 3)).astype(np.float32)


def general_cases():
    """The general-position inputs of tests/test_gpu_render.py, seeds fixed: name -> (kind, data, height, width, radius)"""
    return {
        "tri40": ("mesh", random_triangles(40, 11), 48, 64, None),
        "tri300": ("mesh", random_triangles(300, 12, 0.12), 136, 160, None),
        "pts300": ("points", random_points(300, 13), 48, 64, 2.5),
        "pts2048": ("points", random_points(2048, 14), 136, 160, 1.5),
    }


def ragged_batch():
    """B = 3 shapes of different sizes, the middle one empty, at 48 x 64: (meshes as (vertices, faces), clouds, radius)"""
    meshes = [random_triangles(25, 21), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), random_triangles(60, 22, 0.25)]
    clouds = [random_points(150, 23), np.zeros((0, 3), np.float32), random_points(40, 24)]
    return meshes, clouds, 2.5


VIEW_ANGLES = ((35.0, 20.0), (-60.0, 30.0), (120.0, -15.0))           # (azim, elev) of the V = 3 shared views; shape b adds 25 b to every azimuth


def decode_png(data):
    """bytes of an 8-bit RGB PNG whose rows all use filter 0 (what save_png writes) -> uint8 (H, W, 3); zlib and struct only"""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, size = 8, b"", None
    while at < len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b"IHDR":
            w, h, bits, colour, comp, flt, lace = struct.unpack(">IIBBBBB", body)
            assert (bits, colour, comp, flt, lace) == (8, 2, 0, 0, 0)
            size = (h, w)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    assert kind == b"IEND" and size is not None
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(size[0], 1 + 3 * size[1])
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(size[0], size[1], 3).copy()


def render_case(case, view, dtype=np.float64, **style):
    kind, data, height, width, radius = case
    if kind == "mesh":
        return render_mesh(data[0], data[1], view, height, width, dtype=dtype, **style)
    return render_points(data, view, height, width, radius, dtype=dtype, **style)
