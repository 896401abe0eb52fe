"""The numpy statement of the device-resident mesh dataset (csrc/mesh_data.hip, include/pcd_hip.h: pcd_mesh_area_sums,
pcd_mesh_batch_clouds): the header's counter layout, counters -> u, the running area sums in the device's tree, the triangle choice, the
point, and the chain with the header's summation order -- everything in fp32 operation by operation (numpy rounds every float32
operation once, and nothing here is contracted), with a float64 form beside it.

What numpy cannot reproduce bit for bit is the device's logf / sincosf: `cloud_fp32` therefore takes the jitter normals (and the
rotation's sine and cosine) as fp32 arrays -- the GPU test reads the normals off `pcd_randn`, which the header names as their
definition -- and `cloud_f64` uses numpy's own in float64, for the tests that compare within a tolerance.

Shared by tests/test_mesh_data_cpu.py and tests/test_gpu_mesh_data.py; nothing here imports the package."""
import numpy as np

import device_data_statement as V

CTR_POINT, CTR_ANGLE, CTR_JITTER, CTR_SPAN, MAX_POINTS = 0, 1 << 24, 1 << 25, 1 << 26, 1 << 24
NORMALIZE, ROTATE, JITTER = V.NORMALIZE, V.ROTATE, V.JITTER
LANES, WAVE = 1024, 64
F = np.float32


def span_ranges(num_points: int, slot: int, offset: int = 0) -> dict:
    """The half-open counter ranges slot `slot` may touch, by purpose."""
    base = offset + slot * CTR_SPAN
    return {"point": (base + CTR_POINT, base + CTR_POINT + num_points), "angle": (base + CTR_ANGLE, base + CTR_ANGLE + 1),
            "jitter": (base + CTR_JITTER, base + CTR_JITTER + num_points), "span": (base, base + CTR_SPAN)}


# ---------------------------------------------------------------------------------------------- counters -> u
def uniforms(n: int, seed: int, ctr0: int) -> np.ndarray:
    """(n, 3) float32: u_k of point i = (word k of counter ctr0 + CTR_POINT + i >> 8) / 2^24, exact in fp32."""
    w = V.philox4x32(np.arange(n, dtype=np.uint64) + np.uint64(ctr0 + CTR_POINT), seed)
    return (w[:, :3] >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)


def angle_u(seed: int, ctr0: int) -> float:
    return ((int(V.philox4x32(ctr0 + CTR_ANGLE, seed)[0, 0]) >> 8) + 0.5) / 16777216.0


def normals_f64(n: int, seed: int, ctr0: int) -> np.ndarray:
    """(n, 3) float64 jitter normals: Box-Muller values 0, 1, 2 of counter ctr0 + CTR_JITTER + i."""
    return V.normals(n, seed, ctr0 + CTR_JITTER - V.CTR_JITTER)


# ---------------------------------------------------------------------------------------------- areas and their running sums
def _corners(vertices, faces, dtype):
    t = np.asarray(vertices, dtype).reshape(-1, 3)[np.asarray(faces, np.int64).reshape(-1, 3)]
    return t[:, 0], t[:, 1], t[:, 2]


def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def areas_fp32(vertices, faces) -> np.ndarray:
    """0.5 * sqrt((nx nx + ny ny) + nz nz), n = (b - a) x (c - a); a non-finite area counts as 0."""
    a, b, c = _corners(vertices, faces, F)
    n = _cross(b - a, c - a)
    with np.errstate(all="ignore"):
        area = F(0.5) * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    assert area.dtype == F
    return np.where(np.isfinite(area) & (area <= F(3.0e38)), area, F(0))


def _scan_up(x):
    """Inclusive scan along the last axis by the shuffle-up ladder o = 1, 2, 4, ...: x[l] += x[l - o] for l >= o."""
    x = x.copy()
    o = 1
    while o < x.shape[-1]:
        y = x.copy()
        y[..., o:] = x[..., o:] + x[..., :-o]
        x, o = y, o * 2
    return x


def running_sums_fp32(vertices, faces) -> np.ndarray:
    """The device's inclusive running sums of one mesh: chunks of 1024 faces; inside a chunk a scan over the 64 lanes of each wave,
    a scan over the 16 wave sums, sum = base + (sums of the waves before + the lane's); base += the chunk's total."""
    area = areas_fp32(vertices, faces)
    nf = len(area)
    out = np.zeros(nf, F)
    base = F(0)
    for c0 in range(0, nf, LANES):
        x = np.zeros(LANES, F)
        x[:min(LANES, nf - c0)] = area[c0:c0 + LANES]
        x = _scan_up(x.reshape(LANES // WAVE, WAVE))
        wsum = _scan_up(x[:, WAVE - 1])
        before = np.concatenate([[F(0)], wsum[:-1]]).astype(F)
        incl = base + (before[:, None] + x)
        assert incl.dtype == F
        out[c0:c0 + LANES] = incl.reshape(-1)[:nf - c0]
        base = F(base + wsum[-1])
    return out


# ---------------------------------------------------------------------------------------------- triangle choice, point, normal
def choose(sums: np.ndarray, u0: np.ndarray) -> np.ndarray:
    """The first triangle whose running sum exceeds u0 * total (the last one at most); sums fp32 non-decreasing, total = sums[-1] > 0."""
    target = np.asarray(u0, F) * F(sums[-1])
    assert target.dtype == F
    return np.minimum(np.searchsorted(sums, target, side="right"), len(sums) - 1).astype(np.int64)


def points_fp32(vertices, faces, index, u) -> np.ndarray:
    """((1 - s) a + (s (1 - u2)) b) + (s u2) c per coordinate, s = sqrt(u1)."""
    a, b, c = _corners(vertices, np.asarray(faces).reshape(-1, 3)[index], F)
    u = np.asarray(u, F)
    s, t = np.sqrt(np.clip(u[:, 1], F(0), F(1)))[:, None], np.clip(u[:, 2], F(0), F(1))[:, None]
    wa, wb, wc = F(1) - s, s * (F(1) - t), s * t
    p = (wa * a + wb * b) + wc * c
    assert p.dtype == F
    return p


def face_normals_fp32(vertices, faces, index) -> np.ndarray:
    a, b, c = _corners(vertices, np.asarray(faces).reshape(-1, 3)[index], F)
    m = _cross(b - a, c - a)
    length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])[:, None]
    ok = (length > 0) & (length <= F(3.0e38))
    with np.errstate(all="ignore"):
        return np.where(ok, m / np.where(ok, length, F(1)), F(0)).astype(F)


def draw_fp32(vertices, faces, n: int, seed: int, ctr0: int):
    """(points (n, 3) fp32, face index (n,), unit normals (n, 3) fp32) of one slot before the chain."""
    sums = running_sums_fp32(vertices, faces)
    u = uniforms(n, seed, ctr0)
    index = choose(sums, u[:, 0])
    return points_fp32(vertices, faces, index, u), index, face_normals_fp32(vertices, faces, index)


# ---------------------------------------------------------------------------------------------- the chain
def column_sum_fp32(x: np.ndarray) -> np.float32:
    """The header's order: lane t adds x[t], x[t + 1024], ... in ascending order to a partial that starts at 0 (padding with +0 adds
    nothing: a partial is never -0); in each wave the butterfly x[l] + x[l ^ o], o = 32 .. 1; the 16 wave sums in ascending order."""
    x = np.asarray(x, F)
    rows = -(-len(x) // LANES)
    padded = np.zeros(rows * LANES, F)
    padded[:len(x)] = x
    acc = np.zeros(LANES, F)
    for row in padded.reshape(rows, LANES):
        acc = acc + row
    w = acc.reshape(LANES // WAVE, WAVE)
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    total = w[0, 0]
    for k in range(1, LANES // WAVE):
        total = total + w[k, 0]
    assert w.dtype == F
    return F(total)


def normalize_fp32(p: np.ndarray):
    """(p - mean) / radius: mean = column sums / float(n), radius = sqrt(max((d0 d0 + d1 d1) + d2 d2)).  -> (cloud, mean, radius)"""
    p = np.asarray(p, F)
    mean = np.array([column_sum_fp32(p[:, c]) for c in range(3)], F) / F(len(p))
    d = p - mean
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    radius = np.sqrt(d2.max())
    assert d.dtype == F and radius.dtype == F
    return d / radius, mean, radius


def rotate_fp32(p, sn, cs):
    p = np.asarray(p, F).copy()
    p0, p2 = p[:, 0].copy(), p[:, 2].copy()
    p[:, 0] = p0 * F(cs) - p2 * F(sn)
    p[:, 2] = p0 * F(sn) + p2 * F(cs)
    return p


def cloud_fp32(vertices, faces, n: int, seed: int, offset: int, slot: int, flags: int, sigma: float = 0.01, clip: float = 0.05,
               jitter_normals=None, sincos=None) -> np.ndarray:
    """The output rows of one slot in fp32, bit for bit.  JITTER needs `jitter_normals` (n, 3) fp32 and ROTATE `sincos` = (sin, cos) fp32,
    the device's values (see the module docstring)."""
    p, _, _ = draw_fp32(vertices, faces, n, seed, offset + slot * CTR_SPAN)
    if flags & ROTATE:
        p = rotate_fp32(normalize_fp32(p)[0], *sincos)
    if flags & JITTER:
        p = p + np.clip(F(sigma) * np.asarray(jitter_normals, F), -F(clip), F(clip))
    if flags & NORMALIZE:
        p = normalize_fp32(p)[0]
    assert p.dtype == F
    return p


def _normalize64(p):
    p = p - p.mean(axis=0)
    return p / np.sqrt((p ** 2).sum(axis=1)).max()


def cloud_f64(vertices, faces, n: int, seed: int, offset: int, slot: int, flags: int, sigma: float = 0.01, clip: float = 0.05):
    """The same rows in float64 (the triangle of each point is the fp32 statement's: the choice is a comparison of fp32 sums), with
    numpy's sine, cosine and normals.  -> (cloud (n, 3), unit normals (n, 3) rotated with the points, face index)"""
    ctr0 = offset + slot * CTR_SPAN
    u = uniforms(n, seed, ctr0).astype(np.float64)
    index = choose(running_sums_fp32(vertices, faces), u[:, 0].astype(F))
    a, b, c = _corners(vertices, np.asarray(faces).reshape(-1, 3)[index], np.float64)
    s, t = np.sqrt(u[:, 1])[:, None], u[:, 2][:, None]
    p = (1.0 - s) * a + s * (1.0 - t) * b + s * t * c
    m = np.cross(b - a, c - a)
    nrm = m / np.linalg.norm(m, axis=1, keepdims=True)
    if flags & ROTATE:
        ang = 2 * np.pi * angle_u(seed, ctr0)
        rot = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        p, nrm = _normalize64(p) @ rot, nrm @ rot
    if flags & JITTER:
        p = p + np.clip(float(F(sigma)) * normals_f64(n, seed, ctr0), -float(F(clip)), float(F(clip)))
    if flags & NORMALIZE:
        p = _normalize64(p)
    return p, nrm, index


# ---------------------------------------------------------------------------------------------- shared test meshes
CUBE_FACES = np.asarray([(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (2, 3, 7), (2, 7, 6), (1, 2, 6), (1, 6, 5),
                         (0, 4, 7), (0, 7, 3)], np.int32)


def box(lo, hi):
    """Closed box with 8 vertices and 12 outward triangles; float32 vertices."""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (3,)), np.broadcast_to(np.asarray(hi, np.float64), (3,))
    v = np.asarray([(lo[0], lo[1], lo[2]), (hi[0], lo[1], lo[2]), (hi[0], hi[1], lo[2]), (lo[0], hi[1], lo[2]),
                    (lo[0], lo[1], hi[2]), (hi[0], lo[1], hi[2]), (hi[0], hi[1], hi[2]), (lo[0], hi[1], hi[2])], np.float32)
    return v, CUBE_FACES.copy()


def random_triangles(count: int, seed: int):
    """`count` separate random triangles in [-1, 1]^3, float32."""
    g = np.random.default_rng(seed)
    first = g.uniform(-0.8, 0.8, (count, 1, 3))
    v = (first + g.uniform(-0.2, 0.2, (count, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * count, dtype=np.int32).reshape(-1, 3)


def ellipsoid(seed: int, rings: int = 6, segments: int = 8):
    """A closed latitude / longitude ellipsoid with random semi-axes and centre: 2 + (rings - 1) * segments vertices."""
    g = np.random.default_rng(seed)
    radii, centre = g.uniform(0.3, 1.0, 3), g.uniform(-0.2, 0.2, 3)
    v = [(0.0, 0.0, 1.0)]
    for r in range(1, rings):
        th = np.pi * r / rings
        v += [(np.sin(th) * np.cos(2 * np.pi * s / segments), np.sin(th) * np.sin(2 * np.pi * s / segments), np.cos(th)) for s in range(segments)]
    v.append((0.0, 0.0, -1.0))
    f = []
    ring = lambda r, s: 1 + (r - 1) * segments + s % segments        # noqa: E731
    for s in range(segments):
        f.append((0, ring(1, s), ring(1, s + 1)))
        f.append((len(v) - 1, ring(rings - 1, s + 1), ring(rings - 1, s)))
        for r in range(1, rings - 1):
            f.append((ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)))
            f.append((ring(r, s), ring(r + 1, s + 1), ring(r, s + 1)))
    return (np.asarray(v) * radii + centre).astype(np.float32), np.asarray(f, np.int32)


def three_triangles_1_2_5():
    """Three right triangles in the plane z = 0 with areas 1, 2 and 5."""
    v = np.asarray([(0, 0, 0), (2, 0, 0), (0, 1, 0), (3, 0, 0), (5, 0, 0), (3, 2, 0), (6, 0, 0), (11, 0, 0), (6, 2, 0)], np.float32)
    return v, np.arange(9, dtype=np.int32).reshape(3, 3)


def write_obj(path, mesh):
    v, f = mesh
    with open(path, "w") as out:
        for x, y, z in np.asarray(v, np.float64):
            out.write(f"v {x:.9g} {y:.9g} {z:.9g}\n")
        for a, b, c in np.asarray(f, np.int64) + 1:
            out.write(f"f {a} {b} {c}\n")
