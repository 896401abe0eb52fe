"""Inputs shared by tests/test_geometry_statement_cpu.py and tests/test_gpu_geometry.py: seeded clouds, their packing, and the statements
of tests/geometry_statement.py, computed once per case and shared by the tests that need them.

Launch shape of `pcd_knn` as built (csrc/cloud_geometry.hip): grid (ceil(nq_max / 256), P), one query per thread, so a cloud's queries end
one below, at and one above a query block at 255 / 256 / 257 (and 511 / 512 / 513, 1023 / 1024 / 1025).  Every block walks ALL targets of
its cloud in LDS tiles of 512 -- there is no target split -- so 511 / 512 / 513 and 1023 / 1024 / 1025 also end one below, at and one above
a tile, and 1300 = 512 + 512 + 276.  Inside a tile the targets go in steps of 4 (the last step padded with points at infinity), so the tiny
clouds 1 .. 5 cover the step; a thread parks its candidates in a queue of 8, and the wave inserts them all once some lane holds more than 4,
so clouds of 6 and more points (5 candidates a point) run the insertion inside the loop and smaller ones only at its end.
Three template instances, K = 8 / 16 / 32, the smallest >= k: k = 1, 8, 9, 16, 17, 32 sit at and on both sides of every boundary.
`pcd_cloud_normals` runs grid (ceil(n_max / 256), P) with one point per thread; `pcd_cloud_outlier_mask` and `pcd_cloud_compact` run one
workgroup of 256 threads per cloud, the compaction in blocks of 256 rows (255 / 256 / 257 again)."""
import functools
import math

import torch

import geometry_statement as G

KS = (1, 8, 9, 16, 17, 32)
K_MAX = 32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def uniform(n, seed):
    return torch.rand(n, 3, generator=_gen(seed)) * 2 - 1


def doubled(n, seed):
    """Every point occurs twice, at two shuffled indices: each point has a neighbour at distance 0 that is not itself."""
    g = _gen(seed)
    x = torch.rand(n, 3, generator=g) * 2 - 1
    x = torch.cat([x, x])
    return x[torch.randperm(2 * n, generator=g)]


def lattice(n, seed):
    """Sites of the integer lattice [-4, 4]^3 scaled by 1/4, drawn with replacement: every d2 is a small multiple of 1/16 and exact in fp32, so
    many candidates are exactly equally far (a site has 6 neighbours at 1/4, 12 at sqrt(2)/4) and some sites are drawn twice."""
    return torch.randint(-4, 5, (n, 3), generator=_gen(seed)).float() / 4


def non_finite(n, seed):
    """A uniform cloud with one NaN coordinate (row 3) and one infinite coordinate (row 10)."""
    x = uniform(n, seed)
    x[3, 1] = float("nan")
    x[10, 0] = float("inf")
    return x


#   name: clouds as (kind, n); every cloud searches itself (exclude_self) -- the call of k_nearest_neighbors(targets=None)
SELF_CASES = {
    # nq_max 1300: 6 query blocks a cloud, the sizes at the edges of the query block and of the LDS tile
    "edges": [("uniform", n) for n in (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1300)],
    # 0, 1, 2, 3 points and k, k + 1 points for each instance boundary: fewer candidates than slots
    "tiny": [("uniform", n) for n in (0, 1, 2, 3, 4, 5, 8, 9, 10, 16, 17, 18, 32, 33, 34)],
    # 512 clouds of 2 .. 8 points in one call: one query block each, grid (1, 512)
    "many_tiny": [("uniform", 2 + (i * 5) % 7) for i in range(512)],
    "doubled": [("doubled", 300), ("doubled", 129)],
    "lattice": [("lattice", 400), ("lattice", 700)],
    "non_finite": [("non_finite", 40), ("uniform", 40), ("non_finite", 300)],
}
#   queries against other targets (no exclusion): (n, m)
PAIR_CASES = {
    "pairs": [(257, 513), (513, 257), (1, 40), (40, 1), (0, 9), (9, 0), (300, 300)],
}
_KINDS = {"uniform": uniform, "doubled": doubled, "lattice": lattice, "non_finite": non_finite}


@functools.lru_cache(maxsize=None)
def self_case(name):
    """-> list of (n_i, 3) fp32 clouds"""
    return [_KINDS[kind](n, 7000 + 17 * i).float().contiguous() for i, (kind, n) in enumerate(SELF_CASES[name])]


@functools.lru_cache(maxsize=None)
def pair_case(name):
    q = [uniform(n, 8000 + 19 * i) for i, (n, m) in enumerate(PAIR_CASES[name])]
    t = [uniform(m, 8001 + 19 * i) for i, (n, m) in enumerate(PAIR_CASES[name])]
    return q, t


@functools.lru_cache(maxsize=None)
def self_statements(name, dtype=torch.float32):
    """[(d2 (n, 32), index (n, 32))] of every cloud of the case against itself, at k = 32: slot s of a smaller k is slot s of this."""
    return [G.knn(x, x, K_MAX, True, dtype) for x in self_case(name)]


@functools.lru_cache(maxsize=None)
def pair_statements(name):
    q, t = pair_case(name)
    return [G.knn(a, b, K_MAX, False) for a, b in zip(q, t)]


def pack(clouds, fill=7.0, rows=None):
    """Ragged (n_i, 3) clouds -> padded (P, max n, 3) fp32 and int32 counts.  The padding rows of a cloud are copies of its own live points,
    cycled: a kernel that reads a padding row as a target finds a neighbour at distance 0 there.  An empty cloud is padded with `fill`."""
    nmax = max(1, max(c.shape[0] for c in clouds)) if rows is None else rows
    buf = torch.full((len(clouds), nmax, 3), fill)
    for i, c in enumerate(clouds):
        n = c.shape[0]
        buf[i, :n] = c
        if 0 < n < nmax:
            buf[i, n:] = c[torch.arange(nmax - n) % n]
    return buf, torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32)


def pack_rows(rows, width, fill, dtype):
    """Ragged per-cloud (n_i, width) tables -> padded (P, max n, width), `fill` in the padding."""
    nmax = max(1, max(r.shape[0] for r in rows))
    buf = torch.full((len(rows), nmax, width), fill, dtype=dtype)
    for i, r in enumerate(rows):
        buf[i, :r.shape[0]] = r
    return buf


# ------------------------------------------------------------------ surfaces with known normals
SPHERE_RADIUS = 0.8
TORUS = (0.6, 0.25)


def sphere(n, seed, radius=SPHERE_RADIUS):
    """-> points (n, 3) fp32 on the sphere of `radius` about the origin, and the analytic unit normals in fp64 OF THE FP32 POINTS."""
    v = torch.randn(n, 3, generator=_gen(seed), dtype=torch.float64)
    x = (radius * v / v.norm(dim=1, keepdim=True)).float()
    return x, x.double() / x.double().norm(dim=1, keepdim=True)


def torus(n, seed, big=TORUS[0], small=TORUS[1]):
    """-> points on the torus about the z axis (tube centre radius `big`, tube radius `small`), uniform in the two angles, and the analytic
    unit normals in fp64 at the angles drawn."""
    g = _gen(seed)
    u = torch.rand(n, generator=g, dtype=torch.float64) * 2 * math.pi
    v = torch.rand(n, generator=g, dtype=torch.float64) * 2 * math.pi
    ring = big + small * torch.cos(v)
    x = torch.stack([ring * torch.cos(u), ring * torch.sin(u), small * torch.sin(v)], dim=1)
    nrm = torch.stack([torch.cos(v) * torch.cos(u), torch.cos(v) * torch.sin(u), torch.sin(v)], dim=1)
    return x.float(), nrm


def sphere_with_outliers(n=1024, outliers=24, seed=31):
    """The sphere and `outliers` far points at radius 1.5 .. 2, at random rows of one cloud.  -> points (n + outliers, 3), is_outlier (bool)."""
    g = _gen(seed)
    x, _ = sphere(n, seed + 1)
    v = torch.randn(outliers, 3, generator=g, dtype=torch.float64)
    far = (v / v.norm(dim=1, keepdim=True) * (1.5 + 0.5 * torch.rand(outliers, 1, generator=g, dtype=torch.float64))).float()
    rows = torch.randperm(n + outliers, generator=g)
    flag = torch.zeros(n + outliers, dtype=torch.bool)
    flag[rows[:outliers]] = True
    out = torch.empty(n + outliers, 3)
    out[flag] = far
    out[~flag] = x
    return out, flag


SURFACE_SIZES = (257, 1024, 1300)
SURFACE_KS = (8, 16, 32)
#   name: (surface, n) -- one batch per k holds all six clouds
SURFACES = [(kind, n) for kind in ("sphere", "torus") for n in SURFACE_SIZES]
# 32 of 257 points cover most of the torus tube's circumference, and the share of points whose two smallest eigenvalues nearly meet (gap <
# 0.1) then runs from 0.8 to 5 % over the seeds (0 to 3.5 % at k = 8).  The direction comparison may leave out 3 %: this seed stays at 1.6 %.
SURFACE_SEEDS = {("torus", 257): 9073}


@functools.lru_cache(maxsize=None)
def surfaces():
    """[(points, analytic normals)] in the order of SURFACES"""
    return [(sphere if kind == "sphere" else torus)(n, SURFACE_SEEDS.get((kind, n), 9000 + 23 * i)) for i, (kind, n) in enumerate(SURFACES)]


@functools.lru_cache(maxsize=None)
def surface_statements(k):
    """Per surface: dict(d2, index: the fp32 stage (a) at k with exclude_self; normals: `G.normals` of those lists)."""
    out = []
    for x, _ in surfaces():
        d2, index = G.knn(x, x, k, True)
        out.append(dict(d2=d2, index=index, normals=G.normals(x, index)))
    return out


GAP_MIN = 0.1           # points whose (l1 - l0) / l2 is below this are left out of the direction comparison ...
GAP_SHARE = 0.03        # ... and at most this share of a case's points may be


# ------------------------------------------------------------------ outlier masks
OUTLIER_RATIOS = (2.0, 1.0)
BAND = 1e-9             # the masks are compared outside |dbar - limit| <= BAND * limit; the cases keep that band empty
RADII = ((0.1, 4), (0.25, 16), (0.05, 1))      # (radius, min_neighbors) of the radius rule, on the k = 16 tables


@functools.lru_cache(maxsize=None)
def outlier_batches():
    """name -> (k, clouds, [d2 (n_i, k)]): the fp32 stage-(a) tables the mask kernel is fed with.  `small` holds an empty cloud, a single point
    (no valid slot: dropped, outside the statistics) and clouds with fewer than k neighbours; `non_finite` rows without a valid slot inside
    larger clouds; `doubled` many distances of exactly 0."""
    out = {}
    for k in SURFACE_KS:
        out[f"surfaces_k{k}"] = (k, [x for x, _ in surfaces()], [s["d2"] for s in surface_statements(k)])
    x, _ = sphere_with_outliers()
    out["sphere_outliers"] = (16, [x], [G.knn(x, x, 16, True)[0]])
    small = [uniform(n, 9500 + n) for n in (0, 1, 3, 5, 9, 17, 33, 40)]
    out["small"] = (16, small, [G.knn(c, c, 16, True)[0] for c in small])
    for name in ("non_finite", "doubled"):
        out[name] = (16, self_case(name), [d2[:, :16].contiguous() for d2, _ in self_statements(name)])
    return out
