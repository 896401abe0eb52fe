"""Inputs shared by tests/test_gpu_surface_metrics.py: seeded clouds with unit normals, their packing, and the fp32 / fp64 statements of
every pair, computed once per case (tests/surface_statement.py) and shared by the tests that need them.

Launch shape of the nearest-neighbour kernel under `pcd_surface_metrics` (csrc/surface_metrics.hip): jobs = 2 P (both directions),
NQ = max(na_max, nb_max), query blocks = ceil(NQ / 1024) (256 threads x 4 queries), target splits = clamp(ceil(1024 / (query blocks x
jobs)), 1, ceil(NQ / 128)), targets per split = ceil(nr / splits), walked in LDS tiles of 512.  `pcd_nearest_neighbors` has jobs = P,
NQ = nq_max and the clamp from nt_max."""
import functools

import torch

import metrics_cases as K
import surface_statement as S

THRESHOLDS = (0.02, 0.04, 0.1)
_FILL = [("uniform", 2 + (i * 5) % 7, 2 + (i * 3) % 7) for i in range(256)]
_EDGES = [("matched", n, m) for n in (1023, 1024, 1025) for m in (511, 512, 513)]

#   name: pairs as (kind, n, m)
CASES = {
    # one query block of which one thread holds a live query, 1 split (max_split = 1)
    "single": [("uniform", 1, 1)],
    # NQ 1025: 2 query blocks, jobs 18, splits = min(ceil(1024 / 36) = 29, ceil(1025 / 128) = 9) = 9: 57 or 114 targets a split; the queries
    # 1023 / 1024 / 1025 end one below, at and one above the first query block
    "edges_split": _EDGES,
    # NQ 1300, P = 256: 2 query blocks, jobs 512, splits = ceil(1024 / 1024) = 1: every block walks all targets in tiles of 512, so 511 / 512 /
    # 513 end one below, at and one above the tile (and 1100 = 512 + 512 + 76, 1300 = 512 + 512 + 276); the rest of the batch is tiny pairs
    "edges_one_split": _EDGES + [("matched", 1300, 1100), ("matched", 1100, 1300), ("uniform", 257, 3), ("uniform", 5, 40), ("uniform", 0, 9)]
                       + _FILL[:256 - 14],
    # P = 1, NQ 1300: 2 query blocks, jobs 2, splits = min(256, 11) = 11: 100 targets a split for b, 119 for a (the last split 110).  Every
    # target of the smaller cloud is some query's nearest neighbour (the matched design), so neighbours sit on both sides of every boundary
    "one_pair_split": [("matched", 1300, 1100)],
    # NQ 1300, jobs 12, splits 43 -> 11.  (257, 3): one target a split and splits 3 .. 10 empty; (5, 40): 5 live queries, the other slots
    # clamped duplicates; (0, 9): an empty cloud
    "ragged": [("matched", 1025, 513), ("matched", 512, 1024), ("uniform", 257, 3), ("uniform", 5, 40), ("matched", 1300, 1300),
               ("uniform", 0, 9)],
    # NQ 8: one query block, jobs 1024, 1 split
    "many_tiny": [("uniform", 2 + (i * 5) % 7, 2 + (i * 3) % 7) for i in range(512)],
}


def unit_normals(n, seed):
    v = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed))
    return v / v.norm(dim=1, keepdim=True).clamp_min(1e-6)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> a, b, normals_a, normals_b: lists of (n_i, 3) fp32 tensors"""
    a, b, ka, kb = [], [], [], []
    for i, (kind, n, m) in enumerate(CASES[name]):
        x, y = K.make(kind, n, m, 5000 + 13 * i)
        a.append(x.float().contiguous())
        b.append(y.float().contiguous())
        ka.append(unit_normals(n, 6000 + 13 * i))
        kb.append(unit_normals(m, 6001 + 13 * i))
    return a, b, ka, kb


@functools.lru_cache(maxsize=None)
def statements(name, thresholds=THRESHOLDS):
    """[(fp32 statement, fp64 statement)] of every pair of the case (`surface_statement.row`)."""
    a, b, ka, kb = case(name)
    return [tuple(S.row(x, y, u, v, thresholds, dt) for dt in (torch.float32, torch.float64)) for x, y, u, v in zip(a, b, ka, kb)]


def pack(clouds, others=None, fill=7.0):
    """Ragged (n_i, 3) clouds -> padded (P, max n, 3) fp32 and int32 counts.  The padding rows of cloud i are copies of `others[i]`, the
    pair's other cloud, cycled: a kernel that reads a padding row as a target finds one of its own queries there, at distance 0.  Where
    the other cloud is empty (or for `others=None`: normals) the padding is `fill`."""
    nmax = max(1, max(c.shape[0] for c in clouds))
    buf = torch.full((len(clouds), nmax, 3), fill)
    for i, c in enumerate(clouds):
        n = c.shape[0]
        buf[i, :n] = c
        if others is not None and others[i].shape[0] > 0 and n < nmax:
            buf[i, n:] = others[i][torch.arange(nmax - n) % others[i].shape[0]]
    return buf, torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32)


def lattice_case(n=400, m=300, dup=60, seed=77):
    """Clouds on the dyadic lattice k / 16 in [-1, 1]^3, here its sites of spacing 1/4: every coordinate difference is a multiple of 1/4,
    every d2 a small multiple of 1/16 and exact in fp32, so equal minima really occur (a site has 6 neighbours at distance exactly 0.25)
    and many queries lie exactly on the threshold 0.25.  `dup` targets are duplicated, so the same d2 also occurs at two indices."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-4, 5, (n, 3), generator=g).float() * 4 / 16
    b = torch.randint(-4, 5, (m, 3), generator=g).float() * 4 / 16
    b = torch.cat([b, b[torch.randperm(m, generator=g)[:dup]]])
    b = b[torch.randperm(b.shape[0], generator=g)]
    return a, b, unit_normals(n, seed + 1), unit_normals(b.shape[0], seed + 2)
