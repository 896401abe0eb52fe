"""The CPU statement of the surface metrics (csrc/surface_metrics.hip; include/pcd_hip.h "surface evaluation"), stage by stage in plain
torch.  `dtype` selects the precision: torch.float32 states what the kernels compute -- they are compiled without contraction, so the
stages that do not depend on an order equal it bit for bit -- and torch.float64 is the yardstick.

  (a) `nearest(q, t)`: d2 = ((dx dx + dy dy) + dz dz) from direct differences, the minimum over the targets whose d2 is finite, and
      the LOWEST index that attains it, written out as a minimum over the indices that hit (no argmin, whose choice among ties is
      not specified).  A query without a finite distance gets (NaN, -1).
  (b) `row(...)`: the columns of one pair from the stage-(a) results of both directions.  The means are sums in double divided in
      double and rounded once; in the fp32 statement the terms (sqrt d2, |n . n'|) are fp32 values, in the fp64 one they are fp64
      values of the same fp32 stage-(a) results -- the two statements start from identical neighbours.  The derived columns
      (CHAMFER_L1, CHAMFER_L2, NC, HAUSDORFF, PRECISION / RECALL / FSCORE) are `derived(...)`, operations on the rounded halves.
  (c) `iou(a, b, threshold)`: integer counts, one division."""
import numpy as np
import torch

ROW = ("ACC", "COMP", "CHAMFER_L1", "ACC2", "COMP2", "CHAMFER_L2", "HAUSDORFF", "NC_A", "NC_B", "NC")
BASE = len(ROW)
ACC, COMP, CHAMFER_L1, ACC2, COMP2, CHAMFER_L2, HAUSDORFF, NC_A, NC_B, NC = range(BASE)
MEANS = (ACC, COMP, ACC2, COMP2, NC_A, NC_B)


def sq_dists(x, y):
    """|x_i - y_j|^2 as (n, m) by direct differences, ((dx*dx + dy*dy) + dz*dz)."""
    dx = x[:, None, 0] - y[None, :, 0]
    dy = x[:, None, 1] - y[None, :, 1]
    dz = x[:, None, 2] - y[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest(q, t, dtype=torch.float32):
    """(n, 3), (m, 3) -> d2 (n,) in `dtype`, index (n,) int32."""
    n, m = q.shape[0], t.shape[0]
    if n == 0 or m == 0:
        return torch.full((n,), float("nan"), dtype=dtype), torch.full((n,), -1, dtype=torch.int32)
    d2 = sq_dists(q.to(dtype), t.to(dtype))
    finite = torch.isfinite(d2)
    cand = torch.where(finite, d2, torch.full_like(d2, float("inf")))
    best = cand.min(dim=1).values
    hit = finite & (cand == best[:, None])
    j = torch.arange(m).expand(n, m)
    lowest = torch.where(hit, j, torch.full_like(j, m)).min(dim=1).values          # the lowest index among the hits
    none = ~finite.any(dim=1)
    return (torch.where(none, torch.full_like(best, float("nan")), best),
            torch.where(none, torch.full_like(lowest, -1), lowest).to(torch.int32))


def sqrt(x, dtype):
    """The correctly rounded square root of fp32 or fp64 values in `dtype`: the IEEE instruction on the fp64 value (numpy), rounded once more
    for fp32 -- innocuous for a square root, 53 >= 2 x 24 + 2.  torch's vectorised CPU sqrt is not correctly rounded on every machine (it was
    seen 1 ulp off), and the kernels' sqrtf is."""
    return torch.from_numpy(np.asarray(np.sqrt(x.double().numpy()))).to(dtype)


def _mean(terms, dtype):
    """Sum in double, one division in double, one rounding to `dtype`."""
    return (terms.double().sum() / terms.shape[0]).to(dtype)


def normal_terms(nq, nt, index, dtype):
    """|n_i . n'_index[i]| = |(x x' + y y') + z z'| per query, in `dtype`."""
    u, v = nq.to(dtype), nt.to(dtype)[index.long()]
    return ((u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]).abs()


def counts(d2_a, d2_b, thresholds):
    """[(number of a within tau, number of b within tau)]: d2 <= tau * tau, one fp32 product, on the fp32 stage-(a) values."""
    out = []
    for tau in thresholds:
        tau2 = torch.tensor(tau, dtype=torch.float32) * torch.tensor(tau, dtype=torch.float32)
        out.append((int((d2_a <= tau2).sum()), int((d2_b <= tau2).sum())))
    return out


def derived(row, far2, within, na, nb, dtype=torch.float32):
    """Fill the derived columns of `row` (the six means present) in `dtype`: far2 = the largest d2 of both directions, within = `counts`."""
    row = row.clone()
    row[CHAMFER_L1] = (row[ACC] + row[COMP]) / 2
    row[CHAMFER_L2] = row[ACC2] + row[COMP2]
    row[HAUSDORFF] = sqrt(far2, dtype)
    row[NC] = (row[NC_A] + row[NC_B]) / 2
    for k, (ca, cb) in enumerate(within):
        p = torch.tensor(ca, dtype=dtype) / torch.tensor(na, dtype=dtype)
        r = torch.tensor(cb, dtype=dtype) / torch.tensor(nb, dtype=dtype)
        row[BASE + 3 * k], row[BASE + 3 * k + 1] = p, r
        row[BASE + 3 * k + 2] = (2 * p * r) / (p + r) if float(p + r) > 0 else torch.zeros((), dtype=dtype)
    return row


def row(a, b, normals_a=None, normals_b=None, thresholds=(), dtype=torch.float32):
    """One pair -> dict(d2_a, index_a, d2_b, index_b: the fp32 stage (a) of both directions; within: the integer counts; row: the
    (BASE + 3 K,) columns in `dtype`).  An empty cloud, or a point without a finite distance, gives an all-NaN row."""
    a, b = a.to(torch.float32), b.to(torch.float32)
    d2_a, index_a = nearest(a, b)
    d2_b, index_b = nearest(b, a)
    out = dict(d2_a=d2_a, index_a=index_a, d2_b=d2_b, index_b=index_b, within=None)
    r = torch.full((BASE + 3 * len(thresholds),), float("nan"), dtype=dtype)
    out["row"] = r
    if a.shape[0] == 0 or b.shape[0] == 0 or bool((index_a < 0).any()) or bool((index_b < 0).any()):
        return out
    r[ACC], r[COMP] = _mean(sqrt(d2_a, dtype), dtype), _mean(sqrt(d2_b, dtype), dtype)
    r[ACC2], r[COMP2] = _mean(d2_a.to(dtype), dtype), _mean(d2_b.to(dtype), dtype)
    if normals_a is not None and normals_b is not None:
        r[NC_A] = _mean(normal_terms(normals_a, normals_b, index_a, dtype), dtype)
        r[NC_B] = _mean(normal_terms(normals_b, normals_a, index_b, dtype), dtype)
    out["within"] = counts(d2_a, d2_b, thresholds)
    out["row"] = derived(r, torch.maximum(d2_a.max(), d2_b.max()), out["within"], a.shape[0], b.shape[0], dtype)
    return out


def iou(a, b, threshold=0.5):
    """Two grids of any shape -> |A and B| / |A or B| as fp32 (NaN for an empty union), occupancy value > threshold."""
    oa, ob = a > threshold, b > threshold
    both, either = int((oa & ob).sum()), int((oa | ob).sum())
    if either == 0:
        return torch.tensor(float("nan"))
    return torch.tensor(both, dtype=torch.float32) / torch.tensor(either, dtype=torch.float32)
