"""The CPU statement of the cloud-geometry kernels (csrc/cloud_geometry.hip; include/pcd_hip.h "local geometry"), stage by stage in plain
torch / numpy.  `dtype` selects the precision where it matters: torch.float32 states what the kernels compute -- they are compiled
without contraction, so the stages that do not depend on an order equal it bit for bit -- and torch.float64 is the yardstick.

  (a) `knn(q, t, k, exclude_self)`: d2 = ((dx dx + dy dy) + dz dz) from direct differences, the candidates (a finite d2, and j != i under
      exclude_self) fully sorted by the key (bits of d2) << 32 | j in fp32 -- by (d2, j) in fp64 -- and the first k taken; (NaN, -1) in
      the slots past the number of candidates.
  (b) `normals(points, index)`: the neighbourhood of i is i and the entries 0 <= index < n of its row; with fewer than 3 members a zero
      normal and a NaN curvature, else `torch.linalg.eigh` in fp64 of the fp64 covariance of the fp32 coordinates about the
      neighbourhood's own mean: the eigenvector of the smallest eigenvalue, curvature l0 / (l0 + l1 + l2), gap = (l1 - l0) / l2.
      `centroid` and `oriented` state the two orientation rules.
  (c) `outlier_statistical(d2, ratio)` / `outlier_radius(d2, radius, min_neighbors)`: the keep masks from the fp32 stage-(a) distances.
  (d) `compact(points, mask, attr)`: the kept rows in order, zeros behind them."""
import numpy as np
import torch

from surface_statement import sq_dists, sqrt

NAN = float("nan")


def knn(q, t, k, exclude_self=False, dtype=torch.float32):
    """(n, 3), (m, 3) -> d2 (n, k) in `dtype`, index (n, k) int32; slot 0 the nearest, equal distances in the order of the index."""
    n, m = q.shape[0], t.shape[0]
    d2_out = torch.full((n, k), NAN, dtype=dtype)
    index_out = torch.full((n, k), -1, dtype=torch.int32)
    if n == 0 or m == 0:
        return d2_out, index_out
    d2 = sq_dists(q.to(dtype), t.to(dtype))
    valid = torch.isfinite(d2)
    j = torch.arange(m).expand(n, m)
    if exclude_self:
        valid = valid & (j != torch.arange(n)[:, None])
    if dtype == torch.float32:
        # a finite d2 >= 0 has a non-negative bit pattern, which orders as the value: the 64-bit key of the header, in a signed integer
        key = (d2.contiguous().view(torch.int32).to(torch.int64) << 32) | j
        key = torch.where(valid, key, torch.full_like(key, torch.iinfo(torch.int64).max))
        order = torch.sort(key, dim=1).indices
    else:
        cand = torch.where(valid, d2, torch.full_like(d2, float("inf")))
        order = torch.sort(cand, dim=1, stable=True).indices                 # stable: equal d2 stay in the order of j
    have = valid.sum(dim=1)
    take = min(k, m)
    order = order[:, :take]
    slot = torch.arange(take)[None, :] < have[:, None]
    d2_out[:, :take] = torch.where(slot, torch.gather(d2, 1, order), torch.full((n, take), NAN, dtype=dtype))
    index_out[:, :take] = torch.where(slot, order, torch.full_like(order, -1)).to(torch.int32)
    return d2_out, index_out


def normals(points, index):
    """(n, 3) fp32 points and (n, k) neighbour lists -> dict(normal (n, 3), curvature (n,), gap (n,), members (n,)) in fp64.  The sign of a
    normal is eigh's; compare directions up to sign."""
    n = points.shape[0]
    out = dict(normal=torch.zeros(n, 3, dtype=torch.float64), curvature=torch.full((n,), NAN, dtype=torch.float64),
               gap=torch.full((n,), NAN, dtype=torch.float64), members=torch.zeros(n, dtype=torch.int64))
    if n == 0:
        return out
    x = points.to(torch.float64)
    idx = torch.cat([torch.arange(n)[:, None], index.long()], dim=1)           # the point itself, then its row
    w = (idx >= 0) & (idx < n)
    nb = torch.where(w[:, :, None], x[idx.clamp(0, n - 1)], torch.zeros((), dtype=torch.float64))      # (n, k + 1, 3), zeros where no member
    wd = w.to(torch.float64)[:, :, None]
    m = w.sum(dim=1)
    out["members"] = m
    mean = (nb * wd).sum(dim=1) / m.clamp_min(1)[:, None]
    e = (nb - mean[:, None, :]) * wd
    cov = torch.einsum("nka,nkb->nab", e, e) / m.clamp_min(1)[:, None, None]
    ok = m >= 3
    finite = torch.isfinite(cov).all(dim=2).all(dim=1)
    use = ok & finite
    lam, vec = torch.linalg.eigh(torch.where(use[:, None, None], cov, torch.eye(3, dtype=torch.float64).expand(n, 3, 3)))
    trace = lam.sum(dim=1)
    out["normal"] = torch.where(use[:, None], vec[:, :, 0], torch.zeros(n, 3, dtype=torch.float64))
    out["curvature"] = torch.where(use & (trace > 0), lam[:, 0].clamp_min(0) / trace, torch.full_like(trace, NAN))
    out["gap"] = torch.where(use & (lam[:, 2] > 0), (lam[:, 1] - lam[:, 0]) / lam[:, 2], torch.full_like(trace, NAN))
    return out


def centroid(points):
    """The fp64 mean of the rows whose three coordinates are finite (zeros without one)."""
    x = points.to(torch.float64)
    ok = torch.isfinite(x).all(dim=1)
    return x[ok].mean(dim=0) if bool(ok.any()) else torch.zeros(3, dtype=torch.float64)


def oriented(normal, points, mode, view=None):
    """mode 1: n . (p - c) >= 0; mode 2: n . (v - p) >= 0.  -> the flipped normals and the dot product that decided, in fp64."""
    x = points.to(torch.float64)
    ray = x - centroid(points) if mode == 1 else view.to(torch.float64)[None, :] - x
    dot = (normal * ray).sum(dim=1)
    return torch.where((dot < 0)[:, None], -normal, normal), dot


def mean_distance(d2):
    """(n, k) fp32 stage-(a) distances -> dbar (n,) fp64: the mean over the valid slots (not NaN) of the correctly rounded fp32 roots, summed
    and divided in double; NaN without a valid slot."""
    valid = ~torch.isnan(d2)
    roots = torch.where(valid, sqrt(torch.where(valid, d2, torch.zeros_like(d2)), torch.float32).double(), torch.zeros(d2.shape, dtype=torch.float64))
    cnt = valid.sum(dim=1)
    return torch.where(cnt > 0, roots.sum(dim=1) / cnt.clamp_min(1), torch.full((d2.shape[0],), NAN, dtype=torch.float64))


def outlier_statistical(d2, ratio):
    """-> dict(mask (n,) uint8, dbar (n,) fp64, mu, sigma, limit): keep iff dbar <= mu + ratio sigma, mu and the population sigma over the
    points that have a dbar, all in double."""
    dbar = mean_distance(d2)
    have = ~torch.isnan(dbar)
    if not bool(have.any()):
        return dict(mask=torch.zeros(d2.shape[0], dtype=torch.uint8), dbar=dbar, mu=NAN, sigma=NAN, limit=NAN)
    v = dbar[have].numpy()
    mu = float(np.sum(v) / v.shape[0])
    sigma = float(np.sqrt(np.sum((v - mu) ** 2) / v.shape[0]))
    limit = mu + float(ratio) * sigma
    return dict(mask=(have & (dbar <= limit)).to(torch.uint8), dbar=dbar, mu=mu, sigma=sigma, limit=limit)


def outlier_radius(d2, radius, min_neighbors):
    """keep iff at least `min_neighbors` slots have d2 <= radius * radius, one fp32 product (a NaN slot never has)."""
    r2 = torch.tensor(radius, dtype=torch.float32) * torch.tensor(radius, dtype=torch.float32)
    return ((d2 <= r2).sum(dim=1) >= min_neighbors).to(torch.uint8)


def compact(points, mask, attr=None, rows=None):
    """-> (points_out (rows, 3), attr_out or None, count): the rows with mask != 0 in order, zeros behind them; `rows` = the padded size."""
    rows = points.shape[0] if rows is None else rows
    keep = mask.bool()
    count = int(keep.sum())
    out = torch.zeros(rows, 3, dtype=points.dtype)
    out[:count] = points[keep]
    attr_out = None
    if attr is not None:
        attr_out = torch.zeros(rows, 3, dtype=attr.dtype)
        attr_out[:count] = attr[keep]
    return out, attr_out, count
