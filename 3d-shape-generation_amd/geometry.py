"""Local geometry of generated clouds on the device (csrc/cloud_geometry.hip; DESIGN.md "Cloud geometry"): the k nearest neighbours of
every point, PCA normals, and statistical / radius outlier removal.

Clouds are packed as `metrics._pack_clouds` packs them: a (P, N, 3) device tensor with optional (P,) counts, or a list of ragged
(n_i, 3) device clouds.  PyTorch allocates; every value comes from a kernel, nothing is read back and nothing synchronises with the
host, so every function here can be captured in a graph.  A CPU tensor raises the usual RuntimeError; bad arguments raise ValueError
before the library is loaded.
"""
from __future__ import annotations

import math
import os

import torch

from . import _lib
from .metrics import _pack_clouds
from .utils import save_point_cloud


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.PCD_KNN_MAX_K:
        raise ValueError(f"k must be an integer in 1 .. {_lib.PCD_KNN_MAX_K}, got {k!r}")
    return k


def _knn(q, nq, t, nt, k, exclude_self):
    P, N, M = q.shape[0], q.shape[1], t.shape[1]
    d2 = torch.empty(P, N, k, dtype=torch.float32, device=q.device)
    index = torch.empty(P, N, k, dtype=torch.int32, device=q.device)
    _lib.check(_lib.load().pcd_knn(q.data_ptr(), nq.data_ptr(), N, t.data_ptr(), nt.data_ptr(), M, P, k, int(exclude_self), d2.data_ptr(),
                                   index.data_ptr(), _lib.stream_ptr()), "knn")
    return d2, index


def k_nearest_neighbors(queries, targets=None, k=16, query_counts=None, target_counts=None):
    """For every query point its k nearest targets, nearest first: -> (d2 (P, N, k) float32, index (P, N, k) int32) with d2 = (dx dx + dy dy)
    + dz dz in fp32 from direct differences (the arithmetic of `metrics.nearest_neighbors`) and equal distances in the order of the index.
    `targets=None`: the neighbours of every point inside its own cloud, the point itself (its own row, not a duplicate of it elsewhere)
    left out.  A query with fewer than k candidates has (NaN, -1) in the trailing slots; a query with a non-finite coordinate and every
    row past a count have them in every slot; a non-finite target is nobody's neighbour.  Slot s does not depend on k.  One enqueue for
    all clouds, bitwise repeatable, a cloud's result independent of the rest of the batch."""
    k = _check_k(k)
    if targets is None and target_counts is not None:
        raise ValueError("target_counts go with targets; within a cloud the query counts apply")
    q, nq = _pack_clouds(queries, query_counts, "queries")
    if targets is None:
        return _knn(q, nq, q, nq, k, True)
    t, nt = _pack_clouds(targets, target_counts, "targets")
    if q.shape[0] != t.shape[0]:
        raise ValueError("queries and targets must hold the same number of clouds")
    return _knn(q, nq, t, nt, k, False)


def _normals(points, counts, index, k, mode, view, return_curvature):
    P, N = points.shape[0], points.shape[1]
    lib = _lib.load()
    normals = torch.empty(P, N, 3, dtype=torch.float32, device=points.device)
    curvature = torch.empty(P, N, dtype=torch.float32, device=points.device) if return_curvature else None
    ws, need = None, 0
    if mode == _lib.PCD_NORMALS_OUTWARD:
        need = int(lib.pcd_cloud_normals_workspace_bytes(P))
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=points.device)
    _lib.check(lib.pcd_cloud_normals(points.data_ptr(), counts.data_ptr(), N, P, index.data_ptr(), k, mode, _lib.ptr(view), normals.data_ptr(),
                                     _lib.ptr(curvature), _lib.ptr(ws), need, _lib.stream_ptr()), "cloud_normals")
    return normals, curvature


def estimate_normals(clouds, k=16, counts=None, orient=None, return_curvature=False):
    """Unit normals (P, N, 3) float32 by principal component analysis of every point's neighbourhood, the point and its k nearest
    neighbours: the eigenvector of the smallest eigenvalue of the neighbourhood's covariance, computed in double on the device.  `orient`:
    None (the sign is unspecified but repeatable), "outward" (away from the centroid of the cloud: n . (p - c) >= 0, right for a star-shaped
    surface) or a (P, 3) tensor of viewpoints (n . (v - p) >= 0).  With `return_curvature` also (P, N) float32 l0 / (l0 + l1 + l2), the
    surface variation, in [0, 1/3].  A point with fewer than two neighbours and every row past a count get a zero normal and a NaN
    curvature."""
    k = _check_k(k)
    view, mode = None, _lib.PCD_NORMALS_UNORIENTED
    if isinstance(orient, str):
        if orient != "outward":
            raise ValueError(f"orient must be None, 'outward' or a (P, 3) tensor of viewpoints, got {orient!r}")
        mode = _lib.PCD_NORMALS_OUTWARD
    elif orient is not None:
        if not isinstance(orient, torch.Tensor) or orient.dim() != 2 or orient.shape[1] != 3:
            raise ValueError("orient must be None, 'outward' or a (P, 3) tensor of viewpoints")
        mode = _lib.PCD_NORMALS_TOWARD_VIEW
    points, cnt = _pack_clouds(clouds, counts, "clouds")
    if mode == _lib.PCD_NORMALS_TOWARD_VIEW:
        if orient.shape[0] != points.shape[0]:
            raise ValueError("orient must hold one viewpoint per cloud")
        if orient.device.type != "cuda":
            raise RuntimeError("geometry runs only on an MI355X device: move the viewpoints to 'cuda' (no CPU path)")
        view = orient.to(torch.float32).contiguous()
    _, index = _knn(points, cnt, points, cnt, k, True)
    normals, curvature = _normals(points, cnt, index, k, mode, view, return_curvature)
    return (normals, curvature) if return_curvature else normals


def remove_outliers(clouds, k=16, std_ratio=2.0, radius=None, min_neighbors=None, counts=None, normals=None, return_mask=False):
    """Drop the stray points of every cloud: -> (clouds (P, N, 3) float32, counts (P,) int32 [, normals (P, N, 3)] [, mask (P, N) uint8]).  The
    kept points stand in their original order at the front of each padded cloud, zeros behind them; `counts` says how many there are and
    stays on the device (no host synchronisation: pass it on as `counts=` / slice after your own `.cpu()`).  Statistical (the default): with
    dbar_i the mean distance of point i to its k nearest neighbours, a point is kept iff dbar_i <= mean + std_ratio * std over its cloud.
    Radius (`radius` given): a point is kept iff at least `min_neighbors` (default k) of its k nearest neighbours lie within `radius`.
    `normals` (packed as the clouds) are compacted alongside; `mask` is the keep mask in the original order."""
    k = _check_k(k)
    if radius is None:
        if min_neighbors is not None:
            raise ValueError("min_neighbors goes with radius")
        if not math.isfinite(float(std_ratio)):
            raise ValueError(f"std_ratio must be finite, got {std_ratio!r}")
        method, rad, need = _lib.PCD_OUTLIER_STATISTICAL, 0.0, 1
    else:
        if not (math.isfinite(float(radius)) and float(radius) >= 0.0):
            raise ValueError(f"radius must be finite and >= 0, got {radius!r}")
        need = k if min_neighbors is None else min_neighbors
        if isinstance(need, bool) or not isinstance(need, int) or not 1 <= need <= k:
            raise ValueError(f"min_neighbors must be an integer in 1 .. k = {k}, got {min_neighbors!r}")
        method, rad = _lib.PCD_OUTLIER_RADIUS, float(radius)
    points, cnt = _pack_clouds(clouds, counts, "clouds")
    attr = None
    if normals is not None:
        attr, _ = _pack_clouds(normals, None, "normals")
        if attr.shape != points.shape:
            raise ValueError("normals must be shaped like their clouds")
    P, N = points.shape[0], points.shape[1]
    lib = _lib.load()
    d2, _ = _knn(points, cnt, points, cnt, k, True)
    mask = torch.empty(P, N, dtype=torch.uint8, device=points.device)
    _lib.check(lib.pcd_cloud_outlier_mask(d2.data_ptr(), cnt.data_ptr(), N, P, k, method, float(std_ratio), rad, need, mask.data_ptr(), None,
                                          _lib.stream_ptr()), "cloud_outlier_mask")
    out = torch.empty_like(points)
    attr_out = torch.empty_like(attr) if attr is not None else None
    kept = torch.empty(P, dtype=torch.int32, device=points.device)
    _lib.check(lib.pcd_cloud_compact(points.data_ptr(), _lib.ptr(attr), mask.data_ptr(), cnt.data_ptr(), N, P, out.data_ptr(),
                                     _lib.ptr(attr_out), kept.data_ptr(), _lib.stream_ptr()), "cloud_compact")
    result = (out, kept)
    if attr is not None:
        result += (attr_out,)
    if return_mask:
        result += (mask,)
    return result


def save_cloud_plys(ply_dir: str, clouds, counts=None, k: int = 16) -> None:
    """Write `sample_{i}.ply` for every cloud of a (P, N, 3) device batch (or ragged list) into `ply_dir`, with outward normals estimated
    from `k` neighbours (`estimate_normals(orient="outward")`); `counts` (P,) says how many rows of each padded cloud to write.  One
    transfer to the host for the whole batch."""
    points, cnt = _pack_clouds(clouds, counts, "clouds")
    normals = estimate_normals(points, k=k, counts=cnt, orient="outward")
    host_points, host_normals, sizes = points.cpu(), normals.cpu(), cnt.tolist()
    for i, n in enumerate(sizes):
        save_point_cloud(os.path.join(ply_dir, f"sample_{i}.ply"), host_points[i, :n], host_normals[i, :n])
