"""Local geometry of generated clouds on the device (csrc/cloud_geometry.hip; DESIGN.md "Cloud geometry"): the k nearest neighbours of
every point, PCA normals, and statistical / radius outlier removal; and closed triangle meshes from clouds by grid closing
(csrc/cloud_mesh.hip; DESIGN.md "Cloud to mesh"): `cloud_to_meshes` and its stages.

Clouds are packed as `metrics._pack_clouds` packs them: a (P, N, 3) device tensor with optional (P,) counts, or a list of ragged
(n_i, 3) device clouds.  PyTorch allocates; every value comes from a kernel, nothing is read back and nothing synchronises with the
host, so every function here can be captured in a graph (`cloud_to_meshes` reads the mesh sizes back once, as it says).  A CPU tensor raises the usual RuntimeError; bad arguments raise ValueError
before the library is loaded.
"""
from __future__ import annotations

import math
import os

import torch

from . import _lib
from .metrics import _pack_clouds
from .utils import Mesh, save_mesh, save_point_cloud


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


# ------------------------------------------------------------------ cloud -> closed mesh (csrc/cloud_mesh.hip; DESIGN.md "Cloud to mesh")
MESH_R_MIN, MESH_R_MAX = 8, 64


def _check_grid(resolution, bounds, inset):
    """-> (R, lo, hi, h): the validated grid of a cloud-to-mesh call, h = (hi - lo) / (R - 1) in double."""
    if isinstance(resolution, bool) or not isinstance(resolution, int) or not MESH_R_MIN <= resolution <= MESH_R_MAX:
        raise ValueError(f"resolution must be an integer in {MESH_R_MIN} .. {MESH_R_MAX} (one 64-bit word per grid row), got {resolution!r}")
    try:
        lo, hi = (float(b) for b in bounds)
    except (TypeError, ValueError):
        raise ValueError(f"bounds must be a pair (lo, hi) of numbers, got {bounds!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"bounds must be finite with lo < hi, got {bounds!r}")
    if isinstance(inset, bool) or not isinstance(inset, (int, float)) or not -1.0 <= float(inset) <= 1.0:
        raise ValueError(f"inset must be a number of pitches in [-1, 1], got {inset!r}")
    return resolution, lo, hi, (hi - lo) / (resolution - 1)


def _check_radius(radius, radius_scale, lo, hi):
    if radius is None:
        if isinstance(radius_scale, bool) or not isinstance(radius_scale, (int, float)) or not (math.isfinite(radius_scale) and radius_scale > 0):
            raise ValueError(f"radius_scale must be a finite number > 0, got {radius_scale!r}")
    elif isinstance(radius, torch.Tensor):
        if radius.dim() != 1:
            raise ValueError("a radius tensor must be shaped (P,), one radius per cloud")
    elif isinstance(radius, bool) or not isinstance(radius, (int, float)) or not (math.isfinite(radius) and 0 < radius <= (hi - lo) / 2):
        raise ValueError(f"radius must be None, a (P,) tensor or a number in (0, (hi - lo) / 2 = {(hi - lo) / 2}] -- the shell costs "
                         f"N (r / h)^3 --, got {radius!r}")


def _radii(points, cnt, radius, radius_scale, inset, h):
    """The radius every cloud is closed with, (P,) float32: max(r_p, (2 - inset) h), r_p given or radius_scale * the cloud's spacing."""
    P, N = points.shape[0], points.shape[1]
    lib = _lib.load()
    out = torch.empty(P, dtype=torch.float32, device=points.device)
    if radius is None:
        d2, _ = _knn(points, cnt, points, cnt, 8, True)
        _lib.check(lib.pcd_cloud_spacing(d2.data_ptr(), cnt.data_ptr(), N, P, 8, None, float(radius_scale), h, float(inset), out.data_ptr(),
                                         _lib.stream_ptr()), "cloud_spacing")
        return out
    if isinstance(radius, torch.Tensor):
        if radius.device.type != "cuda":
            raise RuntimeError("geometry runs only on an MI355X device: move the radii to 'cuda' (no CPU path)")
        if radius.shape[0] != P:
            raise ValueError("a radius tensor must hold one radius per cloud")
        given = radius.to(device=points.device, dtype=torch.float32).contiguous()
    else:
        given = torch.full((P,), float(radius), dtype=torch.float32, device=points.device)
    _lib.check(lib.pcd_cloud_spacing(None, None, 0, P, 0, given.data_ptr(), 1.0, h, float(inset), out.data_ptr(), _lib.stream_ptr()),
               "cloud_spacing")
    return out


def _words(t, what):
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[1] != t.shape[2] or t.dtype != torch.int64:
        raise ValueError(f"{what} must be a (P, R, R) int64 tensor of row words, bit x of word [z][y] = node (z, y, x)")
    if not MESH_R_MIN <= t.shape[1] <= MESH_R_MAX:
        raise ValueError(f"{what}: the resolution must lie in {MESH_R_MIN} .. {MESH_R_MAX}, got {t.shape[1]}")
    if t.device.type != "cuda":
        raise RuntimeError("geometry runs only on an MI355X device: move the grid words to 'cuda' (no CPU path)")
    return t.contiguous()


def cloud_radius(clouds, resolution=64, radius=None, radius_scale=1.5, inset=0.0, bounds=(-1.25, 1.25), counts=None):
    """The ball radius `cloud_to_meshes` closes every cloud with, (P,) float32 on the device.  `radius=None`: radius_scale * s_p, s_p the mean
    distance from a point to its 8th nearest neighbour over the points that have 8; a number or a (P,) tensor: that.  In every case at least
    (2 - inset) pitches h = (hi - lo) / (resolution - 1), which is also what a cloud of fewer than 9 points gets."""
    R, lo, hi, h = _check_grid(resolution, bounds, inset)
    _check_radius(radius, radius_scale, lo, hi)
    points, cnt = _pack_clouds(clouds, counts, "clouds")
    return _radii(points, cnt, radius, radius_scale, inset, h)


def _shell_fill(points, cnt, R, lo, h, radii):
    P, N = points.shape[0], points.shape[1]
    dev = points.device
    shell = torch.empty(P, R, R, dtype=torch.int64, device=dev)
    outside = torch.empty(P, R, R, dtype=torch.int64, device=dev)
    info = torch.empty(P, 3, dtype=torch.int32, device=dev)
    sweeps = torch.empty(P, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().pcd_cloud_shell_fill(points.data_ptr(), cnt.data_ptr(), N, P, R, lo, h, radii.data_ptr(), shell.data_ptr(),
                                                outside.data_ptr(), info.data_ptr(), sweeps.data_ptr(), _lib.stream_ptr()), "cloud_shell_fill")
    return shell, outside, info, sweeps


def cloud_shell_grid(clouds, resolution=64, radius=None, radius_scale=1.5, inset=0.0, bounds=(-1.25, 1.25), counts=None):
    """Stages 1 - 3 of `cloud_to_meshes`: -> (shell (P, R, R) int64, outside (P, R, R) int64, info (P, 3) int32, radius (P,) float32).  A word
    [z][y] holds the nodes of one grid row, bit x = node x (read the int64 as unsigned).  Shell: the nodes within the radius of a finite point
    of the cloud; outside: the free nodes that the grid's surroundings reach through free nodes, 6-connected; info = (shell nodes, enclosed
    nodes, shell nodes on the six faces of the grid)."""
    R, lo, hi, h = _check_grid(resolution, bounds, inset)
    _check_radius(radius, radius_scale, lo, hi)
    points, cnt = _pack_clouds(clouds, counts, "clouds")
    radii = _radii(points, cnt, radius, radius_scale, inset, h)
    shell, outside, info, _ = _shell_fill(points, cnt, R, lo, h, radii)
    return shell, outside, info, radii


def grid_outside(shell, return_sweeps=False):
    """The fill alone: shell words (P, R, R) int64 -> (outside (P, R, R) int64, info (P, 3) int32 [, sweeps (P,) int32]); `sweeps` counts the
    passes over the grid until one changed nothing (-1 would say the cap of R^3 was passed)."""
    words = _words(shell, "shell")
    P, R = words.shape[0], words.shape[1]
    outside = torch.empty_like(words)
    info = torch.empty(P, 3, dtype=torch.int32, device=words.device)
    sweeps = torch.empty(P, dtype=torch.int32, device=words.device)
    _lib.check(_lib.load().pcd_grid_fill_outside(words.data_ptr(), P, R, outside.data_ptr(), info.data_ptr(), sweeps.data_ptr(),
                                                 _lib.stream_ptr()), "grid_fill_outside")
    return (outside, info, sweeps) if return_sweeps else (outside, info)


def _depth_field(outside, R, h, radii, inset, want_d2):
    P = outside.shape[0]
    v = torch.empty(P, R, R, R, dtype=torch.float32, device=outside.device)
    d2 = torch.empty(P, R, R, R, dtype=torch.int32, device=outside.device) if want_d2 else None
    _lib.check(_lib.load().pcd_grid_depth_field(outside.data_ptr(), P, R, h, radii.data_ptr(), float(inset), _lib.ptr(d2), v.data_ptr(),
                                                _lib.stream_ptr()), "grid_depth_field")
    return v, d2


def grid_depth_field(outside, radius, inset=0.0, bounds=(-1.25, 1.25), return_d2=False):
    """Stages 4 and 5: outside words (P, R, R) int64 and the radii (P,) float32 as `cloud_radius` returns them (used as they are, no clamp) ->
    v (P, R, R, R) float32 [, D2 (P, R, R, R) int32].  D2 is the exact squared distance in pitches to the nearest outside node, the layer round
    the grid included; v = 0 on outside nodes and 1 + ((sqrt(D2) h - r) - inset h) elsewhere, so the closed solid is v > 1."""
    if not isinstance(radius, torch.Tensor) or not isinstance(outside, torch.Tensor) or radius.shape != outside.shape[:1]:
        raise ValueError("radius must be a (P,) tensor, one radius per grid")
    words = _words(outside, "outside")
    R, lo, hi, h = _check_grid(int(words.shape[1]), bounds, inset)
    if radius.device.type != "cuda":
        raise RuntimeError("geometry runs only on an MI355X device: move the radii to 'cuda' (no CPU path)")
    v, d2 = _depth_field(words, R, h, radius.to(torch.float32).contiguous(), inset, return_d2)
    return (v, d2) if return_d2 else v


def _project(verts, vcnt, points, cnt, index, k, scale, offset, out):
    P, V = verts.shape[0], verts.shape[1]
    _lib.check(_lib.load().pcd_project_to_cloud(verts.data_ptr(), vcnt.data_ptr(), V, _lib.ptr(points), _lib.ptr(cnt),
                                                0 if points is None else points.shape[1], P, _lib.ptr(index), k, scale, offset,
                                                out.data_ptr(), _lib.stream_ptr()), "project_to_cloud")
    return out


def project_to_cloud(vertices, clouds, k=8, vertex_counts=None, counts=None, index=None):
    """Stage 7: move every vertex onto the plane fitted to its k nearest points of its own cloud: c their mean, n the unit eigenvector of the
    least eigenvalue of their covariance, v' = v - ((v - c) . n) n, in double on the device, rounded to fp32 once.  `vertices` (P, V, 3) with
    optional `vertex_counts`, packed like the clouds; -> (P, V, 3) float32, rows past a count zero.  A vertex with fewer than 3 neighbours stays
    where it is.  `index` (P, V, k) int32: neighbour lists to use instead of searching."""
    k = _check_k(k)
    verts, vcnt = _pack_clouds(vertices, vertex_counts, "vertices")
    points, cnt = _pack_clouds(clouds, counts, "clouds")
    if verts.shape[0] != points.shape[0]:
        raise ValueError("vertices and clouds must hold the same number of clouds")
    if index is None:
        _, index = _knn(verts, vcnt, points, cnt, k, False)
    elif not isinstance(index, torch.Tensor) or index.shape != (verts.shape[0], verts.shape[1], k) or index.dtype != torch.int32:
        raise ValueError("index must be a (P, V, k) int32 tensor")
    elif index.device.type != "cuda":
        raise RuntimeError("geometry runs only on an MI355X device: move the index lists to 'cuda' (no CPU path)")
    return _project(verts, vcnt, points, cnt, index.contiguous(), k, 1.0, 0.0, torch.zeros_like(verts))


def cloud_to_meshes(clouds, resolution=64, radius=None, radius_scale=1.5, inset=0.0, bounds=(-1.25, 1.25), counts=None, project=True, k=8,
                    return_info=False):
    """One closed triangle mesh per cloud, by morphological closing on a grid (DESIGN.md "Cloud to mesh"): -> list of `utils.Mesh`, views of one
    padded (P, Vmax, 3) vertex tensor and one packed face tensor; with `return_info` also a dict of device tensors `radius` (P,) float32 and
    `shell`, `enclosed`, `border` (P,) int32.

    The grid has `resolution` nodes per axis over `bounds` = (lo, hi), pitch h = (hi - lo) / (resolution - 1).  (1) The radius r of a cloud is
    `radius` (a number, or a (P,) tensor) or, for None, `radius_scale` times the cloud's spacing, the mean distance to the 8th nearest neighbour;
    in every case at least (2 - inset) h.  (2) Shell: the nodes within r of a point.  (3) Outside: the free nodes reached from the grid's
    surroundings through free nodes; the free nodes left are enclosed.  (4, 5) The solid (shell + enclosed) is eroded by r + inset h through the
    exact distance to the outside: what remains is the closing of the point set by a ball of radius r with its cavities filled.  (6) Surface
    nets (`utils.voxel_tensor_to_meshes`' kernels) on that field, mapped to `bounds`.  (7) `project`: every vertex moves onto the plane fitted
    to its `k` nearest points of the cloud (`project_to_cloud`); the faces do not change, so the mesh stays closed and consistently oriented as
    a complex, but self-intersection after the projection is not excluded.  No oriented normals are needed anywhere.  All integer and bit work,
    or fp32 without contraction: bitwise repeatable, a cloud's mesh independent of the rest of the batch.  One host read (the mesh sizes), as in
    `voxel_tensor_to_meshes`, and no other synchronisation.

    Limits.  Gaps narrower than 2 r are bridged.  A part thinner than about (1 + inset) pitches, and any open sheet at inset >= 0, vanishes;
    inset = -1 keeps it as a slab of two pitches that the projection flattens.  `bounds` must hold the cloud plus r + 2 h, or the solid is cut
    at the border: `border` > 0 reports shell nodes on the faces of the grid.  A shell that does not seal (`enclosed` == 0 on a shape that has
    an inside) gives an empty or fragmentary mesh: raise `radius_scale`.  Clouds of fewer than 9 points get the least radius; empty clouds and
    clouds whose solid erodes away give empty meshes, no error."""
    R, lo, hi, h = _check_grid(resolution, bounds, inset)
    _check_radius(radius, radius_scale, lo, hi)
    k = _check_k(k)
    points, cnt = _pack_clouds(clouds, counts, "clouds")
    P, dev = points.shape[0], points.device
    lib = _lib.load()
    radii = _radii(points, cnt, radius, radius_scale, inset, h)
    _, outside, info, sweeps = _shell_fill(points, cnt, R, lo, h, radii)
    v, _ = _depth_field(outside, R, h, radii, inset, False)
    ws = torch.empty(max(lib.pcd_mesh_workspace_bytes(P, R, R, R), 4) // 4, dtype=torch.int32, device=dev)
    sizes = torch.empty(P, 2, dtype=torch.int32, device=dev)
    _lib.check(lib.pcd_mesh_count(v.data_ptr(), P, R, R, R, 1.0, ws.data_ptr(), sizes.data_ptr(), _lib.stream_ptr()), "mesh_count")
    host = torch.cat([sizes.reshape(-1), sweeps]).cpu().tolist()          # the one host read: the outputs are sized on the host
    nv, nf, done = host[0:2 * P:2], host[1:2 * P:2], host[2 * P:]
    if min(done) < 0:
        raise RuntimeError("cloud_to_meshes: the outside fill passed its cap of resolution^3 sweeps")
    vmax = max(nv)
    verts = torch.zeros(P, max(vmax, 1), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(sum(nf), 3, dtype=torch.int32, device=dev)
    if vmax > 0:
        offsets = torch.stack([torch.arange(P, dtype=torch.int64, device=dev) * vmax,
                               torch.cumsum(sizes[:, 1], dim=0, dtype=torch.int64) - sizes[:, 1]], dim=1).contiguous()
        _lib.check(lib.pcd_mesh_emit(v.data_ptr(), P, R, R, R, 1.0, ws.data_ptr(), offsets.data_ptr(), verts.data_ptr(), faces.data_ptr(),
                                     _lib.stream_ptr()), "mesh_emit")
        vcnt = sizes[:, 0].contiguous()
        _project(verts, vcnt, None, None, None, 0, (hi - lo) / 2, (lo + hi) / 2, verts)      # the nets' [-1, 1] -> bounds
        if project:
            _, index = _knn(verts, vcnt, points, cnt, k, False)
            _project(verts, vcnt, points, cnt, index, k, 1.0, 0.0, verts)
    meshes = [Mesh(verts[p, :nv[p]], f) for p, f in enumerate(torch.split(faces, nf))]
    if return_info:
        return meshes, {"radius": radii, "shell": info[:, 0], "enclosed": info[:, 1], "border": info[:, 2]}
    return meshes


def save_cloud_meshes(mesh_dir: str, clouds, counts=None, resolution: int = 64, radius_scale: float = 1.5, fmt: str = "obj", log=None):
    """`cloud_to_meshes` on a batch and one `sample_{i}.{fmt}` per cloud in `mesh_dir`; per shape the vertices, faces and enclosed nodes go to
    `log` (a logging.Logger), with a warning where the shell touches the border of the grid or the mesh is empty.  -> the meshes."""
    if fmt not in ("obj", "ply"):
        raise ValueError(f"fmt must be 'obj' or 'ply', got {fmt!r}")
    meshes, info = cloud_to_meshes(clouds, resolution=resolution, radius_scale=radius_scale, counts=counts, return_info=True)
    enclosed, border = info["enclosed"].tolist(), info["border"].tolist()
    for i, mesh in enumerate(meshes):
        save_mesh(os.path.join(mesh_dir, f"sample_{i}.{fmt}"), mesh)
        if log is not None:
            log.info(f"mesh {i}: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces, {enclosed[i]} enclosed nodes")
            if border[i] > 0:
                log.warning(f"mesh {i}: {border[i]} shell nodes on the border of the grid: the solid is cut there (widen the bounds)")
            if mesh.faces.shape[0] == 0:
                log.warning(f"mesh {i} is empty: the shell did not seal or the solid eroded away (raise --mesh-radius-scale)")
    return meshes
