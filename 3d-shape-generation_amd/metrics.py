"""Evaluation metrics with the reference's signatures (reference metrics.py), on HIP kernels.

`chamfer_distance`, `normalize_to_cube`, `compute_metrics` run on the device; the exact
Hungarian EMD stays a host-side scipy solve exactly as in the reference (metrics.py:49-92).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .utils import voxelize


def _prep(x: torch.Tensor) -> torch.Tensor:
    if x.device.type != "cuda":
        raise RuntimeError("metrics run only on an MI355X device: move the clouds to 'cuda' (no CPU path)")
    x = x.unsqueeze(0) if x.dim() == 2 else x
    return x.to(torch.float32).contiguous()


def normalize_to_cube(points: torch.Tensor) -> torch.Tensor:
    """metrics.py:7-21: centre on the bbox midpoint, scale by the max |coord| (per cloud)."""
    p = _prep(points)
    out = torch.empty_like(p)
    _lib.check(_lib.load().pcd_normalize_to_cube(p.data_ptr(), p.shape[0], p.shape[1], out.data_ptr(),
                                                 _lib.stream_ptr()), "normalize_to_cube")
    return out


def chamfer_distance(x, y, scaling_factor=1e+3):
    """metrics.py:23-47: mean_i min_j |x_i-y_j| + mean_j min_i |x_i-y_j| (unsquared L2), one scalar
    for the whole batch, times `scaling_factor`.  Distances are direct differences in fp32, which is
    closer to the exact value than the reference's matmul-form `torch.cdist`.
    Runs through the batched pair kernels (`pcd_pair_metrics`: queries x target splits x pairs blocks, so a single
    cloud pair still spreads over the chip); with equal sizes the batch-joint mean is the mean of the per-pair values."""
    return chamfer_per_sample(x, y, scaling_factor).mean()


def chamfer_per_sample(x, y, scaling_factor=1e+3) -> torch.Tensor:
    """Chamfer distance of each (x_b, y_b) pair, (B,) -- what test_point_ddpm.py:85-86 loops over."""
    x, y = _prep(x), _prep(y)
    if x.shape[0] != y.shape[0]:
        raise ValueError("batch sizes must match")
    return _pair_rows(x, y, False)[:, 0] * scaling_factor


def _pair_call(a, ca, b, cb, sinkhorn, epsilon, thresh, max_iter) -> torch.Tensor:
    """pcd_pair_metrics on packed (P, NA, 3) / (P, NB, 3) clouds with the host counts ca / cb: rows (P, 3) = (Chamfer x1,
    Sinkhorn EMD | 0, voxel BCE)."""
    P, dev = len(ca), a.device
    counts = torch.tensor([ca, cb], dtype=torch.int32)
    # log(mu + 1e-10) with the reference's fp32 torch ops (metrics.py:133-134,141), one value per pair and side
    logm = torch.log(torch.ones(2, P) / counts.to(torch.float32) + 1e-10)
    na, nb, log_mu, log_nu = torch.cat([counts, logm.view(torch.int32)]).to(dev)       # one copy to the device for the four rows
    lib = _lib.load()
    out = torch.empty(P, 3, dtype=torch.float32, device=dev)
    need = int(lib.pcd_pair_metrics_workspace_bytes(P, a.shape[1], b.shape[1]))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(lib.pcd_pair_metrics(a.data_ptr(), na.data_ptr(), a.shape[1], b.data_ptr(), nb.data_ptr(), b.shape[1], P,
                                    1 if sinkhorn else 0, float(epsilon), float(thresh), int(max_iter), log_mu.data_ptr(),
                                    log_nu.data_ptr(), out.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), "pair_metrics")
    return out


def _pair_rows(a: torch.Tensor, b: torch.Tensor, sinkhorn: bool, epsilon=1e-2, thresh=1e-5, max_iter=100) -> torch.Tensor:
    """_pair_call on dense (P, N, 3) / (P, M, 3) clouds."""
    P = a.shape[0]
    return _pair_call(a, [a.shape[1]] * P, b, [b.shape[1]] * P, sinkhorn, epsilon, thresh, max_iter)


def earth_mover_distance_cpu(x, y, scaling_factor=1):
    """metrics.py:49-92: exact assignment on the host (scipy Hungarian), bug-for-bug divisor
    (`x_pc.shape[1]` is the coordinate dimension 3, not the point count: SURVEY.md A.5)."""
    from scipy.optimize import linear_sum_assignment
    xn, yn = normalize_to_cube(x).cpu().numpy(), normalize_to_cube(y).cpu().numpy()
    if xn.shape[0] != yn.shape[0]:
        raise AssertionError("Batch sizes must be the same")
    vals = []
    for a, b in zip(xn, yn):
        dist = np.linalg.norm(a[:, None] - b[None, :], axis=-1)
        r, c = linear_sum_assignment(dist)
        vals.append(dist[r, c].sum() / max(a.shape[1], b.shape[1]))
    return torch.tensor(vals, device=x.device).mean() * scaling_factor


def earth_mover_distance_gpu(x, y, epsilon=1e-2, thresh=1e-5, max_iter=100, scaling_factor=1):
    """metrics.py:94-158: log-domain Sinkhorn on the device."""
    x, y = _prep(x), _prep(y)
    if x.shape[0] == 1 and y.shape[0] == 1:
        # one pair: batch-global C.max() and convergence test ARE per pair, so the device-resident loop applies
        return _pair_rows(x, y, True, epsilon, thresh, max_iter)[0, 1] * scaling_factor
    from .sinkhorn import sinkhorn_emd           # batch-joint cost normalisation and convergence test, as the reference
    return sinkhorn_emd(normalize_to_cube(x), normalize_to_cube(y), epsilon, thresh, max_iter) * scaling_factor


def voxel_bce(gen: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """BCE between two binary occupancy grids (metrics.py:181): every mismatching voxel costs
    100 (torch clamps log at -100), matching voxels cost 0, mean over all voxels."""
    if gen.shape != ref.shape:
        raise ValueError("grids must have the same shape")
    out = torch.empty(1, dtype=torch.float32, device=gen.device)
    _lib.check(_lib.load().pcd_binary_bce_mean(gen.data_ptr(), ref.data_ptr(), gen.numel(), out.data_ptr(),
                                               _lib.stream_ptr()), "binary_bce_mean")
    return out[0]


def pair_metrics(a_clouds, b_clouds, use_approximate_gpu_emd=False, epsilon=1e-2, thresh=1e-5, max_iter=100) -> torch.Tensor:
    """(P, 3) rows [Chamfer x1e3, EMD, voxel BCE] of the independent pairs (a_p, b_p): row p is what
    `compute_metrics(a_p, b_p, use_approximate_gpu_emd)` returns for that pair alone (the per-sample loop of
    test_point_ddpm.py:85-92), but all pairs run in ONE enqueue of batched kernels (`pcd_pair_metrics`) with no host
    synchronisation.  `a_clouds` / `b_clouds`: (P, N, 3) tensors or python lists of ragged (n_i, 3) clouds; a pair with
    an empty cloud has no metrics (the reference would raise) and gets a NaN row.  The exact Hungarian EMD
    (use_approximate_gpu_emd=False) stays a host-side scipy solve per pair, exactly as in the reference."""
    P = len(a_clouds)
    dev = a_clouds[0].device if P else torch.device("cuda")
    rows = torch.full((P, 3), float("nan"), dtype=torch.float32, device=dev)
    keep = [i for i in range(P) if a_clouds[i].shape[0] > 0 and b_clouds[i].shape[0] > 0]
    if not keep:
        return rows
    if dev.type != "cuda":
        raise RuntimeError("metrics run only on an MI355X device: move the clouds to 'cuda' (no CPU path)")

    def pack(clouds):
        counts = [int(clouds[i].shape[0]) for i in keep]
        if isinstance(clouds, torch.Tensor) and len(keep) == P:
            return clouds.to(torch.float32).contiguous(), counts
        buf = torch.zeros(len(keep), max(counts), 3, dtype=torch.float32, device=dev)
        for j, i in enumerate(keep):
            buf[j, :counts[j]] = clouds[i]
        return buf, counts

    out = _pair_call(*pack(a_clouds), *pack(b_clouds), use_approximate_gpu_emd, epsilon, thresh, max_iter)
    out[:, 0] *= 1e3                                         # chamfer_distance's default scaling_factor
    if not use_approximate_gpu_emd:
        for j, i in enumerate(keep):
            out[j, 1] = earth_mover_distance_cpu(a_clouds[i], b_clouds[i]).to(torch.float32)
    rows[torch.tensor(keep, device=dev)] = out
    return rows


def compute_metrics(generated_samples, reference_samples, use_approximate_gpu_emd=False):
    """metrics.py:160-183 -> (chamfer x1e3, EMD, voxel BCE)."""
    avg_cd = chamfer_distance(generated_samples, reference_samples)
    if use_approximate_gpu_emd:
        avg_emd = earth_mover_distance_gpu(generated_samples, reference_samples)
    else:
        avg_emd = earth_mover_distance_cpu(generated_samples, reference_samples)
    recon_loss = voxel_bce(voxelize(generated_samples), voxelize(reference_samples))
    return avg_cd, avg_emd, recon_loss


# ------------------------------------------------------------------ surface metrics (csrc/surface_metrics.hip; DESIGN.md "Surface metrics")
DEFAULT_THRESHOLDS = (0.02, 0.04, 0.1)          # 1, 2 and 5 % of the side of the [-1, 1] cube every conversion here uses


def surface_columns(thresholds=DEFAULT_THRESHOLDS):
    """Column names of a `surface_metrics` row: the ten of `_lib.PCD_SURF_ROW`, then PRECISION / RECALL / FSCORE per threshold."""
    cols = list(_lib.PCD_SURF_ROW)
    for t in thresholds:
        cols += [f"PRECISION@{float(t):g}", f"RECALL@{float(t):g}", f"FSCORE@{float(t):g}"]
    return cols


def _pack_clouds(clouds, counts=None, what="clouds"):
    """(P, N, 3) tensor or list of ragged (n_i, 3) clouds -> fp32 (P, max(N, 1), 3) device buffer (zeros past a count) and int32 device counts."""
    if isinstance(clouds, torch.Tensor):
        if clouds.dim() != 3 or clouds.shape[-1] != 3:
            raise ValueError(f"{what} must be a (P, N, 3) tensor or a list of (n, 3) tensors")
        if clouds.device.type != "cuda":
            raise RuntimeError("metrics run only on an MI355X device: move the clouds to 'cuda' (no CPU path)")
        P, n = clouds.shape[0], clouds.shape[1]
        buf = clouds.to(torch.float32).contiguous() if n > 0 else torch.zeros(P, 1, 3, dtype=torch.float32, device=clouds.device)
        if counts is None:
            cnt = torch.full((P,), n, dtype=torch.int32, device=clouds.device)
        else:
            cnt = torch.as_tensor(counts).to(device=clouds.device, dtype=torch.int32).clamp(0, n).contiguous()
            if cnt.shape != (P,):
                raise ValueError(f"the counts of {what} must have one entry per pair")
        return buf, cnt
    clouds = list(clouds)
    if counts is not None:
        raise ValueError(f"counts go with a padded tensor; a list of {what} carries its own sizes")
    for c in clouds:
        if c.device.type != "cuda":
            raise RuntimeError("metrics run only on an MI355X device: move the clouds to 'cuda' (no CPU path)")
        if c.dim() != 2 or c.shape[1] != 3:
            raise ValueError(f"{what} must be a (P, N, 3) tensor or a list of (n, 3) tensors")
    if not clouds:
        raise ValueError(f"no {what}")
    dev = clouds[0].device
    sizes = [int(c.shape[0]) for c in clouds]
    buf = torch.zeros(len(clouds), max(1, max(sizes)), 3, dtype=torch.float32, device=dev)
    for i, c in enumerate(clouds):
        buf[i, :sizes[i]] = c
    return buf, torch.tensor(sizes, dtype=torch.int32).to(dev)


def nearest_neighbors(queries, targets, query_counts=None, target_counts=None):
    """For every query point its nearest target: -> (d2 (P, N) float32, index (P, N) int32) with d2 = min_j ((dx dx + dy dy) + dz dz) in
    fp32 from direct differences and index the LOWEST j that attains it.  `queries` / `targets`: (P, N, 3) / (P, M, 3) device tensors
    (`*_counts` (P,) optionally say how many rows of each pair count) or lists of ragged (n_i, 3) clouds, padded here.  A query with no finite
    distance to any target (a non-finite query, no targets, all targets non-finite) and every row past a count get (NaN, -1); a non-finite
    target is nobody's neighbour.  One enqueue for all pairs, bitwise repeatable, a pair's result independent of the rest of the batch."""
    q, nq = _pack_clouds(queries, query_counts, "queries")
    t, nt = _pack_clouds(targets, target_counts, "targets")
    if q.shape[0] != t.shape[0]:
        raise ValueError("queries and targets must hold the same number of pairs")
    P, N, M = q.shape[0], q.shape[1], t.shape[1]
    lib = _lib.load()
    d2 = torch.empty(P, N, dtype=torch.float32, device=q.device)
    index = torch.empty(P, N, dtype=torch.int32, device=q.device)
    need = int(lib.pcd_nearest_workspace_bytes(P, N, M))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=q.device)
    _lib.check(lib.pcd_nearest_neighbors(q.data_ptr(), nq.data_ptr(), N, t.data_ptr(), nt.data_ptr(), M, P, d2.data_ptr(), index.data_ptr(),
                                         ws.data_ptr(), need, _lib.stream_ptr()), "nearest_neighbors")
    return d2, index


def surface_metrics(a, b, normals_a=None, normals_b=None, thresholds=DEFAULT_THRESHOLDS) -> torch.Tensor:
    """(P, 10 + 3 K) float32 rows of the standard surface-reconstruction metrics between the point sets a_p and b_p (a the prediction, b the
    reference), in the coordinates given -- no per-cloud normalisation.  Columns (`surface_columns(thresholds)`), with d the distance of a
    point to its nearest neighbour in the other set: ACC / COMP = mean d over a / over b, CHAMFER_L1 = their mean, ACC2 / COMP2 = the means
    of d^2, CHAMFER_L2 = their sum, HAUSDORFF = the largest d of both directions, NC_A / NC_B = mean |n . n'| of a point's normal with its
    nearest neighbour's (NC their mean; NaN unless both `normals_*` are given), then per threshold t PRECISION = the share of a within t of
    b, RECALL = the share of b within t of a (d^2 <= t t), FSCORE = their harmonic mean (0 when both are 0).  The normal consistency takes
    the ABSOLUTE dot product, the standard choice: it is blind to a flipped winding, on purpose.  `a` / `b` (and the normals, packed the
    same way): (P, N, 3) device tensors or lists of ragged (n_i, 3) clouds.  A pair with an empty cloud, or with any non-finite coordinate,
    gets an all-NaN row; the other rows are not affected.  One enqueue (`pcd_surface_metrics`), no host synchronisation; means in double,
    rounded once; bitwise repeatable and independent of the rest of the batch."""
    thresholds = tuple(float(t) for t in thresholds)
    if len(thresholds) > _lib.PCD_SURF_MAX_THRESHOLDS or any(not (np.isfinite(t) and t >= 0.0) for t in thresholds):
        raise ValueError(f"thresholds must be at most {_lib.PCD_SURF_MAX_THRESHOLDS} finite values >= 0, got {thresholds!r}")
    pa, na = _pack_clouds(a, None, "a")
    pb, nb = _pack_clouds(b, None, "b")
    if pa.shape[0] != pb.shape[0]:
        raise ValueError("a and b must hold the same number of pairs")
    P, NA, NB = pa.shape[0], pa.shape[1], pb.shape[1]
    ka = kb = None
    if normals_a is not None and normals_b is not None:
        ka, _ = _pack_clouds(normals_a, None, "normals_a")
        kb, _ = _pack_clouds(normals_b, None, "normals_b")
        if ka.shape != pa.shape or kb.shape != pb.shape:
            raise ValueError("normals must be shaped like their clouds")
    lib = _lib.load()
    K = len(thresholds)
    rows = torch.empty(P, _lib.PCD_SURF_ROW_BASE + 3 * K, dtype=torch.float32, device=pa.device)
    need = int(lib.pcd_surface_metrics_workspace_bytes(P, NA, NB))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=pa.device)
    taus = (_lib.f32 * max(K, 1))(*thresholds)
    _lib.check(lib.pcd_surface_metrics(pa.data_ptr(), _lib.ptr(ka), na.data_ptr(), NA, pb.data_ptr(), _lib.ptr(kb), nb.data_ptr(), NB, P, taus,
                                       K, rows.data_ptr(), None, None, None, None, ws.data_ptr(), need, _lib.stream_ptr()), "surface_metrics")
    return rows


def voxel_iou(a: torch.Tensor, b: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
    """(P,) float32 intersection over union of two batches of grids (P, ...) with occupancy value > threshold, counted in integers; NaN where
    both grids are empty."""
    if a.shape != b.shape or a.dim() < 2:
        raise ValueError("grids must be two (P, ...) tensors of the same shape")
    if a.device.type != "cuda" or b.device.type != "cuda":
        raise RuntimeError("metrics run only on an MI355X device: move the grids to 'cuda' (no CPU path)")
    P = a.shape[0]
    ga, gb = a.to(torch.float32).reshape(P, -1).contiguous(), b.to(torch.float32).reshape(P, -1).contiguous()
    out = torch.empty(P, dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().pcd_voxel_iou(ga.data_ptr(), gb.data_ptr(), P, ga.shape[1], float(threshold), out.data_ptr(), _lib.stream_ptr()),
               "voxel_iou")
    return out


def mesh_columns(thresholds=DEFAULT_THRESHOLDS):
    """Column names of a `mesh_metrics` row: `surface_columns(thresholds)` and IOU."""
    return surface_columns(thresholds) + ["IOU"]


def mesh_metrics(meshes_a, meshes_b, num_points=10000, thresholds=DEFAULT_THRESHOLDS, seed=0, iou_resolution=32, iou_fill="solid",
                 bounds=(-1.0, 1.0), return_samples=False):
    """(P, 10 + 3 K + 1) float32 rows (`mesh_columns(thresholds)`) scoring the meshes a_p against b_p, lists of `Mesh` / (vertices, faces)
    pairs on the device: `num_points` points with face normals are drawn by area from each surface (`utils.sample_mesh_points`; side a
    under `seed`, side b under `seed + 1`, so a mesh compared with itself is not compared with the same draws), `surface_metrics` scores
    the samples, and the last column IOU is `voxel_iou` of `utils.meshes_to_voxel_tensor(..., iou_resolution, iou_fill, bounds)` of both
    sides (NaN with `iou_resolution=None`).  A pair in which either mesh has no faces -- a decoded field below the threshold -- gets a NaN
    row.  With `return_samples` also a dict: `keep` (the pairs that were scored) and their `points_a`, `normals_a`, `points_b`, `normals_b`."""
    from .utils import meshes_to_voxel_tensor, sample_mesh_points
    meshes_a, meshes_b = list(meshes_a), list(meshes_b)
    if len(meshes_a) != len(meshes_b):
        raise ValueError("meshes_a and meshes_b must hold the same number of meshes")
    P, K = len(meshes_a), len(tuple(thresholds))
    for m in meshes_a + meshes_b:
        if m[0].device.type != "cuda" or m[1].device.type != "cuda":
            raise RuntimeError("metrics run only on an MI355X device: move the meshes to 'cuda' (no CPU path)")
    dev = meshes_a[0][0].device if P else torch.device("cuda")
    rows = torch.full((P, _lib.PCD_SURF_ROW_BASE + 3 * K + 1), float("nan"), dtype=torch.float32, device=dev)
    keep = [i for i in range(P) if all(m[0].shape[0] > 0 and m[1].shape[0] > 0 for m in (meshes_a[i], meshes_b[i]))]
    samples = dict(keep=keep, points_a=None, normals_a=None, points_b=None, normals_b=None)
    if keep:
        ka, kb = [meshes_a[i] for i in keep], [meshes_b[i] for i in keep]
        pa, na = sample_mesh_points(ka, num_points, seed=int(seed), return_normals=True)
        pb, nb = sample_mesh_points(kb, num_points, seed=int(seed) + 1, return_normals=True)
        samples.update(points_a=pa, normals_a=na, points_b=pb, normals_b=nb)
        out = torch.full((len(keep), rows.shape[1]), float("nan"), dtype=torch.float32, device=dev)
        out[:, :-1] = surface_metrics(pa, pb, na, nb, thresholds)
        if iou_resolution is not None:
            out[:, -1] = voxel_iou(meshes_to_voxel_tensor(ka, iou_resolution, iou_fill, bounds),
                                   meshes_to_voxel_tensor(kb, iou_resolution, iou_fill, bounds))
        rows[torch.tensor(keep, device=dev)] = out
    return (rows, samples) if return_samples else rows
