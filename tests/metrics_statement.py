"""The CPU statement of the evaluation metrics, stage by stage: `normalize_to_cube`, Chamfer, the log-domain Sinkhorn EMD
(reference metrics.py:7-47, 94-183) and the voxel BCE (utils.py:488-509), in plain torch with the reference's operations in the
reference's order.  Two things differ from the reference on purpose:
  * distances are direct differences, d2 = dx*dx + dy*dy + dz*dz summed left to right, never the matmul form of `torch.cdist`
    (which cancels: SURVEY A.5).  In fp32 that is the expression of the HIP kernels that are compiled without contraction, so
    their stages equal this statement bit for bit;
  * every stage is returned, not only the last number.
`dtype` selects the precision of every stage after the normalisation: torch.float32 is what the kernels should compute,
torch.float64 is the yardstick.  The normalisation itself always runs in fp32, as the reference does on its fp32 clouds and as
`oracle.torch_oracle.chamfer_distance_exact` does: it is a bit-exact stage of the kernels, so the yardstick for the stages behind
it starts from the same clouds.  log(mu + 1e-10) is likewise the fp32 value the host hands to the kernels.

Per-pair form: `pair(a, b, ...)` (own cost maximum, own stop).  Batch-joint form: `sinkhorn(xn, yn, ...)` on (B, n, 3) / (B, m, 3)
(one `C.max()` and one stop test for the whole batch, as metrics.py:120-150 does with a batch and as `shapegen_amd.sinkhorn`
does)."""
import torch
import torch.nn.functional as F


def normalize(p):
    """metrics.py:17-21 on (..., n, 3), in p's dtype."""
    center = (p.max(dim=-2, keepdim=True)[0] + p.min(dim=-2, keepdim=True)[0]) / 2
    p = p - center
    scale = p.abs().max(dim=-2, keepdim=True)[0].max(dim=-1, keepdim=True)[0]
    return p / scale


def sq_dists(x, y):
    """|x_i - y_j|^2 as (..., n, m) by direct differences, ((dx*dx + dy*dy) + dz*dz)."""
    dx = x[..., :, None, 0] - y[..., None, :, 0]
    dy = x[..., :, None, 1] - y[..., None, :, 1]
    dz = x[..., :, None, 2] - y[..., None, :, 2]
    return dx * dx + dy * dy + dz * dz


def chamfer(xn, yn):
    """metrics.py:41-46 on normalised clouds (n, 3), (m, 3): per-query min d^2 in both directions, the two sums of the unsquared
    minima and the distance (scaling 1).  sqrt is monotone, so sqrt(min d^2) is the reference's min of the distances."""
    d2 = sq_dists(xn, yn)
    mins_a, mins_b = d2.min(dim=1)[0], d2.min(dim=0)[0]
    ra, rb = mins_a.sqrt(), mins_b.sqrt()
    return dict(mins_a=mins_a, mins_b=mins_b, sums=torch.stack([ra.sum(), rb.sum()]), chamfer=ra.mean() + rb.mean())


def log_marginal(n):
    """log(mu + 1e-10) of metrics.py:133-134,141 with fp32 torch ops: what the host computes and hands to the kernels."""
    return torch.log(torch.ones(1) / n + 1e-10)[0]


def dual_update(dist, cmax, epsilon, log_marg, dual_q):
    """metrics.py:141 (and :144 with `dist` transposed): rows of `dist` (..., n, m) against the dual of the columns (..., m)."""
    C = dist / cmax
    return epsilon * (log_marg - torch.logsumexp(-(1 / epsilon) * C + dual_q[..., None, :], dim=-1))


def row_costs(dist, cmax, epsilon, alpha, beta):
    """metrics.py:153-156 before the last sum: sum_j P_ij C_ij per row."""
    C = dist / cmax
    P = torch.exp(-(1 / epsilon) * C + alpha[..., :, None] + beta[..., None, :])
    return (P * C).sum(dim=-1)


def sinkhorn(xn, yn, epsilon=1e-2, thresh=1e-5, max_iter=100, dtype=torch.float64):
    """metrics.py:116-158 on normalised clouds (B, n, 3), (B, m, 3), batch-joint: one cost maximum and one stop test for the batch.
    -> cmax, iters (one dict per iteration run: alpha (B, n), beta (B, m), err_alpha, err_beta), stop (iterations run), alpha, beta,
    row_cost (B, n), emd (B,)."""
    xn, yn = xn.to(dtype), yn.to(dtype)
    n, m = xn.shape[-2], yn.shape[-2]
    dist = sq_dists(xn, yn).sqrt()
    cmax = dist.max()
    log_mu, log_nu = log_marginal(n).to(dtype), log_marginal(m).to(dtype)
    alpha = torch.zeros(xn.shape[:-1], dtype=dtype)
    beta = torch.zeros(yn.shape[:-1], dtype=dtype)
    dist_t = dist.transpose(-1, -2)
    iters = []
    for _ in range(max_iter):
        a_prev, b_prev = alpha, beta
        alpha = dual_update(dist, cmax, epsilon, log_mu, beta)
        beta = dual_update(dist_t, cmax, epsilon, log_nu, alpha)
        err_a, err_b = (alpha - a_prev).abs().max(), (beta - b_prev).abs().max()
        iters.append(dict(alpha=alpha, beta=beta, err_alpha=err_a, err_beta=err_b))
        if err_a < thresh and err_b < thresh:
            break
    rc = row_costs(dist, cmax, epsilon, alpha, beta)
    return dict(cmax=cmax, iters=iters, stop=len(iters), alpha=alpha, beta=beta, row_cost=rc, emd=rc.sum(dim=-1))


def voxel_indices(points, res=32):
    """utils.py:501-502 on fp32 points (..., 3): the clamped integer coordinates."""
    return ((points + 1) * (res - 1) / 2).long().clamp(0, res - 1)


def voxelize(points, res=32):
    """utils.py:488-509 for one cloud (n, 3): occupancy (res, res, res) indexed [x][y][z]."""
    idx = voxel_indices(points, res)
    vox = torch.zeros(res, res, res)
    vox[idx[:, 0], idx[:, 1], idx[:, 2]] = 1
    return vox


def pair(a, b, dtype=torch.float64, with_sinkhorn=True, epsilon=1e-2, thresh=1e-5, max_iter=100):
    """What `compute_metrics(a, b, use_approximate_gpu_emd=True)` (metrics.py:160-183) computes for ONE pair of fp32 clouds (n, 3),
    (m, 3), every stage kept: an, bn (fp32), mins_a, mins_b, sums, chamfer, then the keys of `sinkhorn` without the batch axis,
    then vox_a, vox_b (indices of the RAW clouds, as metrics.py:181 passes them) and bce."""
    a, b = a.to(torch.float32), b.to(torch.float32)
    an, bn = normalize(a), normalize(b)
    out = dict(an=an, bn=bn)
    out.update(chamfer(an.to(dtype), bn.to(dtype)))
    if with_sinkhorn:
        s = sinkhorn(an[None], bn[None], epsilon, thresh, max_iter, dtype)
        out.update(cmax=s["cmax"], stop=s["stop"], alpha=s["alpha"][0], beta=s["beta"][0], row_cost=s["row_cost"][0], emd=s["emd"][0],
                   iters=[dict(alpha=i["alpha"][0], beta=i["beta"][0], err_alpha=i["err_alpha"], err_beta=i["err_beta"])
                          for i in s["iters"]])
    out.update(vox_a=voxel_indices(a), vox_b=voxel_indices(b), bce=F.binary_cross_entropy(voxelize(a), voxelize(b)))
    return out
