"""Inputs shared by tests/test_metrics_statement_cpu.py (which records how far the fp32 statement lies from the fp64 one on them)
and tests/test_gpu_metrics.py (whose bounds are 8 x those deviations).  Everything comes from seeded CPU generators."""
import functools

import torch


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def lattice(n, seed):
    """n points of a cubic lattice of spacing 1/6, each coordinate jittered by +-0.01: neighbours stay >= 1/6 - 0.02 apart."""
    g = _gen(seed)
    side = 1
    while side ** 3 < n:
        side += 1
    idx = torch.randperm(side ** 3, generator=g)[:n]
    ijk = torch.stack([idx // (side * side), (idx // side) % side, idx % side], 1).to(torch.float32)
    return ijk / 6 + (torch.rand(n, 3, generator=g) * 2 - 1) * 0.01


def matched(n, m, seed):
    """The matched-cloud design: the larger cloud is a jittered lattice, the smaller one a random permutation of (a subset of) it
    plus +-0.002.  Every point of the smaller cloud is then the unique nearest neighbour of exactly one point of the larger one,
    ~60 times closer than any other, so dropping any single target moves the Chamfer distance by ~(1/6) / n."""
    big = lattice(max(n, m), seed)
    g = _gen(seed + 1)
    small = big[torch.randperm(max(n, m), generator=g)[:min(n, m)]] + (torch.rand(min(n, m), 3, generator=g) * 2 - 1) * 0.002
    return (big, small) if n >= m else (small, big)


def uniform(n, m, seed):
    g = _gen(seed)
    return torch.rand(n, 3, generator=g) * 2 - 1, torch.rand(m, 3, generator=g) * 2 - 1


def gaussian(n, m, seed):
    g = _gen(seed)
    return torch.randn(n, 3, generator=g), 0.7 * torch.randn(m, 3, generator=g) + 0.2


def make(kind, n, m, seed):
    return {"matched": matched, "uniform": uniform, "gaussian": gaussian}[kind](n, m, seed)


def pack(clouds):
    """Ragged (n_i, 3) clouds -> padded (P, max n, 3) fp32 (padding 7.0: no kernel may read it) and int32 counts."""
    nmax = max(1, max(c.shape[0] for c in clouds))
    buf = torch.full((len(clouds), nmax, 3), 7.0)
    for i, c in enumerate(clouds):
        buf[i, :c.shape[0]] = c
    return buf, torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32)


# ---- Chamfer launch shapes of pcd_pair_metrics.  With NQ = max(na_max, nb_max): cqblocks = ceil(NQ / 1024),
# tsplit = clamp(ceil(1024 / (cqblocks * 2P)), 1, max_split = ceil(NQ / 128)), targets per split = ceil(nr / tsplit) in LDS tiles of 512.
#   name: (pairs as (kind, n, m), indices of the pairs the statement is evaluated on)
CHAMFER_CASES = {
    # cqblocks 2, tsplit = ceil(1024 / 1024) = 1: every block walks all targets, tiles 512 + 512 + 76 (b) and 512 + 512 + 276 (a)
    "tsplit1_tiles": ([("matched", 1300, 1100)] * 256, (0, 1, 37, 100, 128, 200, 254, 255)),
    # cqblocks 2, tsplit = ceil(1024 / 4) = 256 clamped to max_split = 16: 128 targets per split
    "tsplit_clamped": ([("matched", 2048, 2048)], (0,)),
    # cqblocks 2, max_split = 11; P = 26 is the smallest P with ceil(1024 / (4P)) = 10 < 11 (P = 25 gives 11): 130 targets per split
    "tsplit_between": ([("matched", 1300, 1300)] * 26, tuple(range(26))),
    # NQ 1300: cqblocks 2, tsplit 43 -> 11.  (257, 3): one target per split, splits 3..10 empty; (5, 40): 5 live queries, slots
    # 1..3 of every thread and slot 0 of threads >= 5 are clamped duplicates; the second query block returns for all but the last pair
    "ragged": ([("matched", 1025, 513), ("matched", 512, 1024), ("uniform", 257, 3), ("uniform", 5, 40), ("matched", 1300, 1300),
                ("uniform", 0, 9)], (0, 1, 2, 3, 4)),
    # NQ 8: cqblocks 1, tsplit 1 = max_split, 1024 blocks of which 8 threads each hold a live query
    # (a one-point cloud normalises to 0 / 0: the normalisation test has it)
    "many_tiny": ([("uniform", 2 + (i * 5) % 7, 2 + (i * 3) % 7) for i in range(512)], tuple(range(512))),
}


def chamfer_case(name):
    spec, check = CHAMFER_CASES[name]
    clouds = [make(kind, n, m, 1000 + 7 * i) for i, (kind, n, m) in enumerate(spec)]
    return [c[0] for c in clouds], [c[1] for c in clouds], check


# ---- Sinkhorn through the pair entry: one call per case.  name: (pairs, epsilon, thresh, max_iter)
PAIR_SINKHORN_CASES = {
    "eps0.01": ([("uniform", 300, 257), ("gaussian", 513, 777), ("matched", 1025, 1025), ("uniform", 5, 40), ("uniform", 2048, 2048)],
                1e-2, 1e-5, 100),
    # pairs that stop at different iterations in one call (the stop is per pair, on the device): the first after 3, the others after 4
    "stops_differ": ([("uniform", 5, 40), ("uniform", 300, 257), ("gaussian", 513, 777), ("uniform", 64, 500)], 0.05, 2e-5, 100),
    # iteration 1 of the first pair ends with err_alpha 0.138 < thresh < err_beta 0.326: beta alone keeps it running (both stop after 2)
    "beta_decides": ([("uniform", 5, 40), ("uniform", 300, 257)], 0.05, 0.212, 100),
    "max_iter_first": ([("uniform", 5, 40), ("uniform", 300, 257)], 0.05, 1e-5, 2),
    "never_stops": ([("uniform", 5, 40), ("gaussian", 64, 100)], 0.05, 0.0, 100),
}


def pair_sinkhorn_case(name):
    spec, epsilon, thresh, max_iter = PAIR_SINKHORN_CASES[name]
    clouds = [make(kind, n, m, 2000 + 11 * i) for i, (kind, n, m) in enumerate(spec)]
    return [c[0] for c in clouds], [c[1] for c in clouds], epsilon, thresh, max_iter


@functools.lru_cache(maxsize=None)
def pair_sinkhorn_statements(name):
    """[(fp64 statement, fp32 statement)] of every pair of the case, each pair on its own (own cost maximum, own stop)."""
    import metrics_statement as S
    a, b, epsilon, thresh, max_iter = pair_sinkhorn_case(name)
    return [tuple(S.pair(x, y, dt, True, epsilon, thresh, max_iter) for dt in (torch.float64, torch.float32)) for x, y in zip(a, b)]


def deviation(r32, r64, key, relative=False):
    """max |fp32 statement - fp64 statement| of one stage (relative to the fp64 value for a scalar such as the EMD)."""
    d = (r32[key].double() - r64[key]).abs()
    return float((d / r64[key].abs()).max()) if relative else float(d.max())


def stop_margin(r64, thresh):
    """How far (as a factor >= 1 on either side) the errors that decide the stop of an fp64 run lie from `thresh`: the smaller of
    thresh / max(err) at the iteration that stopped and max(err) / thresh at every iteration that went on."""
    f = float("inf")
    for k, it in enumerate(r64["iters"]):
        e = max(float(it["err_alpha"]), float(it["err_beta"]))
        if k == len(r64["iters"]) - 1 and e < thresh:
            f = min(f, thresh / e if e > 0 else float("inf"))
        else:
            f = min(f, e / thresh if thresh > 0 else float("inf"))
    return f


# ---- batch-joint entry points: (n, m) with batch 3, normalised clouds
JOINT_SIZES = ((257, 513), (1025, 300), (64, 500))
JOINT_EPSILONS = (1e-2, 0.2)


def joint_case(n, m):
    """x (3, n, 3), y (3, m, 3) normalised (uniform, Gaussian, uniform), a non-zero dual of y and a dual of x to be overwritten."""
    from metrics_statement import normalize
    g = _gen(3000 + n)
    x = torch.stack([uniform(n, m, 31 + n)[0], gaussian(n, m, 32 + n)[0], uniform(n, m, 33 + n)[0]])
    y = torch.stack([uniform(n, m, 31 + n)[1], gaussian(n, m, 32 + n)[1], uniform(n, m, 33 + n)[1]])
    dual_q = (torch.rand(3, m, generator=g) * 2 - 1) * 0.05
    dual_p = (torch.rand(3, n, generator=g) * 2 - 1) * 0.05
    return normalize(x), normalize(y), dual_q, dual_p


@functools.lru_cache(maxsize=None)
def joint_stages(n, m, epsilon):
    """One alpha half-iteration from the non-zero dual and the cost stage, in fp64 and fp32, on fp32 inputs shared with the kernels:
    cmax (the fp32 statement's), log_mu, and for the cost stage the duals of a converged fp64 run rounded to fp32."""
    import metrics_statement as S
    x, y, dual_q, dual_p = joint_case(n, m)
    cmax = S.sq_dists(x, y).sqrt().max()
    log_mu = S.log_marginal(n)
    done = S.sinkhorn(x, y, epsilon)
    alpha, beta = done["alpha"].float(), done["beta"].float()
    out = dict(cmax=cmax, log_mu=log_mu, alpha=alpha, beta=beta)
    for dt in (torch.float64, torch.float32):
        dist = S.sq_dists(x.to(dt), y.to(dt)).sqrt()
        rc = S.row_costs(dist, cmax.to(dt), epsilon, alpha.to(dt), beta.to(dt))
        out[dt] = dict(dual=S.dual_update(dist, cmax.to(dt), epsilon, log_mu.to(dt), dual_q.to(dt)), row_cost=rc, cost=rc.sum(dim=-1))
    return out


def joint_stage_deviations(n, m, epsilon):
    s = joint_stages(n, m, epsilon)
    r64, r32 = s[torch.float64], s[torch.float32]
    return dict(dual=deviation(r32, r64, "dual"), row_cost=deviation(r32, r64, "row_cost"), cost=deviation(r32, r64, "cost", True))


# ---- pcd_binary_bce_mean: lengths below, at and far above the block of 1024, none but the last a multiple of it
BCE_LENGTHS = (315, 1025, 32768 * 2)
BCE_KINDS = ("binary", "probabilities", "clamped")


def bce_case(n, kind):
    """-> x, target (n,) fp32 and the exact mean where there is one.  binary: two occupancy grids that differ in k voxels, the last
    one among them (every differing voxel costs exactly 100).  probabilities: x in (0, 1) against binary targets.  clamped: x exactly
    0 or 1 (and a few probabilities) against both targets, so log(0) meets the -100 clamp on either side."""
    g = _gen(4000 + n)
    t = (torch.rand(n, generator=g) < 0.4).float()
    if kind == "binary":
        flip = torch.rand(n, generator=g) < 0.1
        flip[-1] = True
        x = torch.where(flip, 1 - t, t)
        return x, t, 100.0 * int(flip.sum()) / n
    if kind == "probabilities":
        return torch.rand(n, generator=g).clamp(1e-6, 1 - 1e-6), t, None
    x = (torch.rand(n, generator=g) < 0.5).float()
    soft = torch.rand(n, generator=g) < 0.25
    x = torch.where(soft, torch.rand(n, generator=g).clamp(1e-6, 1 - 1e-6), x)
    x[-1], t[-1] = 0.0, 1.0
    x[0], t[0] = 1.0, 0.0
    return x, t, None
