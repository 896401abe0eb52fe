"""Cases, fp64 statements, fp32 statements in the kernels' order, and derived error bounds for the kernels of csrc/train.hip.
Shared by tests/test_train_cases_cpu.py (which holds this file to account on the CPU) and tests/test_gpu_train_kernels.py (which judges
every launch against it, column by column).  Plain torch on the CPU, seeded CPU generators, float64 arithmetic; nothing of the library
is imported here.

Notation: u32 = 2^-24 and u16 = 2^-11 are the unit roundoffs of fp32 and fp16 (half an ulp, relative).

SUMS.  A kernel sum over terms t_i lies within  sum_bound(L, sum|t_i|) = 1.1 * L * u32 * sum|t_i|  of the fp64 sum, L being the longest
chain of additions any term goes through: every addition rounds its partial sum by at most u32 relative, the partial sums are at
most sum|t_i|, so n chained additions cost (1 + u32)^n - 1 <= 1.1 n u32 for every n used here.  A correct kernel reaches this only if
every rounding of its longest chain goes the same way, and a dropped row costs about sum|t| / m, thousands of times more.
  column strips (cr_grid below restates csrc/train.hip's): a lane adds rpb / 32 rows, 32 lanes are added in order, then the chunks in
      order: L = strip_chain(c, rows, groups) = rpb / 32 + 32 + chunks >= 37, for pcd_colsum_f16 and dbeta (terms exact in fp32),
      pcd_vec3_outer (terms carry one product rounding) and dgamma (terms g * xhat carry the roundings of xhat = (z - mean) * rstd:
      subtraction 1, rsqrtf 1 ulp = 2 and its argument 1/2, two products: 5.5 u32 relative).  The roundings on the terms are not links
      of L; against the 37 and more additions they are what the factor 1.1 and the one-way worst case leave room for, and
      tests/test_train_cases_cpu.py shows the fp32 statement in the kernels' order at no more than 0.2 of these bounds.
  pcd_bn_batch_stats: d = z - z[0].  |mean - fp64| <= sum_bound(L, sum|d|) / m + 2 u32 |mean|  (the sum of d; the division and the
      final z[0] + s1 / m round the mean itself).
      var = s2 / m - (s1 / m)^2 with s2 = sum d^2 (d^2 carries 3 roundings): the s2 part is within (L + 4) u32 mean(d^2), the square of
      s1 / m within 2 (L + 2) u32 (mean|d|)^2 <= 2 (L + 2) u32 mean(d^2) (Cauchy-Schwarz), the subtraction u32 mean(d^2): together
      (3 L + 9) u32 mean(d^2) <= var_bound = 4 L u32 mean(d^2) since L >= 37.  mean(d^2) = var + (mean - z[0])^2 is what the one-pass
      formula cancels against.  A constant column has d = 0 exactly: both bounds are 0 there and the kernel must be exact.
      running = (1 - momentum) * running + momentum * new: the two products, the difference 1 - momentum and the sum are 4 roundings on
      the sum of the magnitudes, plus momentum times the error of new; the unbiased factor m / (m - 1) adds 2 roundings.
  pcd_matmul_f32, by route: 64 + ceil(k / 64) (few rows, B [k][n]: 64 deep blocks, then the blocks in order), ceil(k / 64) + 6 (few rows,
      B [n][k]: a lane's stride, then 6 butterfly steps), and k + 3 on the generic route.  The generic chain was first taken as k, the
      additions of the products alone.  That missed three roundings which at small k are the whole error: each product a * b is
      rounded, the bias is the chain's first addend and, with accumulate, the old C is added last.  At k = 1 these three are all there
      is, and the fp32 statement (correct code, tests/test_train_cases_cpu.py) stands at 1.94 x the bound with L = k on the case
      33 x 1 x 257 with bias and accumulate; so the generic chain counts them.  The two few-rows routes have the same three roundings
      behind chains of 7 and 65 and more links, and keep theirs.
  pcd_l1_loss: a lane's grid stride, 8 tree levels, one atomic add per block: strides + 8 + blocks.
  GroupNorm (not set by anything but this file): a lane's stride over the group and 6 butterfly steps, ceil(gsz / 64) + 6, plus the
      roundings on the terms; dgamma / dbeta: one thread adds the rows: rows (+ 4 on g * xhat).

ELEMENTS.  An fp16 output is within  half_bound(want, S, K) = u16 |want| + K u32 S + 2^-25  (want clamped to +-65504 as the kernels
saturate; S the sum of the magnitudes of the terms of the expression; 2^-25 half the fp16 subnormal spacing).  K counts roundings, each
rounding of a sub-expression being at most u32 times the magnitudes below it; the count is rounded up to the K stated, which also
covers the second-order term u16 K u32 S (the fp16 rounding acts on the fp32 value, not on `want`):
  pcd_bn_apply_f16: (z - mean) 1, rsqrtf 2 (1 ulp) + 1/2 (its argument), times gamma 1, product 1, + beta 1: 6.5, K = 8.
  pcd_bn_backward_f16 dz = (gamma * rstd) * (g - dbeta / m - xhat * dgamma / m): xhat 4.5; 1 / m and the product 2 each on dbeta / m and
      dgamma / m; xhat * (dgamma / m) 7.5; two subtractions: the bracket is within 8.5 u32 of its term magnitudes; gamma * rstd 3.5 and
      the outer product 1: 13.  K = 16.
  pcd_vec3_expand_f16: the three products (u32 on each term: 1 on S), two additions: 3, K = 4.
  pcd_enc1_linear (fp32 out, no second-order term): the three products 1, three additions 3: K = 4.
  SiLU y = x / (1 + expf(-x)): expf 1 ulp = 2, addition 1, division 1: K = 4.  Where expf(-x) overflows fp32 (x < -88.7) the kernel
      gives 0 for a true |y| < |x| / FLT_MAX: that floor is added (it is a property of the number format).  Its backward
      dy * s * (1 + x * (1 - s)), s = 1 / (1 + expf(-x)): s within 4 u32, 1 - s within 4 u32 s + u32, times x, plus 1, two products:
      within 8 u32 |dy| s (1 + |x|), floor |dy| (1 + |x|) (1 / FLT_MAX + 2^-149): s itself is subnormal just before the overflow
      and then carries an absolute rounding of 2^-150.
  GroupNorm y from the kernel's own (mean, rstd): subtraction, three products / additions: K = 4.  dx = rstd * (gg - s1 - xhat * s2):
      K = 8 on the term magnitudes plus the sum bounds of s1 (terms dy * gamma, then / gsz: chain + 2) and s2 (terms dy * gamma *
      xhat, xhat 2 roundings: chain + 5); they are not returned, so their error stays in this launch.
  AdamW: parameters within 4 u32 |w| + 4 u32 lr of the fp64 statement; exp_avg 4 roundings and exp_avg_sq 5 on their term magnitudes.

EACH STAGE IS FED ITS PREDECESSOR'S OWN fp32 OUTPUT: apply and backward take the fp32 (mean, var) of the case, dz the (dgamma, dbeta) the
entry point returned, GroupNorm's y and backward the (mean, rstd) its forward returned.  No error stacks across launches.

NO ELEMENT NEAR THE ReLU THRESHOLD.  bn_case / gn_case move every element whose fp64 pre-activation y = t + beta, t = (z - mean) * rstd
* gamma, has |y| < MARGIN * (|t| + |beta|) away from zero.  The forward form (z - mean) * (rstd * gamma) + beta and the backward form
((z - mean) * rstd) * gamma + beta differ from fp64 by at most 8 u32 (|t| + |beta|) = 5e-7 of that scale, MARGIN is 1e-3: the mask is
the same in fp64, in either fp32 form and in the kernel, and nothing is ever excluded from a comparison.  The only exempt columns are
the constant ones with beta = 0, whose pre-activation is exactly 0 in every arithmetic (z - mean = 0, 0 * x + 0 = 0): mask off."""
import functools
import math

import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -11
F16_MAX = 65504.0
FLT_MAX = 3.4028234663852886e38
EPS = float(torch.tensor(1e-5, dtype=torch.float32))          # the fp32 value the kernels receive
MOMENTUM = float(torch.tensor(0.1, dtype=torch.float32))
MARGIN = 1e-3
CR_COLS, CR_LANES = 64, 32


def f32(v):
    """A Python float rounded to fp32 (what a `float` argument of an entry point holds)."""
    return float(torch.tensor(v, dtype=torch.float32))


def sat16(t):
    """Round to fp16 as the kernels do: clamped to the largest normal, never +-inf."""
    return t.clamp(-F16_MAX, F16_MAX).half()


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ launch geometry
def cr_grid(c, rows_per_group, groups=1):
    """(rows per block, chunks per group) of the column-strip kernels: csrc/train.hip's cr_grid."""
    cb = ceil_div(c, CR_COLS)
    chunks = max(2048 // (cb * groups), 1)
    rpb = max(ceil_div(ceil_div(rows_per_group, chunks), CR_LANES) * CR_LANES, 4 * CR_LANES)
    return rpb, ceil_div(rows_per_group, rpb)


def strip_chain(c, rows_per_group, groups=1):
    rpb, chunks = cr_grid(c, rows_per_group, groups)
    return rpb // CR_LANES + CR_LANES + chunks


def matmul_route(m, trans_a, trans_b):
    return "generic" if trans_a or m > 32 else ("nt" if trans_b else "nn")


def matmul_chain(route, k):
    return {"generic": k + 3, "nn": 64 + ceil_div(k, 64), "nt": ceil_div(k, 64) + 6}[route]


def l1_blocks(n):
    return min(ceil_div(n, 256), 1024)


def l1_chain(n):
    return ceil_div(n, l1_blocks(n) * 256) + 8 + l1_blocks(n)


# ------------------------------------------------------------------------------------------------------------ bounds
def sum_bound(L, abs_sum):
    return 1.1 * L * U32 * abs_sum


def half_bound(want, S, K):
    return U16 * want.abs().clamp(max=F16_MAX) + K * U32 * S + 2.0 ** -25


def mean_bound(L, d_abs_sum, m, mean):
    return sum_bound(L, d_abs_sum) / m + 2 * U32 * mean.abs()


def var_bound(L, d_sq_mean):
    return 4 * L * U32 * d_sq_mean


# ------------------------------------------------------------------------------------------------------------ BatchNorm cases
FAMILIES = ("randn", "mean_p30", "mean_m30", "mean_p1000", "mean_m1000", "tiny_spread", "const", "zero", "row0_outlier",
            "last_outlier", "spike", "saturate", "const_beta0", "const_beta_pos", "const_beta_neg")
CONSTANT = ("const", "zero", "const_beta0", "const_beta_pos", "const_beta_neg")
EXEMPT = ("const_beta0",)          # pre-activation exactly 0
BN_MS = (1, 31, 32, 33, 128, 129, 257, 2305)
BN_CS = (8, 64, 72, 200)            # c % 8 == 0: the 16-byte path
BN_CS_RAGGED = (1, 12, 37)          # every element on its own (not for pcd_bn_batch_stats, which requires c % 8 == 0)


def column_names(c, rot):
    """Round robin: column j is of family (j + rot) % 15, so any 15 neighbouring columns hold every family (the two 8-column groups
    around a 64-column block boundary do), and over the rotations 8 i of bn_cases every family stands in the first and last group."""
    return [FAMILIES[(j + rot) % len(FAMILIES)] for j in range(c)]


def _column(name, m, g):
    r = torch.randn(m, generator=g, dtype=torch.float64)
    if name == "randn":
        return r
    if name.startswith("mean_"):
        return float(name[6:]) * (1 if name[5] == "p" else -1) + 0.7 * r
    if name == "tiny_spread":
        return 5 + 1e-4 * r
    if name in CONSTANT:
        return torch.full((m,), {"const": 3.25, "zero": 0.0, "const_beta0": 2.5, "const_beta_pos": -1.5, "const_beta_neg": 7.0}[name],
                          dtype=torch.float64)
    if name == "row0_outlier":           # the shift z[0] of the one-pass statistics is 8 sigma off the mean
        col = 30 + 0.7 * r
        col[0] = 30 + 8 * 0.7
        return col
    if name == "last_outlier":
        col = 30 + 0.7 * r
        col[m - 1] = 30 - 8 * 0.7
        return col
    if name == "spike":
        col = 0.01 * r
        col[m // 3] = 100.0
        return col
    assert name == "saturate"
    return r


def bn_pre64(z, mean, var, gamma, beta):
    """(t, y, rstd) in fp64 from whatever (mean, var) is handed in: t = (z - mean) * rstd * gamma, y = t + beta."""
    rstd = 1 / torch.sqrt(var.double() + EPS)
    t = (z.double() - mean.double()) * rstd * gamma.double()
    return t, t + beta.double(), rstd


def bn_stats64(z):
    """(mean, biased var) over the rows, fp64, two passes."""
    zd = z.double()
    mean = zd.mean(0)
    return mean, ((zd - mean) ** 2).mean(0)


def in_band(z, mean, var, gamma, beta, names, margin=MARGIN):
    """The elements a ReLU decision could go either way on: |y| < margin (|t| + |beta|), outside the exempt columns."""
    t, y, _ = bn_pre64(z, mean, var, gamma, beta)
    band = y.abs() < margin * (t.abs() + beta.double().abs())
    band[:, [n in EXEMPT for n in names]] = False
    return band


def bn_case(m, c, rot=0, seed=0):
    """One BatchNorm case: z fp32 [m][c] by column family, gamma / beta fp32 (every third gamma negative), the fp32 (mean, var) handed to
    apply and backward (the fp64 statistics of z, rounded), da fp16, running statistics.  No element is near the ReLU threshold."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * m + c)
    names = column_names(c, rot)
    gamma = (0.5 + torch.rand(c, generator=g, dtype=torch.float64)) * torch.where(torch.arange(c) % 3 == 2, -1.0, 1.0)
    beta = 0.3 * torch.randn(c, generator=g, dtype=torch.float64)
    z = torch.empty(m, c, dtype=torch.float64)
    for j, name in enumerate(names):
        z[:, j] = _column(name, m, g)
        if name == "saturate":
            gamma[j] = 4e4 * (1 if gamma[j] > 0 else -1)       # |y| reaches 1e5: the kernels must give +-65504
        if name.startswith("const_beta"):
            beta[j] = {"0": 0.0, "_pos": 0.25, "_neg": -0.25}[name[len("const_beta"):]]
    z, gamma, beta = z.float(), gamma.float(), beta.float()
    for it in range(40):
        mean64, var64 = bn_stats64(z)
        mean, var = mean64.float(), var64.float()
        band = in_band(z, mean, var, gamma, beta, names, 1.5 * MARGIN)
        if not band.any():
            break
        t, y, rstd = bn_pre64(z, mean, var, gamma, beta)
        b = beta.double().expand_as(y)
        push = torch.where(y >= 0, 1.0, -1.0) * 8e-3 * (it + 1) * b.abs()          # |t| ~ |beta| in the band: y -> 4e-3 (it + 1) of the scale
        znew = mean.double() + (push - b) / (rstd * gamma.double())
        z = torch.where(band, znew, z.double()).float()
    assert not band.any(), (m, c, rot, seed)
    da = (3 * torch.randn(m, c, generator=g)).half()
    rm, rv = torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    return dict(m=m, c=c, names=names, z=z, gamma=gamma, beta=beta, mean=mean, var=var, da=da, running_mean=rm, running_var=rv)


@functools.lru_cache(maxsize=None)
def bn_cases(c, seed=0):
    """The cases of one width, one per m of BN_MS; built once and shared (nobody writes into them)."""
    return tuple(bn_case(m, c, rot=8 * i, seed=seed) for i, m in enumerate(BN_MS))


# ------------------------------------------------------------------------------------------------------------ BatchNorm statements
def bn_stats_statement(z, running_mean=None, running_var=None):
    """pcd_bn_batch_stats in fp64 with its bounds: mean, biased var; running statistics as torch updates them (unbiased variance;
    at m = 1 the biased value, as the kernel documents)."""
    m, c = z.shape
    L = strip_chain(c, m)
    mean, var = bn_stats64(z)
    d = z.double() - z[0].double()
    out = dict(mean=mean, var=var, mean_bound=mean_bound(L, d.abs().sum(0), m, mean), var_bound=var_bound(L, (d * d).mean(0)))
    if running_mean is not None:
        mom = MOMENTUM
        unb = var * m / (m - 1) if m > 1 else var
        rm, rv = running_mean.double(), running_var.double()
        out["running_mean"] = (1 - mom) * rm + mom * mean
        out["running_var"] = (1 - mom) * rv + mom * unb
        out["running_mean_bound"] = mom * out["mean_bound"] + 4 * U32 * ((1 - mom) * rm.abs() + mom * mean.abs())
        unb_bound = (out["var_bound"] * m / (m - 1) + 2 * U32 * unb) if m > 1 else out["var_bound"]
        out["running_var_bound"] = mom * unb_bound + 4 * U32 * ((1 - mom) * rv.abs() + mom * unb)
    return out


K_APPLY, K_DZ, K_EXPAND, K_ENC1, K_SILU, K_SILU_BWD, K_GN, K_GN_DX = 8, 16, 4, 4, 4, 8, 4, 8


def bn_apply_statement(z, mean, var, gamma, beta, relu):
    """pcd_bn_apply_f16: (want, bound); want is not yet clamped and rounded."""
    t, y, _ = bn_pre64(z, mean, var, gamma, beta)
    want = y.clamp_min(0) if relu else y
    return want, half_bound(want, t.abs() + beta.double().abs(), K_APPLY)


def bn_backward_statement(da, z, mean, var, gamma, beta, relu):
    """dbeta, dgamma of pcd_bn_backward_f16 with their bounds, and what bn_dz_statement needs."""
    m, c = z.shape
    L = strip_chain(c, m)
    _, y, rstd = bn_pre64(z, mean, var, gamma, beta)
    xh = (z.double() - mean.double()) * rstd
    g = da.double() * (y > 0) if relu else da.double()
    return dict(dbeta=g.sum(0), dgamma=(g * xh).sum(0), dbeta_bound=sum_bound(L, g.abs().sum(0)),
                dgamma_bound=sum_bound(L, (g * xh).abs().sum(0)), g=g, xh=xh, rstd=rstd)


def bn_dz_statement(bw, gamma, dgamma, dbeta, m):
    """dz from the (dgamma, dbeta) handed in (the entry point's own fp32 output on the device): (want, bound)."""
    k = gamma.double() * bw["rstd"]
    kb, kg = dbeta.double() / m, dgamma.double() / m
    want = k * (bw["g"] - kb - bw["xh"] * kg)
    return want, half_bound(want, k.abs() * (bw["g"].abs() + kb.abs() + (bw["xh"] * kg).abs()), K_DZ)


def colsum_statement(x, rows_per_group, groups):
    c = x.shape[1]
    xd = x.double().reshape(groups, rows_per_group, c)
    return xd.sum(1), sum_bound(strip_chain(c, rows_per_group, groups), xd.abs().sum(1))


def vec3_outer_statement(mat, vec):
    """out[j][k] = sum_m vec[m][j] mat[m][k], vsum[j] = sum_m vec[m][j], with bounds."""
    m, k = mat.shape
    L = strip_chain(k, m)
    v, a = vec.double(), mat.double()
    return dict(out=v.t() @ a, out_bound=sum_bound(L, v.abs().t() @ a.abs()), vsum=v.sum(0), vsum_bound=sum_bound(L, v.abs().sum(0)))


def vec3_expand_statement(vec, w):
    v, wd = vec.double(), w.double()
    want = v @ wd
    return want, half_bound(want, v.abs() @ wd.abs(), K_EXPAND)


def enc1_statement(x, n_points, w, tbias):
    """z0[m][c] = sum_j x[m][j] w[c][j] + tbias[m // n_points][c]: (want, bound), fp32 output."""
    rows = torch.arange(x.shape[0]) // n_points
    tb = tbias.double()[rows]
    return x.double() @ w.double().t() + tb, K_ENC1 * U32 * (x.double().abs() @ w.double().abs().t() + tb.abs())


def colmax_statement(a, batch, n_points):
    """(max, FIRST index attaining it) per shape and column, as torch.max on the CPU gives them."""
    v = a.float().reshape(batch, n_points, -1)
    mx = v.max(1).values
    idx = torch.arange(n_points).reshape(1, -1, 1).expand_as(v)
    first = torch.where(v == mx.unsqueeze(1), idx, n_points).min(1).values
    return mx, first.int()


def maxpool_backward_statement(dg, arg, batch, n_points):
    c = dg.shape[1]
    da = torch.zeros(batch, n_points, c, dtype=torch.float16)
    da.scatter_(1, arg.long().unsqueeze(1), sat16(dg).unsqueeze(1))
    return da.reshape(batch * n_points, c)


def l1_statement(pred, target, scale):
    """(loss_sum, bound, dpred): dpred is exact, +-(float32(scale) / float32(n)) or 0."""
    n = pred.numel()
    d = pred.double() - target.double()
    gs = torch.tensor(scale, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    return d.abs().sum(), sum_bound(l1_chain(n), d.abs().sum()), torch.sign(d).float() * gs


def matmul_statement(a, b, trans_a, trans_b, bias, c_old):
    """C = (accumulate ? C : 0) + op(A) op(B) + bias: (want, sum of the term magnitudes); a, b are the logical stored matrices."""
    A = a.double().t() if trans_a else a.double()
    B = b.double().t() if trans_b else b.double()
    want, mag = A @ B, A.abs() @ B.abs()
    if bias is not None:
        want, mag = want + bias.double(), mag + bias.double().abs()
    if c_old is not None:
        want, mag = want + c_old.double(), mag + c_old.double().abs()
    return want, mag


def silu_statement(x):
    xd = x.double()
    y = xd * torch.sigmoid(xd)
    return y, K_SILU * U32 * y.abs() + xd.abs() / FLT_MAX


def silu_backward_statement(x, dy):
    xd, dyd = x.double(), dy.double()
    s = torch.sigmoid(xd)
    return dyd * s * (1 + xd * (1 - s)), K_SILU_BWD * U32 * dyd.abs() * s * (1 + xd.abs()) + dyd.abs() * (1 + xd.abs()) * (1 / FLT_MAX + 2.0 ** -149)


# ------------------------------------------------------------------------------------------------------------ GroupNorm
GN_SHAPES = ((3, 200, 2), (1, 64, 1), (5, 128, 8), (16, 4096, 8))


def _gn_pre64(x, mean, rstd, gamma, beta, groups):
    rows, c = x.shape
    xh = ((x.double().reshape(rows, groups, -1) - mean.double().unsqueeze(2)) * rstd.double().unsqueeze(2)).reshape(rows, c)
    t = xh * gamma.double()
    return xh, t, t + beta.double()


def gn_stats64(x, groups):
    rows, c = x.shape
    xg = x.double().reshape(rows, groups, -1)
    mean = xg.mean(2)
    var = ((xg - mean.unsqueeze(2)) ** 2).mean(2)
    return mean, var, 1 / torch.sqrt(var + EPS)


def gn_case(rows, c, groups, seed=0):
    """x fp32 [rows][c] with per-group offsets and scales, group 0 of the last row constant; gamma (mixed signs), beta; dy.  No element
    near the ReLU threshold (by the fp64 statistics: the kernel's own differ by 1e-6 of the scale, MARGIN is 1e-3)."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * rows + c + groups)
    gsz = c // groups
    x = torch.randn(rows, groups, gsz, generator=g, dtype=torch.float64)
    x = x * (0.1 + 3 * torch.rand(rows, groups, 1, generator=g, dtype=torch.float64)) + 20 * torch.randn(rows, groups, 1, generator=g, dtype=torch.float64)
    x[rows - 1, 0] = 4.75
    x = x.reshape(rows, c).float()
    gamma = ((0.5 + torch.rand(c, generator=g)) * torch.where(torch.arange(c) % 3 == 2, -1.0, 1.0)).float()
    beta = (0.3 * torch.randn(c, generator=g)).float()
    beta = torch.where(beta.abs() < 1e-3, torch.full_like(beta, 0.1), beta)
    for it in range(40):
        mean, var, rstd = gn_stats64(x, groups)
        _, t, y = _gn_pre64(x, mean, rstd, gamma, beta, groups)
        band = y.abs() < 1.5 * MARGIN * (t.abs() + beta.double().abs())
        if not band.any():
            break
        b = beta.double().expand_as(y)
        push = torch.where(y >= 0, 1.0, -1.0) * 8e-3 * (it + 1) * b.abs()
        k = (rstd.unsqueeze(2).expand(rows, groups, gsz).reshape(rows, c)) * gamma.double()
        xnew = mean.unsqueeze(2).expand(rows, groups, gsz).reshape(rows, c) + (push - b) / k
        x = torch.where(band, xnew, x.double()).float()
    assert not band.any(), (rows, c, groups)
    dy = torch.randn(rows, c, generator=g)
    return dict(rows=rows, c=c, groups=groups, x=x, gamma=gamma, beta=beta, dy=dy)


def gn_in_band(case, margin=MARGIN):
    mean, _, rstd = gn_stats64(case["x"], case["groups"])
    _, t, y = _gn_pre64(case["x"], mean, rstd, case["gamma"], case["beta"], case["groups"])
    return y.abs() < margin * (t.abs() + case["beta"].double().abs())


def gn_stats_statement(x, groups):
    """(mean, rstd) [rows][groups] in fp64 with bounds.  The kernel's variance is a second pass about its own fp32 mean: a mean off by
    e adds e^2 to it; rstd = (var + eps)^-1/2 moves by rstd^3 / 2 per unit of variance, and takes 3 u32 of its own (rsqrtf, argument)."""
    rows, c = x.shape
    gsz = c // groups
    L = ceil_div(gsz, 64) + 6
    mean, var, rstd = gn_stats64(x, groups)
    mb = sum_bound(L + 1, x.double().reshape(rows, groups, gsz).abs().sum(2)) / gsz + U32 * mean.abs()
    vb = sum_bound(L + 4, var * gsz) / gsz + 1.1 * mb * mb + 2 * U32 * var
    return dict(mean=mean, rstd=rstd, mean_bound=mb, rstd_bound=0.5 * rstd ** 3 * vb + 3 * U32 * rstd)


def gn_y_statement(x, mean, rstd, gamma, beta, groups, relu):
    """y from the (mean, rstd) handed in: (want, bound), fp32 output."""
    _, t, y = _gn_pre64(x, mean, rstd, gamma, beta, groups)
    return (y.clamp_min(0) if relu else y), K_GN * U32 * (t.abs() + beta.double().abs())


def gn_backward_statement(dy, x, mean, rstd, gamma, beta, groups, relu):
    """dx, dgamma, dbeta from the (mean, rstd) handed in, with bounds."""
    rows, c = x.shape
    gsz = c // groups
    L = ceil_div(gsz, 64) + 6
    xh, _, y = _gn_pre64(x, mean, rstd, gamma, beta, groups)
    g = dy.double() * (y > 0) if relu else dy.double()
    gg = g * gamma.double()
    grp = lambda t: t.reshape(rows, groups, gsz)
    s1, s2 = grp(gg).mean(2, keepdim=True), grp(gg * xh).mean(2, keepdim=True)
    e1 = sum_bound(L + 2, grp(gg).abs().sum(2, keepdim=True)) / gsz
    e2 = sum_bound(L + 5, grp(gg * xh).abs().sum(2, keepdim=True)) / gsz
    rs = rstd.double().unsqueeze(2)
    dx = rs * (grp(gg) - s1 - grp(xh) * s2)
    T = grp(gg).abs() + s1.abs() + (grp(xh) * s2).abs()
    dxb = rs * (K_GN_DX * U32 * T + e1 + grp(xh).abs() * e2)
    return dict(dx=dx.reshape(rows, c), dx_bound=dxb.reshape(rows, c), dgamma=(g * xh).sum(0), dbeta=g.sum(0),
                dgamma_bound=sum_bound(rows + 4, (g * xh).abs().sum(0)), dbeta_bound=sum_bound(rows, g.abs().sum(0)))


# ------------------------------------------------------------------------------------------------------------ AdamW
def adamw_statement(w, g, m1, m2, ema, lr, b1, b2, eps, wd, step, grad_scale, decay=0.0, fp32_corrections=True):
    """One step as adamw_element writes it, in fp64 from the fp32 arguments: returns (w, m1, m2, ema, bounds) with bounds a dict.
    The bias corrections are the host's fp32 1 - b^step (fp32_corrections) or exact (to compare with torch.optim.AdamW)."""
    lr, b1, b2, eps, wd, decay = (f32(v) for v in (lr, b1, b2, eps, wd, decay))
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    if fp32_corrections:
        bc1, bc2 = f32(bc1), f32(bc2)
    gr = g.double() * f32(1.0 / grad_scale)
    wd_ = w.double() * (1 - lr * wd)
    m = b1 * m1.double() + f32(1 - b1) * gr
    v = b2 * m2.double() + f32(1 - b2) * gr * gr
    wn = wd_ - (lr / bc1) * m / (torch.sqrt(v) / math.sqrt(bc2) + eps)
    en = decay * ema.double() + f32(1 - decay) * wn if ema is not None else None
    bounds = dict(w=4 * U32 * wn.abs() + 4 * U32 * lr, m1=4 * U32 * ((b1 * m1.double()).abs() + (f32(1 - b1) * gr).abs()),
                  m2=5 * U32 * ((b2 * m2.double()).abs() + f32(1 - b2) * gr * gr))
    if ema is not None:
        bounds["ema"] = bounds["w"] + 3 * U32 * ((decay * ema.double()).abs() + (f32(1 - decay) * wn).abs())
    return wn, m, v, en, bounds


def adamw_case(n, step, seed=0):
    """Parameters, scaled gradient (scale 64), moments with exp_avg_sq >= exp_avg^2 as a running mean of squares has (zero at step 1)."""
    g = torch.Generator().manual_seed(17 * seed + 3 * n + step)
    w, gr = torch.randn(n, generator=g), 64.0 * torch.randn(n, generator=g)
    if step == 1:
        m1, m2 = torch.zeros(n), torch.zeros(n)
    else:
        m1 = 0.3 * torch.randn(n, generator=g)
        m2 = m1 * m1 + 0.1 * torch.rand(n, generator=g)
    return dict(w=w, g=gr, m1=m1, m2=m2, ema=w + 0.01 * torch.randn(n, generator=g))


ADAMW_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, grad_scale=64.0, decay=0.999)


# ------------------------------------------------------------------------------------------------------------ fp32 statements, kernel order
def strip_sum32(T, rows_per_group, groups=1, drop_last_ragged_row=False, grid_cols=None):
    """Column sums of T fp32 [groups * rows_per_group][cols] in the column-strip kernels' order: a lane adds its rows (row0 + lane + 32 i)
    in order, the 32 lanes are added in order, the chunks in order.  drop_last_ragged_row is the mutant that loses the last row of a
    ragged last chunk.  grid_cols: the width that sets the launch geometry where it is not T's (pcd_vec3_outer's vsum)."""
    cols = T.shape[1]
    rpb, chunks = cr_grid(grid_cols or cols, rows_per_group, groups)
    T = T.reshape(groups, rows_per_group, cols)
    if drop_last_ragged_row and rows_per_group % rpb != 0:
        T = T.clone()
        T[:, -1] = 0
    pad = torch.zeros(groups, chunks * rpb, cols, dtype=torch.float32)
    pad[:, :rows_per_group] = T
    P = pad.reshape(groups, chunks, rpb // CR_LANES, CR_LANES, cols)
    lane = torch.zeros(groups, chunks, CR_LANES, cols, dtype=torch.float32)
    for i in range(rpb // CR_LANES):
        lane = lane + P[:, :, i]
    blk = torch.zeros(groups, chunks, cols, dtype=torch.float32)
    for r in range(CR_LANES):
        blk = blk + lane[:, :, r]
    out = torch.zeros(groups, cols, dtype=torch.float32)
    for y in range(chunks):
        out = out + blk[:, y]
    return out


def bn_stats32(z, unbiased_mutant=False, **mut):
    """pcd_bn_batch_stats' arithmetic: one pass, sums of d = z - z[0] and d^2 in the lane order, fp32 throughout."""
    m = z.shape[0]
    d = z - z[0]
    s1, s2 = strip_sum32(d, m, **mut)[0], strip_sum32(d * d, m, **mut)[0]
    fm = torch.tensor(float(m), dtype=torch.float32)
    d1 = s1 / fm
    var = (s2 / fm - d1 * d1).clamp_min(0)
    if unbiased_mutant and m > 1:
        var = var * fm / (fm - 1)
    return z[0] + d1, var


def bn_running32(mean, var, m, rm, rv):
    mom = torch.tensor(MOMENTUM, dtype=torch.float32)
    fm = torch.tensor(float(m), dtype=torch.float32)
    unb = var * fm / (fm - 1) if m > 1 else var
    return (1 - mom) * rm + mom * mean, (1 - mom) * rv + mom * unb


def bn_apply32(z, mean, var, gamma, beta, relu):
    y = (z - mean) * (torch.rsqrt(var + torch.tensor(EPS, dtype=torch.float32)) * gamma) + beta
    return sat16(y.clamp_min(0) if relu else y)


def bn_backward32(da, z, mean, var, gamma, beta, relu, ge_mutant=False, no_dgamma_mutant=False, zero_last_ragged_column=False, **mut):
    """pcd_bn_backward_f16's arithmetic: (dgamma, dbeta, dz).  Mutants: the mask with >= for >, dz without its dgamma / m term, the last
    column of a ragged 8-column group zeroed, and strip_sum32's."""
    m, c = z.shape
    rs = torch.rsqrt(var + torch.tensor(EPS, dtype=torch.float32))
    xh = (z - mean) * rs
    y = xh * gamma + beta
    g = da.float() * ((y >= 0) if ge_mutant else (y > 0)) if relu else da.float()
    dbeta, dgamma = strip_sum32(g, m, **mut)[0], strip_sum32(g * xh, m, **mut)[0]
    if zero_last_ragged_column and c % 8 != 0:
        dbeta[c - 1] = 0
        dgamma[c - 1] = 0
    inv_m = 1 / torch.tensor(float(m), dtype=torch.float32)
    kg = torch.zeros_like(dgamma) if no_dgamma_mutant else dgamma * inv_m
    return dgamma, dbeta, sat16(gamma * rs * (g - dbeta * inv_m - xh * kg))


def colsum32(x, rows_per_group, groups, zero_last_ragged_column=False, **mut):
    out = strip_sum32(x.float(), rows_per_group, groups, **mut)
    if zero_last_ragged_column and x.shape[1] % 8 != 0:
        out[:, -1] = 0
    return out


def vec3_outer32(mat, vec, **mut):
    m = mat.shape[0]
    a = mat.float()
    return torch.stack([strip_sum32(vec[:, j:j + 1] * a, m, **mut)[0] for j in range(3)]), strip_sum32(vec, m, grid_cols=mat.shape[1], **mut)[0]


def matmul32(a, b, trans_a, trans_b, bias, c_old, bias_per_block_mutant=False):
    """pcd_matmul_f32's arithmetic on the route it takes, fp32.  Mutant: the few-rows route for B [k][n] adds the bias in every k block."""
    A = (a.t() if trans_a else a).float()
    B = (b.t() if trans_b else b).float()
    m, k = A.shape
    n = B.shape[1]
    route = matmul_route(m, trans_a, trans_b)
    zero = torch.zeros(m, n, dtype=torch.float32)
    bz = bias if bias is not None else torch.zeros(n, dtype=torch.float32)
    if route == "generic":
        s = zero + bz
        for i in range(k):
            s = s + A[:, i:i + 1] * B[i:i + 1]
        return c_old + s if c_old is not None else s
    if route == "nn":
        s = c_old.clone() if c_old is not None else zero
        for y in range(ceil_div(k, 64)):
            acc = zero
            for i in range(64 * y, min(k, 64 * y + 64)):
                acc = acc + A[:, i:i + 1] * B[i:i + 1]
            s = s + (acc + bz if (y == 0 or bias_per_block_mutant) else acc)
        return s
    lanes = torch.zeros(64, m, n, dtype=torch.float32)
    for i in range(k):
        lanes[i % 64] = lanes[i % 64] + A[:, i:i + 1] * B[i:i + 1]
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ o]
    v = lanes[0] + bz
    return c_old + v if c_old is not None else v


def l1_32(pred, target):
    """pcd_l1_loss' sum: grid stride per lane, the block's 256 lanes by a halving tree, the blocks in index order (the atomic adds
    arrive in any order; this is one of them)."""
    n = pred.numel()
    blocks = l1_blocks(n)
    lanes = blocks * 256
    d = (pred - target).abs()
    pad = torch.zeros(ceil_div(n, lanes) * lanes, dtype=torch.float32)
    pad[:n] = d
    s = torch.zeros(lanes, dtype=torch.float32)
    for row in pad.reshape(-1, lanes):
        s = s + row
    red = s.reshape(blocks, 256)
    o = 128
    while o > 0:
        red = red[:, :o] + red[:, o:2 * o]
        o //= 2
    total = torch.zeros((), dtype=torch.float32)
    for v in red[:, 0]:
        total = total + v
    return total


def colmax32(a, batch, n_points, last_index_mutant=False):
    """pcd_colmax_argmax_f16's order: four row partitions (row % 4), then the partitions combined.  Mutant: ties keep the LAST index."""
    v = a.float().reshape(batch, n_points, -1)
    best = torch.full((batch, v.shape[2]), -float("inf"))
    bi = torch.zeros(batch, v.shape[2], dtype=torch.int32)
    for part in range(4):
        pb, pi = torch.full_like(best, -float("inf")), torch.zeros_like(bi)
        for r in range(part, n_points, 4):
            take = (v[:, r] >= pb) if last_index_mutant else (v[:, r] > pb)
            pb, pi = torch.where(take, v[:, r], pb), torch.where(take, torch.tensor(r, dtype=torch.int32), pi)
        if part == 0:
            best, bi = pb, pi
        else:
            take = (pb > best) | ((pb == best) & ((pi > bi) if last_index_mutant else (pi < bi)))
            best, bi = torch.where(take, pb, best), torch.where(take, pi, bi)
    return best, bi


def gn32(x, gamma, beta, groups, relu):
    """pcd_groupnorm_f32's arithmetic: lanes stride the group, butterfly sums, two passes: (y, mean, rstd)."""
    rows, c = x.shape
    gsz = c // groups
    steps = ceil_div(gsz, 64)
    idx = torch.arange(64)

    def wave_sum(t):                 # t [rows][groups][gsz]
        pad = torch.zeros(rows, groups, steps * 64, dtype=torch.float32)
        pad[:, :, :gsz] = t
        pad = pad.reshape(rows, groups, steps, 64)
        s = torch.zeros(rows, groups, 64, dtype=torch.float32)
        for i in range(steps):
            s = s + pad[:, :, i]
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, :, idx ^ o]
        return s[:, :, 0]
    xg = x.reshape(rows, groups, gsz)
    fg = torch.tensor(float(gsz), dtype=torch.float32)
    mu = wave_sum(xg) / fg
    d = xg - mu.unsqueeze(2)
    rs = torch.rsqrt(wave_sum(d * d) / fg + torch.tensor(EPS, dtype=torch.float32))
    y = (d * rs.unsqueeze(2)).reshape(rows, c) * gamma + beta
    return (y.clamp_min(0) if relu else y), mu, rs


def gn_backward32(dy, x, mean, rstd, gamma, beta, groups, relu):
    rows, c = x.shape
    gsz = c // groups
    xh = ((x.reshape(rows, groups, gsz) - mean.unsqueeze(2)) * rstd.unsqueeze(2)).reshape(rows, c)
    mask = (xh * gamma + beta > 0) if relu else torch.ones_like(xh, dtype=torch.bool)
    g = dy * mask
    gg = (dy * gamma) * mask
    fg = torch.tensor(float(gsz), dtype=torch.float32)
    s1 = gg.reshape(rows, groups, gsz).sum(2, keepdim=True) / fg
    s2 = (gg * xh).reshape(rows, groups, gsz).sum(2, keepdim=True) / fg
    dx = rstd.unsqueeze(2) * (gg.reshape(rows, groups, gsz) - s1 - xh.reshape(rows, groups, gsz) * s2)
    dgamma, dbeta = torch.zeros(c), torch.zeros(c)
    for r in range(rows):
        dgamma, dbeta = dgamma + g[r] * xh[r], dbeta + g[r]
    return dx.reshape(rows, c), dgamma, dbeta


def adamw32(w, g, m1, m2, ema, lr, b1, b2, eps, wd, step, grad_scale, decay=0.0):
    """adamw_element in fp32: every product and sum rounded, the two fused multiply-adds formed exactly in fp64 and rounded once."""
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    lr, b1, b2, eps, wd, decay = (t(v) for v in (lr, b1, b2, eps, wd, decay))
    bc1, bc2 = t(1 - float(b1) ** step), t(1 - float(b2) ** step)
    gr = g * t(1.0 / grad_scale)
    wn = ((-(lr * wd)).double() * w.double() + w.double()).float()
    m = b1 * m1 + (1 - b1) * gr
    v = b2 * m2 + (1 - b2) * gr * gr
    wn = wn - (lr / bc1) * m / (torch.sqrt(v) / torch.sqrt(bc2) + eps)
    en = (decay.double() * ema.double() + ((1 - decay) * wn).double()).float() if ema is not None else None
    return wn, m, v, en


# ------------------------------------------------------------------------------------------------------------ the other cases
COLSUM_GROUPS, COLSUM_ROWS = (1, 3), (1, 127, 128, 129, 500)
VEC3_KS = (8, 64, 72)                       # 64 is the width the trainers pass
COLMAX_NS, COLMAX_CS, COLMAX_BATCHES = (1, 2, 3, 4, 5, 257), (1, 63, 64, 65, 130), (1, 3)
TRANSPOSE_SIZES = (1, 7, 8, 63, 64, 65, 72)
MATMUL_MS, MATMUL_KS, MATMUL_NS = (1, 32, 33), (1, 63, 64, 65, 300), (1, 70, 255, 256, 257)
L1_NS = (1, 255, 257, 262144 + 257)
ADAMW_NS, ADAMW_STEPS = (1, 3, 4, 1003), (1, 100000)


def family_matrix(rows, c, rot, g):
    """fp16 [rows][c] by column family (for the kernels that read fp16 activations), and the column names."""
    names = column_names(c, rot)
    return torch.stack([_column(n, rows, g) for n in names], dim=1).half(), names


def colsum_case(rows_per_group, groups, c, seed=0):
    g = torch.Generator().manual_seed(7 * seed + 1000 * rows_per_group + 10 * c + groups)
    return family_matrix(rows_per_group * groups, c, 8 * COLSUM_ROWS.index(rows_per_group) + groups, g)


def vec3_case(m, k, seed=0):
    """mat fp16 [m][k] by column family, vec fp32 [m][3] with one column far from zero and one tiny."""
    g = torch.Generator().manual_seed(11 * seed + 1000 * m + k)
    mat, names = family_matrix(m, k, 8 * BN_MS.index(m), g)
    vec = torch.randn(m, 3, generator=g) * torch.tensor([1.0, 0.7, 1e-3]) + torch.tensor([0.0, 30.0, 0.0])
    return mat, vec, names


def expand_case(m, k, seed=0):
    """vec fp32 [m][3], w fp32 [3][k]; column 0 of w large enough that vec3_expand saturates on some rows."""
    g = torch.Generator().manual_seed(13 * seed + 1000 * m + k)
    vec, w = torch.randn(m, 3, generator=g), torch.randn(3, k, generator=g)
    w[:, 0] *= 1e5
    return vec, w


def enc1_case(m, n_points, c1, seed=0):
    g = torch.Generator().manual_seed(19 * seed + 1000 * m + 10 * n_points + c1)
    return torch.randn(m, 3, generator=g), torch.randn(c1, 3, generator=g), torch.randn(ceil_div(m, n_points), c1, generator=g)


def colmax_case(batch, n_points, c, seed=0):
    """fp16 [batch * n_points][c] of small integers (many exact ties); column 0 all equal, column 1 all -inf, column 2 with its maximum in
    rows 1 and 4 (two row partitions, the later row in the earlier partition), column 3 with it in the first and the last row."""
    g = torch.Generator().manual_seed(23 * seed + 1000 * n_points + 10 * c + batch)
    a = (torch.randint(0, 5, (batch, n_points, c), generator=g) - 2).float()
    a[:, :, 0] = 2.0
    if c > 1:
        a[:, :, 1] = -float("inf")
    if c > 2 and n_points >= 5:
        a[:, 1, 2] = 9.0
        a[:, 4, 2] = 9.0
    if c > 3:
        a[:, 0, 3] = 9.0
        a[:, n_points - 1, 3] = 9.0
    dg = torch.randn(batch, c, generator=g)
    dg[:, 0] = 1e6                          # the scatter saturates
    return a.reshape(batch * n_points, c).half(), dg


def matmul_case(m, k, n, seed=0):
    g = torch.Generator().manual_seed(29 * seed + 100000 * m + 1000 * k + n)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(a=rn(m, k), b=rn(k, n), bias=rn(n), c_old=rn(m, n))


def l1_case(n, seed=0):
    g = torch.Generator().manual_seed(31 * seed + n)
    pred, target = torch.randn(n, generator=g), torch.randn(n, generator=g)
    pred[::7] = target[::7]                 # exact zeros: sign(0) = 0
    return pred, target


def silu_case(seed=0):
    g = torch.Generator().manual_seed(37 + seed)
    x = torch.cat([torch.linspace(-90, 90, 1001), torch.tensor([0.0, -0.0, -90.0, 90.0, -88.8, -88.7, 88.7, -87.0, 1e-30, -1e-30])])
    return x, torch.randn(x.numel(), generator=g)
