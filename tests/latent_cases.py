"""Cases, fp64 statements, fp32 statements in the kernels' order, and derived error bounds for the latent denoiser's kernels: csrc/skinny.hip,
csrc/latent.hip and csrc/latent_persist.hip.  Shared by tests/test_latent_cases_cpu.py (which holds this file to account on the CPU) and
tests/test_gpu_latent_kernels.py (which judges every launch against it: slab by slab, (row, group) by (row, group), row by row).  Plain torch on
the CPU, seeded CPU generators, float64 arithmetic; nothing of the library is imported here (the callers hand in packed weights).  u32, u16,
sum_bound, half_bound, the column families and gn_case are tests/train_cases.py's (imported, not copied).

LAUNCH GEOMETRY, restated from csrc/skinny.hip (tests/test_latent_cases_cpu.py checks it against the library's host functions).
  split-K GEMM: a block owns 32 columns and a K slice of ks = pick_ks(k, c): 512, halved while above 256 and (c / 32) * (k / ks) < 256, then halved
      until it divides k; k / ks slabs.  The slice's 64-deep chunks are dealt round-robin to four waves, a wave's chunks run in sequence through one
      accumulator, then (r0 + r1) + (r2 + r3): the longest chain of a slab element is gemm_chain = 64 * ceil((ks / 64) / 4) + 2.
  fused layer: a workgroup owns bc = max(gsz, 32) columns in mode 0 (32 in modes 1 and 2) = CT = bc / 32 column tiles, and its 16 waves are CT tiles x
      KSPLIT = 16 / CT splits of the full K; chunk ch goes to split ch % KSPLIT; the splits are added in order, then bias + row bias (one value):
      fused_chain = 64 * ceil(chunks / KSPLIT) + KSPLIT + 2.  GroupNorm sums there: CT values per thread, then log2(gsz / CT) <= 5 butterfly steps.
  pcd_skinny_finish: one block of 256 threads per (row, split), split = groups in mode 0, else 8 if c % 8 == 0 and 1 if not.  Pre-activation: bias,
      + row bias, + the slabs in slab order (nslabs + 1 additions).  GroupNorm sums: a thread's stride ceil(gsz / 256), 6 butterfly steps, the four
      waves as (w0 + w1) + (w2 + w3): finish_gn_chain = ceil(gsz / 256) + 6 + 2.
  groupnorm_relu_kernel (csrc/latent.hip): one wave per group: gn_chain = ceil(gsz / 64) + 6, the chain of train_cases' GroupNorm.

STATEMENTS.
  slabs.  fp16 x fp16 products are exact in fp32, so only the additions round: slab s of the GEMM lies within sum_bound(gemm_chain, sum |a| |w|)
      of the fp64 dot over ITS slice (slab_statement), both sums over k in [s ks, (s + 1) ks).  On small integers (|a|, |w| <= 3: every partial sum
      below 5120 * 9 < 2^24) every order of additions is exact and the device must equal the fp64 slice sum bit for bit: that pins each k to its slab.
  finish32.  bias, + row bias, + slabs in slab order, all fp32 additions (nothing a compiler can contract); mode 2 stores that, mode 1 stores
      sat16(max(v, 0)).  No rounding is left to chance: the device must agree with finish32 BITWISE in modes 1 and 2.  Mode 0 is then judged from
      finish32's pre-activation, which is bitwise the kernel's: the split-K sum's error does not enter the GroupNorm comparison (each stage is fed
      its predecessor's own fp32 output).
  GroupNorm + ReLU (finish mode 0 with L = finish_gn_chain, pcd_groupnorm_relu_f16 with L = gn_chain, the fused kernel with L = CT + 6), gn_relu_statement.
      The kernels do not return (mean, rstd), so their error is carried into the output bound, with train_cases.gn_stats_statement's derivation:
        mean within mb = sum_bound(L + 1, sum |x|) / gsz + u32 |mean|          (the sum, the division)
        var  within vb = sum_bound(L + 4, gsz var) / gsz + 1.1 mb^2 + 2 u32 var  (second pass about the kernel's own mean; d * d carries 3 roundings)
        rstd within rb = rstd^3 vb / 2 + 3 u32 rstd                             (rsqrtf 1 ulp, its argument)
      y = (x - mean) * rstd * gamma + beta then moves by at most |gamma| (rstd mb + |x - mean| rb), plus its own K = 4 roundings (subtraction, two
      products, addition; counted as train_cases counts pcd_groupnorm_f32's y) on S = |t| + |beta|.  ReLU is 1-Lipschitz, so the bound on y is a
      bound behind the ReLU whichever side of zero either value falls: no margin is needed for the forward output (the gn_case data keep train_cases'
      "no element near the threshold" rule all the same, and the CPU module asserts it).  The fp16 store rounds the kernel's fp32 value v, |v| <=
      |want| + ybound: out within ybound + u16 (min(|want|, 65504) + ybound) + 2^-25 = half_bound(want, S, 4) + the statistics' terms + u16 ybound.
      Beyond 65504 + ybound the output is 65504 exactly, never inf.
  the fused kernel, mode 0.  Its pre-activation z is not returned, so the GEMM's error enters GroupNorm: d_i = sum_bound(fused_chain, sum |a| |w| +
      |bias| + |row_bias|), propagated to first order (xhat_i = (z_i - mean) rstd; a perturbation e of z moves mean by mean(e), the variance by
      2 mean((z - mean) e), so xhat_i by rstd (e_i - mean(e) - xhat_i mean(xhat e))):
        |dy_i| <= 1.1 |gamma_i| rstd (d_i + mean(d) + |xhat_i| mean(|xhat| d))
      on top of the GroupNorm terms above.  The factor 1.1 covers the second order only where max(d) rstd <= 0.05: a condition on the INPUTS that the
      CPU module asserts for every fused case; it is not a tolerance.  Where z is exact in fp32 (integers; zero activations under a row bias
      alone, z = row_bias) d is 0.  Modes 1 and 2: z within d, then the fp16 rounding.
  the whole network, network(): the packed fp16 weights, the hoisted time row, fp32 z rounded to fp16 on load (sat16), every activation rounded with
      sat16 where the kernels store fp16 (after each GroupNorm + ReLU and after output.0's ReLU), the skip halves concatenated as csrc/latent.hip does
      ([g1 | z4], [d | z3], [d | z2], [d | z1]), eps in the working precision.  ddim(): n steps around it with pcd_ddim_update's operation order
      (include/pcd_hip.h): x0 = (z - n * eps) / s; z = s2 * x0 + n2 * eps.  dtype float64 is the statement; float32 with the three summation orders of
      ORDERS (torch's own, K reversed, 64-deep chunks dealt to four accumulators) are its fp32 twins: correct code in three different orders.
      Judged per row r: E_abs = max_r max_j |err_rj| / max_j |want_rj| and E_l2 = max_r |err_r|_2 / |want_r|_2, and the same per column.  The bounds
      for the device are 3 x the largest figure over the three twins, computed when a test runs (network_figures, bounds_from), never hard-coded: the errors are
      discrete fp16 rounding flips, the kernel's order is one more draw from the population the three orders are drawn from, and over 192 row
      samples the largest row stood at 2.2 x the median.  Per column only from 31 rows up: in a single row a column's scale is one element, which may
      be as near zero as it likes.

CASES: the smallest that reach each path (GEMM_MS, GEMM_SHAPES, FINISH_*, GN_*, FUSED_*; what each reaches stands beside it).  Every GEMM shape also
runs with ldw = k + 8, the gap columns holding fp16 NaN.  Two kinds of data per case: small integers (exact), and the train_cases families set
through the free operands: for finish and pcd_groupnorm_relu_f16 one family per (row, group) over the group's channels (gn_family_case), for the
fused kernel the same matrix as row_bias over zero activations, and a per-group bias of +-30 / +-1000 over a randn product.  In every family case
gamma of channel 1 is 1e6: that channel's pre-activation passes 65504 and must come out as 65504.  nonfinite_rows() puts an inf and a NaN into one
(row, group); every other (row, group) must come out bitwise as without them.  Buffers carry GUARD NaN elements past their end (guarded / guard_ok).

MEASURED on the CPU (tests/test_latent_cases_cpu.py prints them): the fp32 statement in the kernels' order against the fp64 statement, largest
error / bound over every case.  Slabs: 0.10 (0.014 at k = 5120).  GroupNorm outputs: finish mode 0 0.995, pcd_groupnorm_relu_f16 0.98, fused mode 0
0.995 where z is exact and 0.67 on the randn product, fused modes 1 / 2 0.975.  The figures near 1 are the fp16 store alone: half an fp16 ulp is
u16 |v| exactly when v stands just above a power of two, so an element whose fp32 value falls near a tie there uses all of u16 |want|, which is
most of its bound; the statistics' terms are what a wrong kernel exceeds (the mutants leave by more than 10 x), not what a right one approaches.
No ratio exceeded 1 and no derivation was changed after measuring.  max(d) rstd over the fused cases: 1.1e-2 (condition: 0.05).
Whole network at B = 64 (weights helpers.latent_sd(), z = latent_input(64), t = 0.73), largest over the three orders, rows / columns: forward E_abs
1.04e-3 / 1.78e-3, E_l2 8.9e-4 / 1.07e-3; 1 DDIM step (ddim_tables) on x0 E_abs 5.1e-4 / 6.0e-4, E_l2 4.4e-4 / 3.8e-4; 4 steps E_abs 3.5e-4 / 4.2e-4,
E_l2 3.5e-4 / 3.2e-4 (the update divides eps' error by the state's scale).  These figures are copied from a run; the tests compute them afresh."""
import functools
import math

import torch

import train_cases as T
from train_cases import U16, U32, F16_MAX, EPS, ceil_div, sat16, sum_bound, half_bound

GUARD = 64
NAN = float("nan")
K_GN = T.K_GN


# ------------------------------------------------------------------------------------------------------------ launch geometry
def pick_ks(k, c):
    ks = 512
    while ks > 256 and (c // 32) * (k // ks) < 256:
        ks >>= 1
    while k % ks:
        ks >>= 1
    return ks


def slab_count(k, c):
    return 0 if k <= 0 or c <= 0 or k % 64 else k // pick_ks(k, c)


def gemm_chain(k, c):
    return 64 * ceil_div(pick_ks(k, c) // 64, 4) + 2


def fused_supported(k, c, mode, groups):
    if k <= 0 or c <= 0 or k % 64 or mode not in (0, 1, 2) or k * c > 768 * 256:
        return False
    if mode == 0:
        return groups > 0 and c % groups == 0 and c // groups in (16, 32, 64, 128)
    return c % 32 == 0


def fused_tiles(c, mode, groups):
    """(bc, CT, KSPLIT)"""
    bc = max(c // groups, 32) if mode == 0 else 32
    return bc, bc // 32, 16 // (bc // 32)


def fused_chain(k, c, mode, groups):
    _, _, ksplit = fused_tiles(c, mode, groups)
    return 64 * ceil_div(k // 64, ksplit) + ksplit + 2


def finish_split(c, mode, groups):
    return groups if mode == 0 else (8 if c % 8 == 0 else 1)


def finish_gn_chain(gsz):
    return ceil_div(gsz, 256) + 6 + 2


def gn_chain(gsz):
    return ceil_div(gsz, 64) + 6


# ------------------------------------------------------------------------------------------------------------ judging
def ratio(err, bound):
    """err / bound element by element, with 0 / 0 = 0, x / 0 = inf and NaN = inf."""
    err = torch.nan_to_num(torch.as_tensor(err, dtype=torch.float64), nan=float("inf"), posinf=float("inf"))
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    return torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def out16_error(got, want):
    """|got - want| of an fp16 output against the fp64 statement clamped to +-65504 (the kernels saturate)."""
    return (got.double() - want.double().clamp(-F16_MAX, F16_MAX)).abs()


def first_bad(r, groups=None):
    """(row, group, channel) of the first element with ratio > 1, or None."""
    bad = (r > 1).nonzero()
    if not len(bad):
        return None
    row, ch = bad[0].tolist()[-2:] if r.dim() >= 2 else (0, bad[0].item())
    return row, (ch // (r.shape[-1] // groups) if groups else None), ch


# ------------------------------------------------------------------------------------------------------------ cases
GEMM_MS = (1, 31, 32, 33, 64, 65, 129, 256)
GEMM_SHAPES = ((64, 0, 32),            # one chunk, three idle waves
               (192, 0, 64),           # ks = 64
               (320, 64, 48),          # ks = 128; the source changes inside slice 2; c % 32 != 0
               (64, 192, 128),         # the source changes inside a wave's chunk sequence
               (1024, 0, 2048),        # ks = 256, 4 slabs
               (4096, 1024, 1024),     # ks = 512, 10 slabs; the 64 KiB LDS-DMA limit (m <= 32 only)
               (256, 0, 8))            # c < 32
GEMM_F32IN_MS = (31, 33, 65, 256)      # one m per kernel instantiation: 1, 2, 4 (3 row tiles) and 8 row tiles
FINISH_NSLABS = (1, 2, 3, 4, 5, 10)
FINISH_SHAPES = ((128, 8), (200, 2), (1024, 1), (4096, 8), (12, 1))       # (c, groups); (12, 1) for modes 1 and 2 only
FINISH_ROWS = 3
GN_GROUPS, GN_GSZ = (1, 2, 3, 5, 8), (16, 100, 512)
GN_ROWS = 3
FUSED_MS = (1, 31, 33, 64, 255, 256)
FUSED_SHAPES = ((64, 0, 48, 3),        # CT = 1, gsz 16, last workgroup half empty
                (192, 0, 256, 8),      # CT = 1, 3 chunks over 16 splits
                (256, 64, 512, 8),     # CT = 2, 5 chunks over 8 splits, two sources
                (128, 0, 1024, 8))     # CT = 4
FUSED_PLAIN = (128, 0, 128)            # modes 1 and 2


def gemm_ms(k1, k2, c):
    return tuple(m for m in GEMM_MS if m <= 32) if (k1, k2, c) == (4096, 1024, 1024) else GEMM_MS


def _gen(*key):
    seed = 17
    for v in key:
        seed = (seed * 1000003 + int(v) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def guarded(t, fill=None):
    """A flat buffer holding t (or `fill` in t's shape) followed by GUARD NaN elements (fp16 / fp32)."""
    buf = torch.full((t.numel() + GUARD,), NAN, dtype=t.dtype)
    buf[:t.numel()] = t.reshape(-1) if fill is None else fill
    return buf


def guard_ok(buf, n):
    return bool(torch.isnan(buf.reshape(-1)[n:]).all()) and buf.numel() == n + GUARD


def pad_ldw(w, ldw):
    """w [c][k] -> [c][ldw], the gap columns fp16 NaN."""
    out = torch.full((w.shape[0], ldw), NAN, dtype=w.dtype)
    out[:, :w.shape[1]] = w
    return out


@functools.lru_cache(maxsize=None)
def gemm_case(m, k1, k2, c, kind):
    """a1 [m][k1], a2 [m][k2] or None, w [c][k1 + k2], fp16.  kind "int": integers in [-3, 3]; "fam": activations by train_cases' column
    families over k (a mean of +-1000 in a column is a weight row's worth of cancellation for the sum), weights randn / sqrt(k)."""
    g = _gen(m, k1, k2, c, kind == "int")
    k = k1 + k2
    if kind == "int":
        a = torch.randint(-3, 4, (m, k), generator=g).half()
        w = torch.randint(-3, 4, (c, k), generator=g).half()
    else:
        a, _ = T.family_matrix(m, k, m % 15, g)
        w = (torch.randn(c, k, generator=g) / math.sqrt(k)).half()
    return dict(a1=a[:, :k1].contiguous(), a2=a[:, k1:].contiguous() if k2 else None, w=w, a=a)


def concat_sources(a1, a2, k1_stride_mutant=False):
    """[a1 | a2]; the mutant reads the second source with k1 as its row stride (inside its own storage)."""
    if a2 is None:
        return a1
    if k1_stride_mutant:
        m, k2 = a2.shape
        flat = a2.reshape(-1)
        idx = (torch.arange(m).unsqueeze(1) * a1.shape[1] + torch.arange(k2).unsqueeze(0)) % flat.numel()
        a2 = flat[idx]
    return torch.cat([a1, a2], 1)


def slab_of_k(k, c, shift_chunks=0):
    """The slab every k belongs to; shift_chunks moves every inner slice boundary (the mutant)."""
    ks = pick_ks(k, c)
    return ((torch.arange(k) - 64 * shift_chunks).clamp_min(0) // ks).clamp_max(k // ks - 1)


def slab_statement(a, w, c, shift_chunks=0):
    """(want [S][m][c] fp64, bound): the fp64 dot over each slab's own K slice."""
    k = a.shape[1]
    sk = slab_of_k(k, c, shift_chunks)
    A, W = a.double(), w.double()[:, :k]
    S = k // pick_ks(k, c)
    want = torch.stack([A[:, sk == s] @ W[:, sk == s].t() for s in range(S)])
    mag = torch.stack([A[:, sk == s].abs() @ W[:, sk == s].abs().t() for s in range(S)])
    return want, sum_bound(gemm_chain(k, c), mag)


def slabs32(a, w, c):
    """The split-K GEMM in fp32 in the kernel's order: per slab four wave accumulators, a wave's chunks (wave, wave + 4, ..) in sequence and k in
    sequence inside a chunk, then (r0 + r1) + (r2 + r3)."""
    m, k = a.shape
    ks = pick_ks(k, c)
    S, nch = k // ks, ks // 64
    A, W = a.float(), w.float()[:, :k]
    acc = torch.zeros(S, 4, m, c, dtype=torch.float32)
    base = (torch.arange(S) * ks).unsqueeze(1) + 64 * torch.arange(4).unsqueeze(0)          # [S][4]: first k of wave's first chunk
    for i in range(ceil_div(nch, 4)):
        live = ((torch.arange(4) + 4 * i) < nch).float().reshape(1, 4, 1, 1)
        for e in range(64):
            kk = (base + 256 * i + e).clamp_max(k - 1).reshape(-1)
            acc = acc + live * (A[:, kk].t().reshape(S, 4, m, 1) * W[:, kk].t().reshape(S, 4, 1, c))
    return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])


# ------------------------------------------------------------------------------------------------------------ finish
def finish32(slabs, bias, row_bias, mode, drop_last_of_4k1=False, no_relu=False, overflow_inf=False, pre=False):
    """pcd_skinny_finish in fp32, the kernel's order.  pre: the pre-activation (what mode 0 normalises).  Mutants: the last slab dropped when
    nslabs % 4 == 1, ReLU missing in mode 1, fp16 overflow to inf."""
    S = slabs.shape[0]
    v = torch.zeros_like(slabs[0]) if bias is None else bias.float().expand_as(slabs[0]).clone()
    if row_bias is not None:
        v = v + row_bias
    for s in range(S - 1 if (drop_last_of_4k1 and S % 4 == 1) else S):
        v = v + slabs[s]
    if mode == 2 or pre:
        return v
    if not no_relu:
        v = torch.where(v > 0, v, torch.zeros_like(v))                     # fmaxf(NaN, 0) = 0, as the kernel's
    return v.half() if overflow_inf else sat16(v)


def gn_relu_statement(x, gamma, beta, groups, L, d=None):
    """GroupNorm(groups) + affine + ReLU -> fp16 of x [rows][c] (fp32 or fp64: the kernel's own pre-activation, or the fp64 one with its error
    bound d [rows][c]): (want fp64, not yet clamped and rounded; bound).  See the module docstring."""
    rows, c = x.shape
    gsz = c // groups
    grp = lambda t: t.reshape(rows, groups, gsz)
    xd, ga, be = x.double(), gamma.double(), beta.double()
    mean, var, rstd = T.gn_stats64(xd, groups)
    mb = sum_bound(L + 1, grp(xd).abs().sum(2)) / gsz + U32 * mean.abs()
    vb = sum_bound(L + 4, var * gsz) / gsz + 1.1 * mb * mb + 2 * U32 * var
    rb = 0.5 * rstd ** 3 * vb + 3 * U32 * rstd
    dev = grp(xd) - mean.unsqueeze(2)
    xh = dev * rstd.unsqueeze(2)
    t = xh.reshape(rows, c) * ga
    y = t + be
    yb = K_GN * U32 * (t.abs() + be.abs()) + ga.abs() * (rstd.unsqueeze(2) * mb.unsqueeze(2) + dev.abs() * rb.unsqueeze(2)).reshape(rows, c)
    if d is not None:
        dd = grp(torch.as_tensor(d, dtype=torch.float64).expand(rows, c))
        prop = rstd.unsqueeze(2) * (dd + dd.mean(2, keepdim=True) + xh.abs() * (xh.abs() * dd).mean(2, keepdim=True))
        yb = yb + 1.1 * ga.abs() * prop.reshape(rows, c)
    want = y.clamp_min(0)
    return want, yb + U16 * (want.clamp(max=F16_MAX) + yb) + 2.0 ** -25


def first_order_ok(x, groups, d):
    """The condition on the inputs under which gn_relu_statement's d term holds: max(d) rstd <= 0.05 in every (row, group)."""
    rows, c = x.shape
    _, _, rstd = T.gn_stats64(x.double(), groups)
    dd = torch.as_tensor(d, dtype=torch.float64).expand(rows, c).reshape(rows, groups, -1)
    return float((dd.max(2).values * rstd).max())


def gn32(x, gamma, beta, groups, chain, unbiased=False, no_eps=False, one_pass=False, wide_stats=False, gamma_wrap=False, overflow_inf=False):
    """GroupNorm + ReLU -> fp16 in fp32 in a kernel's order.  chain: "finish" (256 threads stride the group, butterfly, (w0 + w1) + (w2 + w3)), "wave"
    (64 lanes stride it, butterfly: groupnorm_relu_kernel), or an int CT (the fused kernel: CT values per thread, butterfly over gsz / CT threads).
    Mutants: unbiased variance, eps left out, one-pass variance E[x^2] - mean^2, a group's statistics taken over 32 channels where gsz = 16, gamma of
    channel i >= 512 read from channel i - 512, fp16 overflow to inf."""
    rows, c = x.shape
    gsz = c // groups
    x = x.float()
    xg = x.reshape(rows, groups, gsz)

    def gsum(t):                                      # t [rows][G][n] -> [rows][G]
        n = t.shape[2]
        if chain == "finish":
            lanes, waves = 256, 4
        elif chain == "wave":
            lanes, waves = 64, 1
        else:
            lanes, waves = max(n // chain, 1), 0
        if waves == 0:                                # fused: thread p holds channels p CT .. p CT + CT - 1
            s = torch.zeros(t.shape[0], t.shape[1], lanes, dtype=torch.float32)
            tt = t.reshape(t.shape[0], t.shape[1], lanes, -1)
            for i in range(tt.shape[3]):
                s = s + tt[..., i]
            o, idx = 1, torch.arange(lanes)
            while o < lanes:
                s = s + s[..., idx ^ o]
                o <<= 1
            return s[..., 0]
        steps = ceil_div(n, lanes)
        pad = torch.zeros(t.shape[0], t.shape[1], steps * lanes, dtype=torch.float32)
        pad[..., :n] = t
        pad = pad.reshape(t.shape[0], t.shape[1], steps, lanes)
        s = torch.zeros(t.shape[0], t.shape[1], lanes, dtype=torch.float32)
        for i in range(steps):
            s = s + pad[:, :, i]
        s = s.reshape(t.shape[0], t.shape[1], waves, 64)
        idx = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[..., idx ^ o]
        s = s[..., 0]
        return (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3]) if waves == 4 else s[..., 0]

    if wide_stats and gsz == 16:                      # pairs of groups share their statistics (an odd last group pairs with zeros)
        pairs = ceil_div(groups, 2)
        xs = torch.zeros(rows, pairs * 32, dtype=torch.float32)
        xs[:, :c] = x
        xs = xs.reshape(rows, pairs, 32)
        n = torch.tensor(32.0)
        mu = gsum(xs) / n
        dv = xs - mu.unsqueeze(2)
        va = gsum(dv * dv) / n
        mu, va = mu.repeat_interleave(2, 1)[:, :groups], va.repeat_interleave(2, 1)[:, :groups]
    else:
        n = torch.tensor(float(gsz))
        mu = gsum(xg) / n
        dv = xg - mu.unsqueeze(2)
        va = gsum(xg * xg) / n - mu * mu if one_pass else gsum(dv * dv) / n
        if unbiased:
            va = va * n / (n - 1)
    rs = torch.rsqrt(va if no_eps else va + torch.tensor(EPS, dtype=torch.float32))
    ga = gamma.float()
    if gamma_wrap:
        ch = torch.arange(c)
        ga = ga[torch.where(ch % gsz >= 512, ch - 512, ch)]
    y = ((xg - mu.unsqueeze(2)) * rs.unsqueeze(2)).reshape(rows, c) * ga + beta.float()
    y = torch.where(y > 0, y, torch.zeros_like(y))                         # fmaxf(NaN, 0) = 0, as the kernels'
    return y.half() if overflow_inf else sat16(y)


def group_names(rows, groups, rot):
    """The family of every (row, group), round robin over train_cases.FAMILIES."""
    return [[T.FAMILIES[(r * groups + g + rot) % len(T.FAMILIES)] for g in range(groups)] for r in range(rows)]


@functools.lru_cache(maxsize=None)
def gn_family_case(rows, c, groups, rot=0):
    """x fp32 [rows][c], one train_cases family per (row, group) over the group's channels; gamma (mixed signs; channel 1: 1e6, which saturates wherever xhat > 0.07),
    beta.  `names` [rows][groups]."""
    g = _gen(rows, c, groups, rot)
    gsz = c // groups
    names = group_names(rows, groups, rot)
    x = torch.stack([torch.cat([T._column(names[r][q], gsz, g) for q in range(groups)]) for r in range(rows)]).float()
    gamma = ((0.5 + torch.rand(c, generator=g)) * torch.where(torch.arange(c) % 3 == 2, -1.0, 1.0)).float()
    if c > 1:
        gamma[1] = 1e6
    beta = (0.3 * torch.randn(c, generator=g)).float()
    return dict(rows=rows, c=c, groups=groups, x=x, gamma=gamma, beta=beta, names=names)


@functools.lru_cache(maxsize=None)
def gn_plain_case(rows, c, groups):
    """train_cases.gn_case: per-group offsets and scales, a constant group, no element near the ReLU threshold."""
    return T.gn_case(rows, c, groups, seed=5)


def split_into_slabs(x, nslabs, bias, row_bias, g):
    """fp32 slabs [nslabs][rows][c] whose finish32 sum with (bias, row_bias) is close to x: the family structure reaches the kernel through the slabs."""
    rest = x.double()
    if bias is not None:
        rest = rest - bias.double()
    if row_bias is not None:
        rest = rest - row_bias.double()
    parts = torch.randn(nslabs, *x.shape, generator=g, dtype=torch.float64) * rest.abs().clamp_min(1e-3) * 0.5
    parts[-1] = rest - parts[:-1].sum(0)
    return parts.float()


def nonfinite_rows(x, groups, row=None, group=None):
    """x with an inf and a NaN inside one (row, group) (the last row's last group by default): (copy, row, group)."""
    rows, c = x.shape
    gsz = c // groups
    row = rows - 1 if row is None else row
    group = groups - 1 if group is None else group
    bad = x.clone()
    bad[row, group * gsz] = float("inf")
    bad[row, group * gsz + gsz // 2] = NAN
    return bad, row, group


# ------------------------------------------------------------------------------------------------------------ fused layer
@functools.lru_cache(maxsize=None)
def fused_case(m, k1, k2, c, groups, kind):
    """kind "int": integer activations, weights, bias, row bias (z exact); "rowbias": zero activations, bias None, row_bias = a family matrix per
    (row, group) (z = row_bias exactly); "groupbias": randn product, bias = a per-group offset of +-30 / +-1000, randn row bias."""
    g = _gen(m, k1, k2, c, groups, ("int", "rowbias", "groupbias").index(kind))
    k = k1 + k2
    gsz = c // groups
    base = gn_family_case(min(m, 3), c, groups, rot=m % 15)
    gamma, beta = base["gamma"], base["beta"]
    names = None
    if kind == "int":
        a = torch.randint(-3, 4, (m, k), generator=g).half()
        w = torch.randint(-3, 4, (c, k), generator=g).half()
        bias = torch.randint(-8, 9, (c,), generator=g).float()
        rb = torch.randint(-8, 9, (m, c), generator=g).float()
        gamma = gamma.clone()
        gamma[1] = 1.5
    elif kind == "rowbias":
        a = torch.zeros(m, k, dtype=torch.float16)
        w = (torch.randn(c, k, generator=g) / math.sqrt(k)).half()
        names = group_names(m, groups, m % 15)
        rb = torch.stack([torch.cat([T._column(names[r][q], gsz, g) for q in range(groups)]) for r in range(m)]).float()
        bias = None
    else:
        a = torch.randn(m, k, generator=g).half()
        w = (torch.randn(c, k, generator=g) / math.sqrt(k)).half()
        off = torch.tensor([30.0, -30.0, 1000.0, -1000.0])[torch.arange(groups) % 4]
        bias = (off.repeat_interleave(gsz) + 0.2 * torch.randn(c, generator=g)).float()
        rb = (0.2 * torch.randn(m, c, generator=g)).float()
        gamma = gamma.clone()
        gamma[1] = 1.5
    return dict(a1=a[:, :k1].contiguous(), a2=a[:, k1:].contiguous() if k2 else None, a=a, w=w, bias=bias, row_bias=rb, gamma=gamma, beta=beta,
                names=names, kind=kind)


def fused_statement(a, w, bias, row_bias, mode, groups, gamma=None, beta=None, exact_z=False):
    """(want fp64 before the clamp and rounding, bound, z fp64, d).  exact_z: the case's pre-activation is exact in fp32 (kinds "int" and "rowbias")."""
    m, k = a.shape
    c = w.shape[0]
    z = a.double() @ w.double()[:, :k].t()
    mag = a.double().abs() @ w.double()[:, :k].abs().t()
    for t in (bias, row_bias):
        if t is not None:
            z, mag = z + t.double(), mag + t.double().abs().expand(m, c)
    d = torch.zeros_like(z) if exact_z else sum_bound(fused_chain(k, c, mode, groups), mag)
    if mode == 0:
        _, ct, _ = fused_tiles(c, 0, groups)
        want, bound = gn_relu_statement(z, gamma, beta, groups, ct + 6, d)
        return want, bound, z, d
    if mode == 1:
        want = z.clamp_min(0)
        return want, d + U16 * (want.clamp(max=F16_MAX) + d) + 2.0 ** -25, z, d
    return z, d + 0 * z, z, d


def fused32(a, w, bias, row_bias, mode, groups, gamma=None, beta=None, row_shift_mutant=False, **mut):
    """pcd_skinny_fused in fp32 in the kernel's order: chunk ch to split ch % KSPLIT, k in sequence, the splits in order, + (bias + row_bias)."""
    m, k = a.shape
    c = w.shape[0]
    _, ct, ksplit = fused_tiles(c, mode, groups)
    A, W = a.float(), w.float()[:, :k]
    nch = k // 64
    acc = torch.zeros(ksplit, m, c, dtype=torch.float32)
    for ch in range(nch):
        s = ch % ksplit
        for e in range(64):
            kk = 64 * ch + e
            acc[s] = acc[s] + A[:, kk:kk + 1] * W[:, kk].unsqueeze(0)
    x = torch.zeros(m, c, dtype=torch.float32)
    for s in range(ksplit):
        x = x + acc[s]
    cb = torch.zeros(m, c, dtype=torch.float32) if bias is None else bias.float().expand(m, c)
    if row_bias is not None:
        cb = cb + row_bias.float()
    z = x + cb
    if mode == 0:
        return gn32(z, gamma, beta, groups, ct, **mut)
    if mode == 1:
        return finish32(z.unsqueeze(0), None, None, 1, **mut)
    return z


# ------------------------------------------------------------------------------------------------------------ the whole network
LAT_K = (256, 128, 256, 512, 1024, 2048, 5120, 1536, 768, 384, 128, 128)
LAT_C = (128, 256, 512, 1024, 2048, 4096, 1024, 512, 256, 128, 128, 256)
LAT_K2 = (0, 0, 0, 0, 0, 0, 1024, 512, 256, 128, 0, 0)
LAT_MODE = (0,) * 10 + (1, 2)
LAT_GROUPS = 8
ORDERS = ("torch", "reversed", "four")


def pack_layers(lin, gn):
    """The packer's (lin, gn) as the kernels hold them: weights fp16, everything else fp32."""
    as_t = lambda v: torch.as_tensor(v)
    layers = []
    for i, (w, b) in enumerate(lin):
        L = dict(w=as_t(w).half(), b=as_t(b).float())
        if i < len(gn):
            L["gamma"], L["beta"] = as_t(gn[i][0]).float(), as_t(gn[i][1]).float()
        layers.append(L)
    assert tuple(L["w"].shape[1] for L in layers) == LAT_K and tuple(L["w"].shape[0] for L in layers) == LAT_C
    return layers


def _matmul(a, w, order):
    """a [m][k] @ w [c][k]^T in a's dtype; order: torch's own, K reversed, or 64-deep chunks dealt to four accumulators, (r0 + r1) + (r2 + r3)."""
    if order == "torch":
        return a @ w.t()
    if order == "reversed":
        return a.flip(1) @ w.flip(1).t()
    k = a.shape[1]
    ch = torch.arange(k) // 64 % 4
    r = [a[:, ch == j] @ w[:, ch == j].t() if bool((ch == j).any()) else torch.zeros(a.shape[0], w.shape[0], dtype=a.dtype) for j in range(4)]
    return (r[0] + r[1]) + (r[2] + r[3])


def layer_inputs(i, acts):
    """The (a1, a2) of layer i from the activations so far (acts[j] = output of layer j; acts[-1] = z16), as csrc/latent.hip wires them."""
    skip = {6: 3, 7: 2, 8: 1, 9: 0}
    return (acts[i - 1], acts[skip[i]]) if i in skip else (acts[i - 1], None)


def network(layers, trow, z, dtype=torch.float64, order="torch", shift_z3_mutant=False, taps=None):
    """eps [B][256] in `dtype` from z fp32 [B][256] and the hoisted time row trow [128] (or [B][128])."""
    acts = {-1: sat16(z.float())}
    for i, L in enumerate(layers):
        a1, a2 = layer_inputs(i, acts)
        if shift_z3_mutant and i == 7:
            a2 = a2.roll(64, 1)
        a = (torch.cat([a1, a2], 1) if a2 is not None else a1).to(dtype)
        bias = torch.as_tensor(trow).to(dtype) if i == 0 else L["b"].to(dtype)
        v = _matmul(a, L["w"].to(dtype), order) + bias
        if LAT_MODE[i] == 0:
            B, c = v.shape
            vg = v.reshape(B, LAT_GROUPS, -1)
            mu = vg.mean(2, keepdim=True)
            dv = vg - mu
            rs = 1 / torch.sqrt((dv * dv).mean(2, keepdim=True) + torch.tensor(EPS, dtype=dtype))
            v = ((dv * rs).reshape(B, c) * L["gamma"].to(dtype) + L["beta"].to(dtype)).clamp_min(0)
            acts[i] = sat16(v)
        elif LAT_MODE[i] == 1:
            acts[i] = sat16(v.clamp_min(0))
        else:
            acts[i] = v
        if taps is not None:
            taps.append(acts[i])
    return acts[len(layers) - 1]


def ddim_tables(nsteps, t0=0.9, t1=0.05):
    """(ts [nsteps], rates fp32 (4, nsteps, 1) = (n, s, n_next, s_next)) of a cosine schedule from t0 down to t1: n = sin, s = cos of (pi / 2) t."""
    ts = torch.tensor([t0 - (t0 - t1) * k / nsteps for k in range(nsteps)], dtype=torch.float64)
    tn = ts - (t0 - t1) / nsteps
    f = lambda t: (torch.sin(0.5 * math.pi * t.clamp_min(0)), torch.cos(0.5 * math.pi * t.clamp_min(0)))
    (n, s), (n2, s2) = f(ts), f(tn)
    return ts.float(), torch.stack([n, s, n2, s2]).float().reshape(4, nsteps, 1)


def ddim(layers, trows, rates, z, nsteps, dtype=torch.float64, order="torch", **mut):
    """nsteps DDIM steps, pcd_ddim_update's operation order: (z, x0) in `dtype`.  trows [nsteps][128]."""
    zz = z.to(dtype)
    x0 = zz
    for k in range(nsteps):
        n, s, n2, s2 = (rates[q, k, 0].to(dtype) for q in range(4))
        eps = network(layers, trows[k], zz.float(), dtype, order, **mut)
        ne = n * eps
        x0 = (zz - ne) / s
        zz = s2 * x0 + n2 * eps
    return zz, x0


def row_col_errors(got, want):
    """dict of the four figures: per row and per column, max-abs over the row's (column's) max-abs, and rel-L2."""
    err, w = (got.double() - want.double()), want.double()
    out = {}
    for name, dim in (("row", 1), ("col", 0)):
        out[name + "_abs"] = float((err.abs().max(dim).values / w.abs().max(dim).values).max())
        out[name + "_l2"] = float((err.norm(dim=dim) / w.norm(dim=dim)).max())
    return out


def network_figures(layers, trows, rates, z, nsteps):
    """want (fp64; eps for nsteps = 0, else (z, x0)) and the figures of each fp32 order: {order: {output: {figure: value}}}."""
    if nsteps == 0:
        run = lambda dt, o: {"eps": network(layers, trows[0], z, dt, o)}
    else:
        run = lambda dt, o: dict(zip(("z", "x0"), ddim(layers, trows, rates, z, nsteps, dt, o)))
    want = run(torch.float64, "torch")
    figs = {o: {name: row_col_errors(got, want[name]) for name, got in run(torch.float32, o).items()} for o in ORDERS}
    return want, figs


def bounds_from(figs, orders=ORDERS, factor=3.0):
    """{output: {figure: factor x the largest over `orders`}}"""
    names = figs[orders[0]].keys()
    return {n: {f: factor * max(figs[o][n][f] for o in orders) for f in figs[orders[0]][n]} for n in names}


def latent_input(batch, seed=11):
    """The first `batch` of 64 rows of randn * 1.2."""
    return (torch.randn(64, 256, generator=torch.Generator().manual_seed(seed)) * 1.2)[:batch].contiguous()
