"""Row families and statements shared by tests/test_ln_cases_cpu.py (which holds the fp32 statement to the fp64 one on them) and
tests/test_gpu_layernorm_rows.py (which holds every launch that contains a LayerNorm to the fp64 statement, row by row).

A family is one fp16 row [C] of a kind a LayerNorm kernel can get wrong: a mean far above the spread, values at the edge of the fp16
range, constant rows, fp16 subnormals, and rows whose |x - mean| does not fit fp16 although every x does (OVERFLOW: a kernel that
forms x - mean in fp16 gets inf there).  Everything comes from seeded CPU generators."""
import torch

EPS = 1e-5
F16_MAX = 65504.0
OVERFLOW_AT = 65520.0        # from here on a value rounds to inf in fp16

# max|x - mean| >= OVERFLOW_AT at every C >= 64
OVERFLOW = ("advice", "one_neg", "last50000")
# ... and at C = 256 only (at C = 64 / 128 the outlier pulls the mean far enough: an ordinary hard row there)
OVERFLOW_256 = "bulk300_outlier"
# rows with max|x| >= 1024: behind a residual the FFN term is below the fp16 resolution of the sum
NEAR_RANGE = ("const60000", "alt60000", "alt65504", "spike", "mean20000", "advice", "one_neg", "last50000", "bulk300_outlier")
FILLER = "filler"            # the rows between the families: randn * 1.5


def sat16(t):
    """Round to fp16 as the kernels do: clamped to the largest normal, never +-inf."""
    return t.clamp(-F16_MAX, F16_MAX).half()


def families(C, generator):
    """name -> fp16 row [C]; every row is finite and has a finite fp64 LayerNorm."""
    g = generator
    rn = lambda: torch.randn(C, generator=g)
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    f = {}
    f["randn"] = rn() * 1.5
    f["mean50"] = 50.0 + 0.1 * rn()
    f["mean_m300"] = -300.0 + 0.5 * rn()
    f["small"] = 0.02 * rn()
    f["subnormal"] = 2e-6 * rn()
    f["const7"] = torch.full((C,), 7.0)
    f["const60000"] = torch.full((C,), 60000.0)
    f["zeros"] = torch.zeros(C)
    f["alt60000"] = sign * 60000.0 * (0.5 + 0.5 * torch.rand(C, generator=g))
    f["alt65504"] = sign * F16_MAX
    f["spike"] = torch.zeros(C)
    f["spike"][C // 3] = F16_MAX
    f["mean20000"] = 20000.0 + 3000.0 * rn()
    # three quarters of the channels near -30000, one quarter near +60000: mean ~ -7500, the upper quarter ~ 67500 above it
    f["advice"] = torch.where(torch.arange(C) % 4 == 3, 60000.0, -30000.0) + 100.0 * rn()
    # all +65504, one -65504: that element lies 131008 (1 - 1 / C) below the mean
    f["one_neg"] = torch.full((C,), F16_MAX)
    f["one_neg"][C // 4 + 1] = -F16_MAX
    # -40000 +- 100, the last element +50000: 90000 (1 - 1 / C) above the mean
    f["last50000"] = -40000.0 + 100.0 * (2 * torch.rand(C, generator=g) - 1)
    f["last50000"][C - 1] = 50000.0
    # 300 + randn with one element at -65504: overflows at C = 256 only, and the one overflow row whose bulk is small enough
    # (fp16 ulp 0.25) for an FFN term to show behind a residual
    f["bulk300_outlier"] = 300.0 + rn()
    f["bulk300_outlier"][C // 2] = -F16_MAX
    return {k: v.half() for k, v in f.items()}


NAMES = tuple(families(64, torch.Generator().manual_seed(0)))


def layout(rows, tile):
    """The family name of every row of a [rows, C] tensor (FILLER for the others), rows >= 2 * tile, tile a multiple of 16 * 8.
    Every family stands in tile 0 and in tile 1, on different lanes (row % 32) and in different waves (row // 32 % 8, and
    row % tile // 32); row 0 and the last row carry a family, the last one a tame one; a filler row follows every other family row;
    a ragged tail behind tile 1 starts with an overflow row."""
    nf = len(NAMES)
    stride = tile // nf
    assert rows >= 2 * tile and stride >= 8 and tile % 32 == 0
    names = [FILLER] * rows
    for i, name in enumerate(NAMES):
        names[stride * i] = name
        names[tile + stride * ((i + 5) % nf) + 3] = name
    if rows - 1 > 2 * tile + 1:
        names[2 * tile] = "one_neg"
    assert names[rows - 1] == FILLER and names[rows - 2] == FILLER
    names[rows - 1] = "randn"
    return names


def rows_tensor(C, rows, tile, seed):
    """(x fp16 [rows, C], names): `layout` filled with the families of C (seeded per C and seed) between rows of randn * 1.5."""
    g = torch.Generator().manual_seed(1000 * seed + C)
    fam = families(C, g)
    names = layout(rows, tile)
    x = (torch.randn(rows, C, generator=g) * 1.5).half()
    for r, name in enumerate(names):
        if name != FILLER:
            x[r] = fam[name]
    return x, names


def affine(C, seed):
    """gamma, beta fp32 for the plain kernels (tests/test_gpu_train_attention.py's)."""
    g = torch.Generator().manual_seed(77 * seed + C)
    return 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)


# ---------------------------------------------------------------------------------------------------------------- statements
def _stats(x, dtype):
    x = x.to(dtype)
    mean = x.mean(dim=-1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(dim=-1, keepdim=True) + EPS)
    return d, mean, rstd


def stats64(x):
    """(mean, rstd) [rows] in fp64: biased variance about the mean, eps 1e-5 inside the root."""
    _, mean, rstd = _stats(x, torch.float64)
    return mean[..., 0], rstd[..., 0]


def stats32(x):
    """What the kernels declare: fp32 sums, two passes."""
    _, mean, rstd = _stats(x, torch.float32)
    return mean[..., 0], rstd[..., 0]


def ln(x, gamma, beta, dtype):
    """LayerNorm over the last axis with `dtype` statistics and affine, not rounded."""
    d, _, rstd = _stats(x, dtype)
    return d * rstd * gamma.to(dtype) + beta.to(dtype)


def ln64(x, gamma, beta):
    return ln(x, gamma, beta, torch.float64)


def ln32(x, gamma, beta):
    """The kernels' declared arithmetic: fp32 two-pass statistics, fp32 affine, clamped to +-65504 and rounded to fp16."""
    return sat16(ln(x, gamma, beta, torch.float32))


def ln_backward32(dy, x, mean, rstd, gamma):
    """dx = fp16(rstd (g dy - mean(g dy) - xhat mean(g dy xhat))) in fp32 from saved statistics [rows]."""
    xh = (x.float() - mean.float()[:, None]) * rstd.float()[:, None]
    gd = dy.float() * gamma.float()
    a = gd.mean(dim=1, keepdim=True)
    b = (gd * xh).mean(dim=1, keepdim=True)
    return sat16(rstd.float()[:, None] * (gd - a - xh * b))


def ln_backward64(dy, x, gamma, beta):
    """(dx, dgamma, dbeta) of sum(dy * LayerNorm(x)) by fp64 autograd."""
    with torch.enable_grad():
        xr = x.double().requires_grad_(True)
        gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        y = torch.nn.functional.layer_norm(xr, (x.shape[1],), gr, br, EPS)
        return torch.autograd.grad(y, (xr, gr, br), dy.double())


def row_rel(a, b):
    """Per-row rel-L2 of a against b, in fp64."""
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)


def ln_linear(x, gamma, beta, w, b, dtype=torch.float64):
    """Linear(fp16(LayerNorm(x))) from the fp16-rounded weights, not rounded (tests/test_gpu_attention.py's statement)."""
    return sat16(ln(x, gamma, beta, dtype)).to(dtype) @ w.half().to(dtype).T + b.to(dtype)


def wide_ffn(x, sd, dtype=torch.float64):
    """pcd_wide_ffn_f16's statement (test_wide_ffn_one_launch_against_fp64): y = fp16(x + fp16(ff.2(fp16(relu(ff.0(fp16(LN2(x)))))))), as fp16."""
    f = lambda k: sd[k].to(dtype)
    h = lambda k: sd[k].half().to(dtype)
    lnx = sat16(ln(x, sd["ln2.weight"], sd["ln2.bias"], dtype)).to(dtype)
    hid = sat16(torch.relu(lnx @ h("ff.0.weight").T + f("ff.0.bias"))).to(dtype)
    return sat16(sat16(hid @ h("ff.2.weight").T + f("ff.2.bias")).to(dtype) + x.to(dtype))


def sab_tail(a, x, sd, dtype=torch.float64):
    """pcd_sab_tail_f16's statement (_tail_fp64): x1 = x + out_proj(a); y = fp16(x1 + ff.2(fp16(relu(ff.0(fp16(LN2(x1))))))), as fp16; x1 stays wide."""
    f = lambda k: sd[k].to(dtype)
    h = lambda k: sd[k].half().to(dtype)
    x1 = x.to(dtype) + a.to(dtype) @ h("attention.out_proj.weight").T + f("attention.out_proj.bias")
    lnx = sat16(ln(x1, sd["ln2.weight"], sd["ln2.bias"], dtype)).to(dtype)
    hid = sat16(torch.relu(lnx @ h("ff.0.weight").T + f("ff.0.bias"))).to(dtype)
    return sat16(x1 + hid @ h("ff.2.weight").T + f("ff.2.bias"))


def ulp16(t):
    """The spacing of fp16 at |t| (of the binade below at a power of two; 2^-24 below the normals)."""
    t = torch.as_tensor(t, dtype=torch.float64).abs().clamp_min(2.0 ** -14)
    return 2.0 ** (torch.floor(torch.log2(t)) - 10)
