"""Every launch of the attention backbone that contains a LayerNorm, judged ROW BY ROW on the families of tests/ln_cases.py: the plain kernels
(pcd_layernorm_f16, pcd_layernorm_train_f16, pcd_layernorm_backward_f16), the three launches that normalise MFMA B fragments in place
(PCD_LN_FRAGMENTS, csrc/device_prims.h: pcd_pw_wide_ln_linear, pcd_sab_head_f16, pcd_wide_ffn_f16) and pcd_sab_tail_f16, which normalises its
fp32 accumulators.  A whole-tensor rel-L2 over 512 rows lets one row that is 3 % wrong through; here every row has its own bound, and a
failure names the launch, C, the row and its family.

Bounds: a LayerNorm (and LayerNorm + Linear) row lies within 1e-3 of the fp64 statement, 2 x what tests/test_ln_cases_cpu.py holds the fp32
statement to.  The overflow families (|x - mean| >= 65520 with every x finite) are the ones a subtraction in fp16 turns into beta."""
import pytest
import torch

import ln_cases as L
from helpers import sab_sd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROW_BOUND = 1e-3             # LayerNorm and LayerNorm + Linear rows against fp64
FACTOR = 4.0                 # a residual launch's row: its whole-tensor bound, or FACTOR x the fp32 statement's own deviation on that row


def _check_rows(launch, C, names, err, bound, what="rel-L2", only=None):
    """err [rows] <= bound (a number or [rows]) on every row (of `only`); the message lists every failing (row, family, figure)."""
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    rows = range(len(names)) if only is None else only
    bad = [(r, names[r], f"{float(err[r]):.3g} > {float(bound[r]):.3g}") for r in rows if not float(err[r]) <= float(bound[r])]
    worst = max(rows, key=lambda r: float(torch.nan_to_num(err[r] / bound[r], nan=float("inf"))))
    print(f"{launch} C = {C}: worst {what} {float(err[worst]):.2e} (bound {float(bound[worst]):.2e}) at row {worst} ({names[worst]})")
    assert not bad, f"{launch}, C = {C}, {what}: {len(bad)} rows fail (row, family, figure): {bad}"


def _lib_st():
    from shapegen_amd import _lib
    return _lib, _lib.load(), _lib.stream_ptr()


@pytest.mark.parametrize("C", [64, 128, 256, 96])
def test_layernorm_rows_by_family(C):
    """pcd_layernorm_f16: the vector kernel (C = 64 / 128 / 256) and the generic one (C = 96), a ragged row count."""
    from shapegen_amd import ops
    x, names = L.rows_tensor(C, 512 + 5, 256, 1)
    ga, be = L.affine(C, 1)
    got = ops.layernorm_f16(x.cuda(), ga.cuda(), be.cuda()).cpu()
    assert got.dtype == torch.float16 and torch.isfinite(got).all()
    _check_rows("pcd_layernorm_f16", C, names, L.row_rel(got, L.ln64(x, ga, be)), ROW_BOUND)


@pytest.mark.parametrize("C", [64, 128, 256])
def test_layernorm_train_and_backward_rows_by_family(C):
    """pcd_layernorm_train_f16: the bits of pcd_layernorm_f16 and the fp64 statistics; pcd_layernorm_backward_f16 on those statistics."""
    _lib, lib, st = _lib_st()
    rows = 512 + 5
    x, names = L.rows_tensor(C, rows, 256, 2)
    ga, be = L.affine(C, 2)
    xd, gd, bd = x.cuda(), ga.cuda(), be.cuda()
    y, y0 = torch.empty_like(xd), torch.empty_like(xd)
    mu, rs = torch.full((rows,), float("nan"), device="cuda"), torch.full((rows,), float("nan"), device="cuda")
    _lib.check(lib.pcd_layernorm_train_f16(xd.data_ptr(), rows, C, gd.data_ptr(), bd.data_ptr(), y.data_ptr(), mu.data_ptr(), rs.data_ptr(), st), "ln_train")
    _lib.check(lib.pcd_layernorm_f16(xd.data_ptr(), rows, C, gd.data_ptr(), bd.data_ptr(), y0.data_ptr(), st), "ln")
    torch.cuda.synchronize()
    _check_rows("pcd_layernorm_train_f16 y", C, names, L.row_rel(y.cpu(), L.ln64(x, ga, be)), ROW_BOUND)
    assert torch.equal(y, y0)                                      # "same values" as pcd_layernorm_f16
    m64, r64 = L.stats64(x)
    xmax = x.double().abs().max(dim=1).values
    _check_rows("pcd_layernorm_train_f16 mean", C, names, (mu.cpu().double() - m64).abs(), 1e-6 * xmax, "|mean - fp64|")
    _check_rows("pcd_layernorm_train_f16 rstd", C, names, (rs.cpu().double() / r64 - 1).abs(), 1e-6, "rstd relative")
    # backward, accumulate = 0
    dy = torch.randn(rows, C, generator=torch.Generator().manual_seed(9 + C)).half()
    dyd = dy.cuda()
    dx = torch.full((rows, C), float("nan"), dtype=torch.float16, device="cuda")
    dgam, dbet = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    ws = torch.empty(lib.pcd_layernorm_backward_workspace_bytes(rows, C) // 4, device="cuda")
    _lib.check(lib.pcd_layernorm_backward_f16(dyd.data_ptr(), xd.data_ptr(), rows, C, mu.data_ptr(), rs.data_ptr(), gd.data_ptr(), 0, dx.data_ptr(),
                                              dgam.data_ptr(), dbet.data_ptr(), ws.data_ptr(), ws.numel() * 4, st), "ln_backward")
    torch.cuda.synchronize()
    gx, gg, gb = L.ln_backward64(dy, x, ga, be)
    assert torch.isfinite(dx.float()).all()
    _check_rows("pcd_layernorm_backward_f16 dx", C, names, L.row_rel(dx.cpu(), gx), 5e-3)
    from helpers import rel_l2
    assert rel_l2(dgam.cpu(), gg) <= 1e-4 and rel_l2(dbet.cpu(), gb) <= 1e-4


@pytest.mark.parametrize("passes", [1, 3])
def test_wide_ln_linear_rows_by_family(passes):
    """pcd_pw_wide_ln_linear (C = 256): LN1 + in_proj of the synthetic block, one and three 256-wide output passes, no ReLU."""
    _lib, lib, st = _lib_st()
    rows, C = 512, 256
    x, names = L.rows_tensor(C, rows, 256, 3)
    sd = sab_sd(C)
    w, b = sd["attention.in_proj_weight"][:256 * passes].half().contiguous(), sd["attention.in_proj_bias"][:256 * passes].float().contiguous()
    ga, be = sd["ln1.weight"].float(), sd["ln1.bias"].float()
    xd, wd, bd, gd, bed = x.cuda(), w.cuda(), b.cuda(), ga.cuda(), be.cuda()
    packed = torch.empty(lib.pcd_pw_wide_ln_linear_packed_bytes(passes), dtype=torch.uint8, device="cuda")
    _lib.check(lib.pcd_pw_wide_ln_linear_pack(wd.data_ptr(), bd.data_ptr(), passes, gd.data_ptr(), bed.data_ptr(), packed.data_ptr(), st))
    out = torch.full((rows, 256 * passes), float("nan"), dtype=torch.float16, device="cuda")
    assert lib.pcd_pw_wide_ln_linear_supported(256, rows) == 1
    _lib.check(lib.pcd_pw_wide_ln_linear(packed.data_ptr(), passes, 0, xd.data_ptr(), rows, out.data_ptr(), st))
    out2 = torch.full_like(out, float("nan"))
    _lib.check(lib.pcd_pw_wide_ln_linear(packed.data_ptr(), passes, 0, xd.data_ptr(), rows, out2.data_ptr(), st))
    got = out.cpu()
    assert torch.isfinite(got).all()
    _check_rows(f"pcd_pw_wide_ln_linear passes = {passes}", C, names, L.row_rel(got, L.ln_linear(x, ga, be, w, b)), ROW_BOUND)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("C", [64, 128])
def test_sab_head_rows_by_family(C):
    """pcd_sab_head_f16: qkv = in_proj(LN1(x)) in one launch."""
    _lib, lib, st = _lib_st()
    from shapegen_amd.networks import _PackedSAB
    rows = 512
    x, names = L.rows_tensor(C, rows, 256, 4)
    sd = sab_sd(C)
    pk = _PackedSAB(sd, "", C, torch.device("cuda"))
    desc = pk.fill(_lib.SabDesc())
    xd = x.cuda()
    qkv = torch.full((rows, 3 * C), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.pcd_sab_head_f16(C, desc.tail_packed, xd.data_ptr(), rows, qkv.data_ptr(), st))
    q2 = torch.full_like(qkv, float("nan"))
    _lib.check(lib.pcd_sab_head_f16(C, desc.tail_packed, xd.data_ptr(), rows, q2.data_ptr(), st))
    got = qkv.cpu()
    assert torch.isfinite(got).all()
    want = L.ln_linear(x, sd["ln1.weight"].float(), sd["ln1.bias"].float(), sd["attention.in_proj_weight"], sd["attention.in_proj_bias"].float())
    _check_rows("pcd_sab_head_f16", C, names, L.row_rel(got, want), ROW_BOUND)
    assert torch.equal(qkv, q2)


def _check_residual_rows(launch, C, names, x, got, want64, want32, tensor_bound):
    """A launch y = x + f(x): rows below 1024 by the rel-L2 of f's term; bulk300_outlier by f's term on its bulk; the other rows near the fp16
    range, where the residual hides f, element by element within one fp16 ulp of the statement."""
    assert got.dtype == torch.float16 and torch.isfinite(got).all(), launch
    xd, g, w64, w32 = x.double(), got.double(), want64.double(), want32.double()
    term = L.row_rel(g - xd, w64 - xd)
    dev32 = L.row_rel(w32 - xd, w64 - xd)
    small = [r for r in range(len(names)) if names[r] not in L.NEAR_RANGE]
    assert all(float(x[r].abs().max()) < 1024 for r in small)
    print(f"{launch} C = {C}: rows below 1024: kernel worst {float(term[small].max()):.2e}, fp32 statement worst {float(dev32[small].max()):.2e} "
          f"(bound: the larger of {tensor_bound:.0e} and {FACTOR:.0f} x the row's fp32 figure)")
    bound = torch.maximum(torch.full_like(dev32, tensor_bound), FACTOR * dev32)
    _check_rows(launch, C, names, term, bound, "rel-L2 of the launch's term, rows below 1024", only=small)
    bulk = torch.ones(x.shape[1], dtype=torch.bool)
    bulk[x.shape[1] // 2] = False
    for r, name in enumerate(names):
        if name == "bulk300_outlier":
            e = float(((g - xd)[r, bulk] - (w64 - xd)[r, bulk]).norm() / (w64 - xd)[r, bulk].norm())
            print(f"{launch} C = {C}: row {r} (bulk300_outlier): term on the bulk rel-L2 {e:.3g}")
            assert e <= 0.1, (launch, C, r, name, e)
        elif name in L.NEAR_RANGE:
            ulps = ((g[r] - w64[r]).abs() / L.ulp16(torch.maximum(g[r].abs(), w64[r].abs()))).max()
            assert float(ulps) <= 1.0, (launch, C, r, name, float(ulps))


def test_wide_ffn_rows_by_family():
    """pcd_wide_ffn_f16 (C = 256, 128-row tiles): y = x + FFN(LN2(x))."""
    _lib, lib, st = _lib_st()
    rows, C = 256, 256
    x, names = L.rows_tensor(C, rows, 128, 5)
    sd = sab_sd(C)
    dev = lambda t: t.cuda().contiguous()
    w1d, b1d, w2d, b2d = dev(sd["ff.0.weight"].half()), dev(sd["ff.0.bias"].float()), dev(sd["ff.2.weight"].half()), dev(sd["ff.2.bias"].float())
    gd, bd, xd = dev(sd["ln2.weight"].float()), dev(sd["ln2.bias"].float()), x.cuda()
    assert lib.pcd_wide_ffn_supported(256, rows) == 1
    packed = torch.empty(lib.pcd_wide_ffn_packed_bytes(), dtype=torch.uint8, device="cuda")
    _lib.check(lib.pcd_wide_ffn_pack(w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), gd.data_ptr(), bd.data_ptr(), packed.data_ptr(), st))
    y = torch.full((rows, C), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.pcd_wide_ffn_f16(packed.data_ptr(), xd.data_ptr(), rows, y.data_ptr(), st), "wide_ffn")
    y2 = torch.full_like(y, float("nan"))
    _lib.check(lib.pcd_wide_ffn_f16(packed.data_ptr(), xd.data_ptr(), rows, y2.data_ptr(), st), "wide_ffn")
    _check_residual_rows("pcd_wide_ffn_f16", C, names, x, y.cpu(), L.wide_ffn(x, sd), L.wide_ffn(x, sd, torch.float32), 2e-3)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("C", [64, 128])
def test_sab_tail_rows_by_family(C):
    """pcd_sab_tail_f16: x1 = x + out_proj(a), y = x1 + FFN(LN2(x1)), LayerNorm on the fp32 accumulators; the families in x, a = 0.7 randn."""
    _lib, lib, st = _lib_st()
    from shapegen_amd.networks import _PackedSAB
    rows = 512
    x, names = L.rows_tensor(C, rows, 256, 6)
    a = (torch.randn(rows, C, generator=torch.Generator().manual_seed(60 + C)) * 0.7).half()
    sd = sab_sd(C)
    pk = _PackedSAB(sd, "", C, torch.device("cuda"))
    desc = pk.fill(_lib.SabDesc())
    assert desc.tail_packed and lib.pcd_sab_tail_supported(C, rows) == 1
    ad, xd = a.cuda(), x.cuda()
    y = torch.full((rows, C), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.pcd_sab_tail_f16(C, desc.tail_packed, ad.data_ptr(), xd.data_ptr(), rows, y.data_ptr(), st))
    y2 = torch.full_like(y, float("nan"))
    _lib.check(lib.pcd_sab_tail_f16(C, desc.tail_packed, ad.data_ptr(), xd.data_ptr(), rows, y2.data_ptr(), st))
    _check_residual_rows("pcd_sab_tail_f16", C, names, x, y.cpu(), L.sab_tail(a, x, sd), L.sab_tail(a, x, sd, torch.float32), 1e-3)
    assert torch.equal(y, y2)
