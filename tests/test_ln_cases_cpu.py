"""The statements of tests/ln_cases.py against each other, on the CPU.  tests/test_gpu_layernorm_rows.py holds the kernels to the fp64
statement at 2 x the bounds asserted here for the fp32 statement (the arithmetic the kernels declare), so these keep those bounds honest:
if the fp32 statement itself left them on some family, a correct kernel could not meet them.

Bounds (C = 64 / 96 / 128 / 256, every affine below): ln32 v. ln64 per row 5e-4 (one fp16 rounding is 2^-11 = 4.9e-4 at worst and 2.8e-4 rms);
mean 1e-7 max|x|; rstd 5e-7 relative; backward 2.5e-3 (the worst rows are those whose dx is an fp16 subnormal)."""
import pytest
import torch

import ln_cases as L

CS = (64, 96, 128, 256)


def _affines(C):
    """The affines of the GPU tests: the random one of the plain kernels, ln1 / ln2 of the synthetic attention block where it exists."""
    out = {"random": L.affine(C, 1)}
    if C != 96:
        from helpers import sab_sd
        sd = sab_sd(C)
        out["ln1"] = (sd["ln1.weight"].float(), sd["ln1.bias"].float())
        out["ln2"] = (sd["ln2.weight"].float(), sd["ln2.bias"].float())
    return out


def _stack(C):
    fam = L.families(C, torch.Generator().manual_seed(C))
    return list(fam), torch.stack(list(fam.values()))


def test_families_are_the_table():
    assert len(L.NAMES) == 16 and set(L.OVERFLOW) | {L.OVERFLOW_256} | set(L.NEAR_RANGE) <= set(L.NAMES)
    for C in CS:
        names, x = _stack(C)
        assert tuple(names) == L.NAMES and x.dtype == torch.float16 and x.shape == (16, C)
        assert torch.isfinite(x).all()
        for ga, be in _affines(C).values():
            assert torch.isfinite(L.ln64(x, ga, be)).all()
        for name, row in zip(names, x):
            assert (float(row.abs().max()) >= 1024) == (name in L.NEAR_RANGE), (C, name)


@pytest.mark.parametrize("C", CS)
def test_overflow_families_keep_their_teeth(C):
    """max|x - mean| does not fit fp16 on the overflow families (a kernel that subtracts in fp16 gets inf there), and does on all others."""
    names, x = _stack(C)
    dev = (x.double() - x.double().mean(dim=1, keepdim=True)).abs().max(dim=1).values
    for name, d in zip(names, dev):
        want = name in L.OVERFLOW or (name == L.OVERFLOW_256 and C == 256)
        assert (float(d) >= L.OVERFLOW_AT) == want, (C, name, float(d))
    # the packed-fp16 subtraction x - fp16(mean) itself: inf exactly there
    mh = L.sat16(x.float().mean(dim=1, keepdim=True))
    inf = torch.isinf(x - mh).any(dim=1)
    assert [n for n, i in zip(names, inf) if i] == [n for n in names if n in L.OVERFLOW or (n == L.OVERFLOW_256 and C == 256)]


@pytest.mark.parametrize("C", CS)
def test_fp32_statement_against_fp64(C):
    names, x = _stack(C)
    m32, r32 = L.stats32(x)
    m64, r64 = L.stats64(x)
    xmax = x.double().abs().max(dim=1).values
    for i, name in enumerate(names):
        assert abs(float(m32[i]) - float(m64[i])) <= 1e-7 * float(xmax[i]), (C, name)
        assert abs(float(r32[i]) / float(r64[i]) - 1) <= 5e-7, (C, name)
    g = torch.Generator().manual_seed(5 * C)
    dy = torch.randn(len(names), C, generator=g).half()
    for key, (ga, be) in _affines(C).items():
        rel = L.row_rel(L.ln32(x, ga, be), L.ln64(x, ga, be))
        for name, r in zip(names, rel):
            assert float(r) <= 5e-4, (C, key, name, float(r))
        dx64, _, _ = L.ln_backward64(dy, x, ga, be)
        rel = L.row_rel(L.ln_backward32(dy, x, m32, r32, ga), dx64)
        for name, r in zip(names, rel):
            assert float(r) <= 2.5e-3, (C, key, name, float(r))


def test_sat16_saturates():
    t = torch.tensor([1e9, -1e9, 65519.0, 65520.0, -70000.0, 1.0], dtype=torch.float64)
    assert L.sat16(t).tolist() == [65504.0, -65504.0, 65504.0, 65504.0, -65504.0, 1.0]
    assert torch.isinf(t.half()).sum() == 4


@pytest.mark.parametrize("rows,tile", [(512, 256), (512 + 5, 256), (256, 128), (512, 128)])
def test_layout_placement(rows, tile):
    names = L.layout(rows, tile)
    assert len(names) == rows and names[0] != L.FILLER and names[-1] != L.FILLER and names[-1] not in L.NEAR_RANGE
    for name in L.NAMES:
        at = [r for r, n in enumerate(names) if n == name]
        assert len(at) >= 2, name
        a, b = at[0], at[1]
        assert a // tile != b // tile, name                                   # different tiles
        assert a // 32 % 8 != b // 32 % 8 and a % tile // 32 != b % tile // 32, name      # different waves of a tile
        assert a % 32 != b % 32, name                                         # different lanes
    for r, n in enumerate(names[:-1]):
        if n != L.FILLER:
            assert names[r + 1] == L.FILLER, (r, n)                           # a normal row behind every family row
    if rows > 2 * tile:
        assert names[2 * tile] in L.OVERFLOW                                  # the ragged tail holds an overflow row
    x, names2 = L.rows_tensor(64, rows, tile, 3)
    fam = L.families(64, torch.Generator().manual_seed(3000 + 64))
    assert names2 == names and x.shape == (rows, 64) and torch.isfinite(x).all()
    assert all(torch.equal(x[r], fam[n]) for r, n in enumerate(names) if n != L.FILLER)
    assert float(x[[r for r, n in enumerate(names) if n == L.FILLER]].abs().max()) < 16
