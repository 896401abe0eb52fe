"""The GEMM route table on the device.  tests/test_abi_cpu.py::test_gemm_host_plan pins what `plan_gemm` decides, row by row; this file RUNS what those
rows launch where no other test does: the generic 256 x 256 tile at ragged and straddling shapes (it is picked only from m >= 16384), the three
256 x 256 fast kernels' column max with more than one shape in a tile, the 128 x 64 tile's residual / column-max / per-row-bias epilogues, the XCD
patch map on a ragged row panel, and `launch_plan`'s re-plan when there is no zero row.

Every case asserts its plan first (`pcd_gemm_plan` with the descriptor it then launches), runs on small integers -- A in [-3, 3], W in [-2, 2], biases
in [-3, 3], residuals in [-5, 5], so every fp32 partial sum is exact -- and compares with `torch.equal` against a float64 statement of the operation.
Outputs have padded rows (ldo = c + 8, ldr = c + 16) prefilled with NaN / a sentinel, and the pad must come back bit for bit; every launch runs
twice into fresh buffers.  GPU only."""
import ctypes as C
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F16, HILO, OUT32, SPLITK, RESID, COLMAX, CMW, WFRAG = range(8)             # PCD_GEMM_ENTRY_*
XP, XW = 5, 6                                                               # PCD_GEMM_FAMILY_*: gemm_xp_kernel, gemm_xw_kernel
SENTINEL32 = -123456.75                                                     # the fill of an fp32 output's rows (no result of these cases)
HILO_SCALE = 1.0 / 64                                                       # hi / lo case: a power of two folded into A keeps |out| inside fp16

# entry, m x (k1 + k2) -> c; strided: A1 / A2 are slices of wider buffers (lda1 = k1 + 64, lda2 = k2 + 128); sb_rps: rows per shape of a per-shape bias
# (0 = none); rps: rows per shape of the column max.  plan: family, tiles_m, tiles_n, grid on 256 CUs, patch_pn, patch_xn.
Case = namedtuple("Case", "name entry m k1 k2 c plan strided bias sb_rps relu rps")


def case(name, entry, m, k1, k2, c, plan, strided=False, bias=True, sb_rps=0, relu=True, rps=0):
    family, tiles_m, tiles_n, grid = plan[:4]
    return Case(name, entry, m, k1, k2, c, (family, tiles_m, tiles_n, grid) + tuple(plan[4:] or (0, 0)), strided, bias, sb_rps, relu, rps)


GENERIC_256 = [
    case("g256-f16-ragged-m", F16, 16392, 256, 0, 256, (3, 65, 1, 65)),
    case("g256-f16-ragged-c", F16, 16384, 256, 0, 264, (3, 64, 2, 128)),
    case("g256-f16-ragged-both-norelu", F16, 16584, 256, 0, 520, (3, 65, 3, 195), relu=False),
    case("g256-f16-whole-then-edge", F16, 18000, 256, 0, 1024, (3, 71, 4, 256)),        # 284 tiles on 256 workgroups
    case("g256-f16-two-strides", F16, 16384, 128, 128, 256, (3, 64, 1, 64), strided=True),          # whole tiles, refused by xp: lda2 != lda1
    case("g256-f16-shape-bias-128", F16, 16384, 256, 0, 256, (3, 64, 1, 64), bias=False, sb_rps=128),
    case("g256-f16-shape-bias-100", F16, 16400, 256, 0, 256, (3, 65, 1, 65), bias=False, sb_rps=100),
    case("g256-hilo-ragged", HILO, 16392, 128, 128, 264, (3, 65, 2, 130)),
    case("g256-residual-ragged", RESID, 16392, 256, 0, 264, (3, 65, 2, 130), relu=False),
    case("g256-out32-whole", OUT32, 16384, 256, 0, 256, (3, 64, 1, 64)),                # the fp32 epilogue has no xp form
    case("g256-out32-shape-bias-100", OUT32, 16400, 256, 0, 264, (3, 65, 2, 130), bias=False, sb_rps=100, relu=False),
    case("g256-colmax-rps64", COLMAX, 16384, 256, 0, 256, (3, 64, 1, 64), rps=64),      # fast path refused by cm_rps % 128
    case("g256-colmax-rps2000", COLMAX, 18000, 256, 0, 512, (3, 71, 2, 142), rps=2000),             # the forward's own ragged case
    case("g256-colmax-rps128-short-last", COLMAX, 16448, 256, 0, 256, (3, 65, 1, 65), rps=128),
]
FAST_256 = [
    case("xp-colmax-rps128", COLMAX, 16384, 256, 0, 256, (XP, 64, 1, 64), rps=128),     # two shapes per tile
    case("xp-colmax-rps640", COLMAX, 20480, 256, 0, 512, (XP, 80, 2, 160), rps=640),
    case("xw-colmax-rps128", CMW, 65536, 128, 0, 256, (XW, 256, 1, 256, 1, 1), rps=128),
    case("xw-colmax-rps384", CMW, 49152, 128, 0, 1024, (XW, 192, 4, 256, 4, 1), rps=384),
    case("xw-colmax-rps640", CMW, 20480, 128, 0, 4096, (XW, 80, 16, 256, 8, 2), rps=640),           # the U-Net's grid for N = 640, B = 32
]
SMALL_TILES = [
    case("t0-f16-ragged", F16, 200, 64, 0, 40, (0, 2, 1, 2)),
    case("t0-f16-shape-bias-100", F16, 300, 64, 0, 64, (0, 3, 1, 3), bias=False, sb_rps=100),
    case("t0-residual", RESID, 200, 64, 0, 64, (0, 2, 1, 2), relu=False),
    case("t0-colmax-rps100", COLMAX, 300, 64, 0, 64, (0, 3, 1, 3), rps=100),            # slow path
    case("t0-colmax-rps128", COLMAX, 384, 64, 0, 64, (0, 3, 1, 3), rps=128),            # fast path
    case("t1-f16-bias-and-shape-bias-100", F16, 300, 64, 0, 136, (1, 3, 2, 6), sb_rps=100),
    case("t1-f16-patch-map-ragged-m", F16, 16383, 64, 0, 256, (1, 128, 2, 256, 2, 1)),
]
CASES = GENERIC_256 + FAST_256 + SMALL_TILES


@pytest.fixture(scope="module")
def lib():
    from shapegen_amd import _lib
    _lib.require_gpu()
    return _lib.load()


def _ints(shape, lo, hi, seed):
    """Integers of [lo, hi] as fp32 on the device, drawn on the host from their own seed."""
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float().cuda()


def _strided(mat, extra):
    """`mat` as the leading columns of a buffer `extra` columns wider; the columns beyond hold values no case's operands have."""
    wide = torch.full((mat.shape[0], mat.shape[1] + extra), 7.0, dtype=mat.dtype, device=mat.device)
    wide[:, :mat.shape[1]] = mat
    return wide[:, :mat.shape[1]]


def _operands(cs, seed):
    """The case's device operands and the float64 statement of what it computes (before the epilogue's rounding and reduction)."""
    k = cs.k1 + cs.k2
    a = _ints((cs.m, k), -3, 3, seed)                                       # A and W from different seeds
    if cs.entry == HILO:
        w = _ints((cs.c, k), -1, 1, seed + 1) * 2049.0                      # 2049 = 2048 + 1 needs the second half
        hi = w.half()
        lo = (w.double() - hi.double()).half()
        assert not torch.equal(hi.double(), w.double()) and torch.equal(hi.double() + lo.double(), w.double())
        w_dev = torch.cat([hi, lo], 1).contiguous()
        a = a * HILO_SCALE
        assert (3 * 2049 * k + 11 / HILO_SCALE) < 2 ** 24                   # every partial sum, in units of the scale, is an exact fp32 integer
    else:
        w = _ints((cs.c, k), -2, 2, seed + 1)
        if cs.rps:
            w[::7] = 0                                                      # column max: columns whose every sum is the bias, so the zero start can win
        w_dev = w.half().contiguous()
        assert k <= 512 and 3 * 2 * k + 11 < 2 ** 24                        # |partial sum| + |bias| + |per-shape bias| + |residual|: exact in fp32
    a1, a2 = a[:, :cs.k1].half().contiguous(), (a[:, cs.k1:].half().contiguous() if cs.k2 else None)
    if cs.strided:
        a1, a2 = _strided(a1, 64), _strided(a2, 128)
        assert a1.stride(0) != a2.stride(0)
    want = a.double() @ w.double().t()
    bias = _ints((cs.c,), -3, 3, seed + 2) if cs.bias else None
    if bias is not None:
        want += bias.double()
    sb = None
    if cs.sb_rps:
        sb = _ints(((cs.m + cs.sb_rps - 1) // cs.sb_rps, cs.c), -3, 3, seed + 3)
        want += sb.double().repeat_interleave(cs.sb_rps, 0)[:cs.m]
    resid = None
    if cs.entry == RESID:
        full = _ints((cs.m, cs.c + 16), -5, 5, seed + 4).half()            # residual rows of c + 16 halfs
        resid = full[:, :cs.c]
    return a1, a2, w_dev, bias, sb, resid, want


def _desc(cs, a1, a2, w, bias, sb):
    from shapegen_amd import _lib
    d = _lib.GemmDesc()
    d.a1, d.lda1, d.k1 = a1.data_ptr(), a1.stride(0), cs.k1
    if a2 is not None:
        d.a2, d.lda2, d.k2 = a2.data_ptr(), a2.stride(0), cs.k2
    d.w, d.ldw = w.data_ptr(), w.stride(0)
    d.bias, d.shape_bias, d.rows_per_shape = _lib.ptr(bias), _lib.ptr(sb), cs.sb_rps
    d.relu, d.m, d.c = int(cs.relu), cs.m, cs.c
    return d


def _plan(lib, d, entry, rps=0, wfrag=False):
    from shapegen_amd import _lib
    pl = _lib.GemmPlan()
    _lib.check(lib.pcd_gemm_plan(d, entry, rps, 0, int(wfrag), C.byref(pl)), "gemm_plan")
    return pl


def _assert_plan(lib, cs, d):
    """The plan of the descriptor that is launched next: a later change of the heuristic must not move the case onto another kernel unnoticed."""
    pl = _plan(lib, d, cs.entry, cs.rps, cs.entry == CMW)
    family, tiles_m, tiles_n, grid, pn, xn = cs.plan
    assert (pl.family, pl.tiles_m, pl.tiles_n) == (family, tiles_m, tiles_n), (cs.name, pl.family, pl.tiles_m, pl.tiles_n)
    tiles = tiles_m * tiles_n
    if family == XW or torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert (pl.grid, pl.patch_pn, pl.patch_xn) == (grid, pn, xn), (cs.name, pl.grid, pl.patch_pn, pl.patch_xn)
    else:                                                                   # another CU count: only what holds on any device
        assert pl.grid <= tiles and (grid == tiles or pl.grid < tiles), (cs.name, pl.grid)
    if family == XP:
        assert pl.zero_shape_bias == 1 and pl.zero_bias == 0
    return pl


def _wfrag(lib, w):
    from shapegen_amd import _lib
    out = torch.empty_like(w)
    _lib.check(lib.pcd_gemm_pack_wfrag(w.data_ptr(), w.shape[1], w.shape[1], w.shape[0], out.data_ptr(), _lib.stream_ptr()), "gemm_pack_wfrag")
    return out


def _launch(lib, cs, d, resid, wfrag):
    """One launch into a fresh, prefilled output; returns the whole buffer, pad columns included."""
    from shapegen_amd import _lib
    s = _lib.stream_ptr()
    ldo = cs.c + 8
    if cs.entry in (COLMAX, CMW):
        out = torch.full(((cs.m + cs.rps - 1) // cs.rps, cs.c), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.pcd_fill_zero(out.data_ptr(), out.numel() * 4, s), "fill_zero")
        if cs.entry == COLMAX:
            _lib.check(lib.pcd_gemm_f16_colmax(d, out.data_ptr(), cs.rps, s), "gemm_f16_colmax")
        else:
            _lib.check(lib.pcd_gemm_f16_colmax_wfrag(d, wfrag.data_ptr(), out.data_ptr(), cs.rps, s), "gemm_f16_colmax_wfrag")
    elif cs.entry == OUT32:
        out = torch.full((cs.m, ldo), SENTINEL32, dtype=torch.float32, device="cuda")
        _lib.check(lib.pcd_gemm_f16_out32(d, out.data_ptr(), ldo, s), "gemm_f16_out32")
    else:
        out = torch.full((cs.m, ldo), float("nan"), dtype=torch.float16, device="cuda")
        if cs.entry == F16:
            _lib.check(lib.pcd_gemm_f16(d, out.data_ptr(), ldo, s), "gemm_f16")
        elif cs.entry == HILO:
            _lib.check(lib.pcd_gemm_f16_hilo(d, out.data_ptr(), ldo, s), "gemm_f16_hilo")
        else:
            _lib.check(lib.pcd_gemm_f16_residual(d, resid.data_ptr(), resid.stride(0), out.data_ptr(), ldo, s), "gemm_f16_residual")
    return out


def _expected(cs, want, resid):
    """The float64 statement through the entry point's epilogue."""
    lo = 0.0 if cs.relu else -65504.0
    if cs.entry in (COLMAX, CMW):
        n = (cs.m + cs.rps - 1) // cs.rps
        full = torch.zeros(n * cs.rps, cs.c, dtype=torch.float64, device=want.device)   # the last shape may be short: rows of 0 change no maximum of a ReLU
        full[:cs.m] = want.clamp_min(0)
        return full.reshape(n, cs.rps, cs.c).max(1)[0].float()
    if cs.entry == OUT32:
        return (want.clamp_min(0) if cs.relu else want).float()
    assert float(want.abs().max()) < 65504                                  # the clamp below is the kernel's, and no case leans on it
    out = want.clamp(lo, 65504.0).half()
    if cs.entry == RESID:
        out = (out.double() + resid.double()).half()                        # half(half(acc + bias) + resid)
    return out


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _check(cs, out, exp, tag):
    body = out if cs.entry in (COLMAX, CMW) else out[:, :cs.c]
    assert torch.equal(body, exp), (cs.name, tag, int((body != exp).sum()), (body != exp).nonzero()[:4].tolist())
    if cs.entry not in (COLMAX, CMW):
        pad = _bits(out[:, cs.c:])
        fill = _bits(torch.full((1,), SENTINEL32 if cs.entry == OUT32 else float("nan"), dtype=out.dtype, device=out.device))
        assert bool((pad == fill).all()), (cs.name, tag, "pad columns written")


@pytest.mark.parametrize("cs", CASES, ids=[c.name for c in CASES])
def test_route(lib, cs):
    from shapegen_amd import ops
    a1, a2, w, bias, sb, resid, want = _operands(cs, 1000 + 10 * CASES.index(cs))
    d = _desc(cs, a1, a2, w, bias, sb)
    _assert_plan(lib, cs, d)
    exp = _expected(cs, want, resid)
    if cs.entry in (COLMAX, CMW):
        assert bool((exp == 0).any()) and bool((exp > 0).any())             # the zero start wins somewhere, and loses somewhere
    elif not cs.relu:
        assert bool((exp < 0).any())                                        # negative outputs must survive
    wfrag = _wfrag(lib, w) if cs.entry == CMW else None
    first = _launch(lib, cs, d, resid, wfrag)
    second = _launch(lib, cs, d, resid, wfrag)
    _check(cs, first, exp, "first launch")
    _check(cs, second, exp, "second launch")
    assert torch.equal(_bits(first), _bits(second)), cs.name
    if cs.plan[0] in (XP, XW):
        # the same column max from the generic kernel (gemm_xp_kernel off; pcd_gemm_f16_colmax never takes gemm_xw_kernel)
        try:
            assert lib.pcd_gemm_set_config(5) == 0
            assert _plan(lib, d, COLMAX, cs.rps).family in (1, 3)
            generic = ops.gemm_f16_colmax(a1, w, bias, cs.rps)
        finally:
            assert lib.pcd_gemm_set_config(7) == 0
        assert torch.equal(_bits(generic), _bits(first)), (cs.name, int((generic != first).sum()))


def test_route_without_the_zero_row(lib):
    """pcd_gemm_f16 at 256 x 128 -> 16640 with a bias and no per-shape bias, tile 3 forced: the plan is gemm_xp_kernel with the zero row standing in for
    the per-shape bias, but the zero row has 16384 columns, so `launch_plan` finds none and re-plans onto the generic 256 x 256 kernel.  The plan
    cannot show this fallback (`pcd_gemm_plan` stops before `launch_plan`): correctness of the output is the only observable -- gemm_xp_kernel
    launched with a null per-shape bias would read through it."""
    from shapegen_amd import _lib
    cs = case("no-zero-row", F16, 256, 128, 0, 16640, (XP, 1, 65, 65))
    a1, a2, w, bias, sb, resid, want = _operands(cs, 77)
    d = _desc(cs, a1, a2, w, bias, sb)
    exp = _expected(cs, want, resid)
    try:
        assert lib.pcd_gemm_set_config(3) == 0
        pl = _assert_plan(lib, cs, d)
        assert pl.zero_shape_bias == 1 and pl.no_zero_row == 0              # NO_ZERO_GENERIC: the generic kernel of the tile
        first = _launch(lib, cs, d, resid, None)
        second = _launch(lib, cs, d, resid, None)
    finally:
        assert lib.pcd_gemm_set_config(-1) == 0
    _check(cs, first, exp, "first launch")
    _check(cs, second, exp, "second launch")
    assert torch.equal(_bits(first), _bits(second))
