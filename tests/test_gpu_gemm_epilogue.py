"""The epilogues of the 256 x 256 GEMM kernels, value by value: the clamp-and-pack of the store epilogues at every fp16 rounding and saturation edge,
gemm_xs_kernel's output placement (direct and dripped chunks, line-aligned rows and rows that are not), and the column-max epilogue that adds the bias
after the maximum.  GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def ops():
    from shapegen_amd import ops as o, _lib
    _lib.require_gpu()
    return o


def _wfrag(w):
    from shapegen_amd import _lib
    wfrag = torch.empty_like(w)
    _lib.check(_lib.load().pcd_gemm_pack_wfrag(w.data_ptr(), w.shape[1], w.shape[1], w.shape[0], wfrag.data_ptr(), _lib.stream_ptr()))
    return wfrag


def _crafted():
    pos = [0.0, 1e-45, 1e-40, 1e-30, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2049.0, 2051.0,
           65504.0, 65519.99, 65520.0, 1e6, float("inf")]
    return torch.tensor(pos + [-v for v in pos], dtype=torch.float32)


@pytest.mark.parametrize("entry", ["f16", "wfrag"])
@pytest.mark.parametrize("relu", [1, 0])
def test_clamp_and_pack_exact(ops, entry, relu):
    """Zero activations: the accumulators are +0 and the store epilogue sees exactly fl(bias + per-shape bias), crafted to sit on every edge of the clamp
    and of the fp32 -> fp16 rounding: +-0, fp32 and fp16 denormals, -1e-30, ties of the fp16 grid (2^-25, 3 * 2^-25, 1 + 2^-11, 1 + 3 * 2^-11, 2049, 2051),
    65504, 65519.99 (rounds down to 65504), 65520 (the tie that rounds to inf), 1e6, +-inf.  The output is, bit for bit and with the sign of zero, the
    CPU statement: torch.clamp in fp32, then .half().  Through pcd_gemm_f16 at 256 x 256 (the generic kernel) and pcd_gemm_f16_wfrag at 65536 x 384 -> 256
    (gemm_xs_kernel).  A NaN sum comes out as the LOWER bound of the clamp (0 with ReLU, -65504 without): what v_med3_f32 makes of it, pinned here."""
    from shapegen_amd import _lib
    lib = _lib.load()
    m, k, c, rps = (256, 64, 256, 128) if entry == "f16" else (65536, 384, 256, 256)
    vals = torch.cat([_crafted(), torch.tensor([float("nan")])])
    nv, shapes = len(vals), m // rps
    col = torch.arange(c)
    # even columns: value j % nv in the bias, the per-shape bias 0; odd columns: value (j + s) % nv in shape s's row of the per-shape bias, the bias 0
    even = col % 2 == 0
    bias = torch.where(even, vals[col % nv], torch.zeros(c))
    sb = torch.where(even[None, :], torch.zeros(shapes, c), vals[(col[None, :] + torch.arange(shapes)[:, None]) % nv])
    sums = torch.zeros(shapes, c) + (bias[None, :] + sb)                    # what the kernel forms: acc (+0) + (bias + per-shape bias), fp32
    assert set(sums[~sums.isnan()].tolist()) >= set(_crafted()[_crafted() != 0].tolist())      # every crafted value is really presented
    lo = 0.0 if relu else -65504.0
    want = torch.clamp(sums, lo, 65504.0).half()
    want[sums.isnan()] = lo                                                 # pinned: NaN -> the lower bound
    a = torch.zeros(m, k, dtype=torch.float16, device="cuda")
    w = torch.randint(-2, 3, (c, k), generator=torch.Generator().manual_seed(1)).half().cuda()
    bias_d, sb_d = bias.cuda(), sb.cuda()                                   # (the descriptor holds addresses only)
    d = ops._desc(a, w, bias_d, None, sb_d, rps, relu=bool(relu))
    out = torch.full((m, c), float("nan"), dtype=torch.float16, device="cuda")
    if entry == "f16":
        _lib.check(lib.pcd_gemm_f16(d, out.data_ptr(), c, _lib.stream_ptr()), "gemm_f16")
    else:
        plan = _lib.GemmPlan()
        _lib.check(lib.pcd_gemm_plan(d, 7, 0, 1, 1, plan), "gemm_plan")
        assert plan.family == 7                                             # gemm_xs_kernel
        _lib.check(lib.pcd_gemm_f16_wfrag(d, _wfrag(w).data_ptr(), out.data_ptr(), c, _lib.stream_ptr()), "gemm_f16_wfrag")
    got = out.cpu().view(torch.int16).reshape(shapes, rps, c)
    wb = want.view(torch.int16)
    bad = (got != wb[:, None, :]).any(1)
    assert not bad.any(), [(float(sums[s, j]), hex(int(got[s, 0, j]) & 0xffff), hex(int(wb[s, j]) & 0xffff)) for s, j in bad.nonzero().tolist()[:8]]


@pytest.fixture(scope="module")
def store_operands():
    g = torch.Generator(device="cuda").manual_seed(21)
    m = 65536
    a1 = torch.randn(m, 768, generator=g, device="cuda").clamp_min(0).half()
    a2 = torch.randn(m, 384, generator=g, device="cuda").half()
    w = (torch.randn(512, 768, generator=g, device="cuda") / 16).half()
    bias = torch.randn(512, generator=g, device="cuda") * 0.1
    return a1, a2, w, bias


@pytest.mark.parametrize("k1,k2,c,pad", [(384, 0, 256, 0), (384, 0, 512, 0), (768, 0, 256, 0), (768, 0, 512, 0), (384, 384, 512, 0), (384, 0, 512, 8),
                                         (768, 0, 512, 8)])
def test_store_kernel_output_placement(ops, store_operands, k1, k2, c, pad):
    """gemm_xs_kernel writes every element of the output once, in its place, and nothing else: random fp16 operands (every bit of the fp32 sums
    matters), an output prefilled with NaN, three launches, bitwise pcd_gemm_f16's output.  6 K tiles (two parked chunks leave per K tile) and 12 (one);
    C 256 (one tile per workgroup: all sixteen chunks of a wave stored from the epilogue) and 512 (two: the first tile drips, the last stores all
    sixteen); two K sources once; and a row stride of c + 8 halfs -- rows that do not start on a 128-byte line -- where the columns beyond c stay NaN."""
    from shapegen_amd import _lib
    lib = _lib.load()
    a1f, a2f, wf, biasf = store_operands
    m = a1f.shape[0]
    a1 = a1f[:, :k1].contiguous()
    a2 = a2f[:, :k2].contiguous() if k2 else None
    w = wf[:c, :k1 + k2].contiguous()
    bias = biasf[:c].contiguous()
    d = ops._desc(a1, w, bias, a2, relu=True)
    plan = _lib.GemmPlan()
    _lib.check(lib.pcd_gemm_plan(d, 7, 0, 1, 1, plan), "gemm_plan")
    assert plan.family == 7 and plan.instance == (0 if k1 + k2 >= 768 else 4)
    ref = ops.gemm_f16(a1, w, bias, a2, relu=True)
    wfrag = _wfrag(w)
    ldo = c + pad
    for rep in range(3):
        out = torch.full((m, ldo), float("nan"), dtype=torch.float16, device="cuda")
        _lib.check(lib.pcd_gemm_f16_wfrag(d, wfrag.data_ptr(), out.data_ptr(), ldo, _lib.stream_ptr()), "gemm_f16_wfrag")
        assert torch.equal(out[:, :c], ref), (rep, int((out[:, :c] != ref).any(1).sum()))
        assert bool(out[:, c:].isnan().all())


@pytest.mark.parametrize("rps", [256, 2048])
def test_colmax_bias_after_max(ops, rps):
    """The column-max epilogue of gemm_xw_kernel and gemm_xp_kernel takes the maximum of the accumulators first and adds the bias once: because
    fl(x + b) is monotone in x the result is, bit for bit, max(0, max over the shape's rows of fl(acc + b)).  Integer operands (the accumulators are
    exact) and non-integer fp32 biases (the add rounds), at the smallest shape gemm_xw_kernel takes: 65536 x 128 -> 256, shapes of 256 and 2048 rows."""
    from shapegen_amd import _lib
    lib = _lib.load()
    m, k, c = 65536, 128, 256
    g = torch.Generator(device="cuda").manual_seed(31 + rps)
    a = torch.randint(-3, 4, (m, k), generator=g, device="cuda").half()
    w = torch.randint(-2, 3, (c, k), generator=g, device="cuda").half()
    bias = torch.randn(c, generator=g, device="cuda") * 7.3 + 0.1
    bias[::5] -= 900.0                                                      # some columns whose every sum is negative: the zero wins
    acc = a.float() @ w.float().t()
    assert float(acc.abs().max()) < 2 ** 24
    want = (acc + bias).clamp_min(0).reshape(-1, rps, c).max(1)[0]
    assert bool((want == 0).any()) and bool((want != want.round()).any())
    d = ops._desc(a, w, bias, relu=True)
    plan = _lib.GemmPlan()
    _lib.check(lib.pcd_gemm_plan(d, 6, rps, 1, 1, plan), "gemm_plan")
    assert plan.family == 6                                                 # gemm_xw_kernel
    out = torch.zeros(m // rps, c, dtype=torch.float32, device="cuda")
    _lib.check(lib.pcd_gemm_f16_colmax_wfrag(d, _wfrag(w).data_ptr(), out.data_ptr(), rps, _lib.stream_ptr()), "gemm_f16_colmax_wfrag")
    lds = ops.gemm_f16_colmax(a, w, bias, rps)
    assert torch.equal(out, want), int((out != want).sum())
    assert torch.equal(lds, want), int((lds != want).sum())
    assert torch.equal(out.view(torch.int32), lds.view(torch.int32))
