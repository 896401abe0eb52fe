"""The narrow ends of the point denoiser on the register-resident engine (csrc/widechain.hip, pw_wide_ends_kernel):
  E23 = enc2.conv1-3 + enc3.conv1-3 (x1 -> x2 stored and kept in registers -> x3),
  D21 = dec2.conv1-3 + dec1.conv1 ([dec3 out | x2] -> ... -> [registers | x1] -> 128 channels),
each with its narrow layer (enc2.conv3 / dec1.conv1) in plain fp16 or as hi | lo weights; and the pooled product reading its fp32 maxima directly.

Exactness argument of the integer tests: weights are a + b 2^-13 with a, b in {-1, 0, 1} (b = 0 without hi / lo), biases small integers, inputs in
{0, 1, 2}.  Every product is then a multiple of 2^-13, and so is every layer output after its fp16 rounding (rounding only coarsens the grid; 2^-13 is a
normal fp16 number).  A sum of multiples of 2^-13 whose every partial sum is below 2048 = 2^11 in magnitude needs at most 24 bits: it is exact in fp32 in
ANY order.  sum |w| |x| + |b| < 2048 is checked on the CPU for every layer, so the kernel must return fp16(exact value) for every layer, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import point_sd, rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EPS_TOL = 3e-3                     # tests/test_gpu_point.py
TILE, GRID_CAP = 256, 256          # rows per tile and the launch code's grid cap (csrc/widechain.hip)
SHAPES = {0: [(128, 128), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256)],      # (C, K) of E23's layers
          1: [(256, 512), (256, 256), (128, 256), (128, 256)]}                              # ... of D21's
NARROW = {0: 2, 1: 3}              # the layer that may carry hi | lo weights
SIZES = (TILE, TILE * (GRID_CAP + 1))
PERIOD = 3 * TILE                  # distinct rows of the integer cases: row r repeats row r % PERIOD, so tile T looks like tile T % 3 (the float64 chain stays small)


def _lib_():
    from shapegen_amd import _lib
    return _lib, _lib.load()


def _pack(chain, hilo, ws, bs):
    """ws: float64 [C][K] per layer -> the chain's packed images on the device (hi | lo for the narrow layer when `hilo`)"""
    from shapegen_amd import packing
    _lib, lib = _lib_()
    dw = []
    for i, w in enumerate(ws):
        if hilo and i == NARROW[chain]:
            dw.append(torch.from_numpy(packing.split_hilo(w.numpy())).cuda().contiguous())
        else:
            dw.append(w.half().cuda().contiguous())
    db = [b.float().cuda().contiguous() for b in bs]
    packed = torch.empty(int(lib.pcd_pw_wide_ends_packed_bytes(chain, hilo)), dtype=torch.uint8, device="cuda")
    wp = (C.c_void_p * len(dw))(*[t.data_ptr() for t in dw])
    bp = (C.c_void_p * len(db))(*[t.data_ptr() for t in db])
    _lib.check(lib.pcd_pw_wide_ends_pack(chain, hilo, wp, bp, packed.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()       # (dw, db may go once the images are built)
    return packed


def _run(chain, hilo, packed, ins, m=None):
    """ins: fp16 device tensors (x1,) for E23 / (dec3 out, x2, x1) for D21 -> (x3, x2) / (out,); NaN-filled outputs"""
    _lib, lib = _lib_()
    m = ins[0].shape[0] if m is None else m
    nan = lambda c: torch.full((ins[0].shape[0], c), float("nan"), dtype=torch.float16, device="cuda")
    if chain == 0:
        x3, x2 = nan(512), nan(256)
        rc = lib.pcd_pw_wide_ends(0, hilo, ins[0].data_ptr(), 0, 0, m, packed.data_ptr(), x3.data_ptr(), x2.data_ptr(), _lib.stream_ptr())
        return rc, (x3, x2)
    out = nan(128)
    rc = lib.pcd_pw_wide_ends(1, hilo, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), m, packed.data_ptr(), out.data_ptr(), 0, _lib.stream_ptr())
    return rc, (out,)


def _integer_case(chain, hilo):
    """weights, biases, PERIOD rows of inputs and their exact expected outputs (float64 holding fp16 values)"""
    g = torch.Generator().manual_seed(900 + 10 * chain + hilo)
    sparse = lambda s_, p: torch.randint(-1, 2, s_, generator=g).double() * (torch.rand(s_, generator=g) < p).double()
    ws = [sparse(s_, 0.08 if s_[1] == 128 else 0.04) for s_ in SHAPES[chain]]      # (denser, and six layers of growth pass 2048)
    if hilo:
        n = NARROW[chain]
        a, b = ws[n], sparse(SHAPES[chain][n], 0.25)
        ws[n] = a + b * 2.0 ** -13
        from shapegen_amd import packing
        hl = packing.split_hilo(ws[n].numpy()).astype(np.float64)
        k = a.shape[1]
        nz = a.numpy() != 0
        assert np.array_equal(hl[:, :k][nz], a.numpy()[nz]) and np.array_equal(hl[:, k:][nz], (b.numpy() * 2.0 ** -13)[nz])     # hi = a, lo = b 2^-13
        assert np.array_equal(hl[:, :k] + hl[:, k:], ws[n].numpy()) and (b.numpy()[nz] != 0).sum() > 100
    bs = [torch.randint(-2, 3, (s_[0],), generator=g).double() for s_ in SHAPES[chain]]
    widths = (128,) if chain == 0 else (256, 256, 128)
    ins = [torch.randint(0, 3, (PERIOD, c), generator=g).double() for c in widths]

    def layer(a, i):
        w, b = ws[i], bs[i]
        assert float((a.abs() @ w.abs().T + b.abs()).max()) < 2048          # every partial sum, in any order, stays exact in fp32
        return torch.relu(a @ w.T + b).half().double()                      # one fp16 rounding per layer
    if chain == 0:
        a = ins[0]
        for i in range(3):
            a = layer(a, i)
        x2 = a
        for i in range(3, 6):
            a = layer(a, i)
        want = (a, x2)
    else:
        a = torch.cat([ins[0], ins[1]], 1)
        for i in range(3):
            a = layer(a, i)
        want = (layer(torch.cat([a, ins[2]], 1), 3),)
    for t in want:
        assert float((t != 0).double().mean()) > 0.05                       # (the case is not a chain of dead layers)
    return ws, bs, ins, want


@pytest.mark.parametrize("hilo", [0, 1])
@pytest.mark.parametrize("chain", [0, 1])
def test_ends_exact_on_integers(chain, hilo):
    """Both chains, with and without hi / lo weights on the narrow layer, at one tile and at grid cap + 1 tiles (one workgroup walks two tiles, the ring
    wraps across them): the outputs equal the float64 chain of fp16(relu(x W^T + b)) exactly (see the module docstring)."""
    ws, bs, ins, want = _integer_case(chain, hilo)
    packed = _pack(chain, hilo, ws, bs)
    for rows in SIZES:
        idx = torch.arange(rows) % PERIOD
        rc, got = _run(chain, hilo, packed, [t[idx].half().cuda() for t in ins])
        assert rc == 0
        for gt, wt in zip(got, want):
            assert torch.equal(gt.cpu(), wt[idx].half()), (chain, hilo, rows)


@pytest.mark.parametrize("hilo", [0, 1])
@pytest.mark.parametrize("chain", [0, 1])
def test_ends_request_forms_bitwise(chain, hilo):
    """Who requests a piece of a weight image (every wave its share / one wave of each SIMD) does not enter the arithmetic: same bits, on random data,
    at one tile and at grid cap + 1 tiles."""
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(77 + 10 * chain + hilo)
    ws = [(torch.randn(s_, generator=g) / s_[1] ** 0.5).double() for s_ in SHAPES[chain]]
    bs = [torch.randn(s_[0], generator=g) * 0.1 for s_ in SHAPES[chain]]
    packed = _pack(chain, hilo, ws, bs)
    widths = (128,) if chain == 0 else (256, 256, 128)
    for rows in SIZES:
        ins = [torch.randn(rows, c, generator=g).clamp_min(0).half().cuda() for c in widths]
        try:
            _lib.check(lib.pcd_pw_wide_config(1))
            rc_a, a = _run(chain, hilo, packed, ins)
            _lib.check(lib.pcd_pw_wide_config(0))
            rc_b, b = _run(chain, hilo, packed, ins)
        finally:
            _lib.check(lib.pcd_pw_wide_config(1))
        assert rc_a == 0 and rc_b == 0
        for ta, tb in zip(a, b):
            assert torch.isfinite(ta).all() and float(ta.float().abs().max()) > 0
            assert torch.equal(ta, tb), (chain, hilo, rows)


@pytest.mark.parametrize("chain", [0, 1])
def test_ends_refuse_ragged_rows(chain):
    """M not a multiple of 256 is an error and nothing is launched: the NaN-filled outputs stay as they were."""
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(5)
    ws = [torch.randn(s_, generator=g).double() * 0.05 for s_ in SHAPES[chain]]
    bs = [torch.zeros(s_[0]) for s_ in SHAPES[chain]]
    packed = _pack(chain, 0, ws, bs)
    widths = (128,) if chain == 0 else (256, 256, 128)
    ins = [torch.rand(512, c, generator=g).half().cuda() for c in widths]
    for m in (100, 257, 511, 0):
        rc, outs = _run(chain, 0, packed, ins, m=m)
        torch.cuda.synchronize()
        assert rc != 0 and b"bad argument" in lib.pcd_last_error()
        assert all(bool(torch.isnan(t).all()) for t in outs)
    assert lib.pcd_pw_wide_ends_packed_bytes(2, 0) == 0
    assert lib.pcd_pw_wide_ends_packed_bytes(chain, 1) > lib.pcd_pw_wide_ends_packed_bytes(chain, 0) > 0


@pytest.fixture(scope="module")
def model():
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=512)
    m.load_state_dict(point_sd(), strict=True)
    return m.to("cuda").eval()


def test_ends_in_the_forward(model):
    """pcd_unet_forward on whole tiles runs E23 and D21 (default) against pcd_unet_config(1), one GEMM launch per layer for the same ten layers: the same
    fp16 operands, fp32 sums in another order, one fp16 rounding per layer either way (the bound of test_wide_chains_in_the_forward); and against the oracle."""
    from oracle import torch_oracle as O
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(78)
    x = torch.randn(2, 512, 3, generator=g)
    t = torch.rand(2, generator=g)
    net = model.model
    eps = net(x.cuda(), t.cuda()).clone()
    x2, x3 = net.tap("x2", 2, 512).clone(), net.tap("x3", 2, 512).clone()
    _lib.check(lib.pcd_unet_config(1))
    try:
        eps_l = net(x.cuda(), t.cuda()).clone()
        x2_l, x3_l = net.tap("x2", 2, 512).clone(), net.tap("x3", 2, 512).clone()
    finally:
        _lib.check(lib.pcd_unet_config(3))
    figures = {"x2": rel_l2(x2.float().cpu(), x2_l.float().cpu()), "x3": rel_l2(x3.float().cpu(), x3_l.float().cpu()),
               "eps": rel_l2(eps.cpu(), eps_l.cpu()), "eps v. oracle": rel_l2(eps.cpu(), O.unet_pointnet_large(point_sd(), "model.", x, t))}
    print(figures)
    assert torch.isfinite(eps).all()
    assert figures["x2"] < 1e-3 and figures["x3"] < 1e-3 and figures["eps"] < 1e-3
    assert figures["eps v. oracle"] < EPS_TOL
    # a capture of dec2's output runs D2 and dec1.conv1 apart (the tensor does not exist inside D21): d2 is there, eps moves by a reordering at the most
    net.capture_decoder(2, 512)
    try:
        eps_c = net(x.cuda(), t.cuda()).clone()
        d2 = net.tap("d2", 2, 512).clone()
    finally:
        net.capture_decoder(2, 512, on=False)
    assert torch.isfinite(d2).all() and float(d2.float().abs().max()) > 0
    assert rel_l2(eps_c.cpu(), eps.cpu()) < 1e-3


def test_forward_fallback_is_bitwise_on_ragged_tiles(model):
    """(3, 100): m is no multiple of 256, so the default configuration runs exactly what pcd_unet_config(1) runs."""
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(79)
    x, t = torch.randn(3, 100, 3, generator=g).cuda(), torch.rand(3, generator=g).cuda()
    eps3 = model.model(x, t).clone()
    _lib.check(lib.pcd_unet_config(1))
    try:
        eps1 = model.model(x, t).clone()
    finally:
        _lib.check(lib.pcd_unet_config(3))
    assert torch.isfinite(eps3).all() and torch.equal(eps3, eps1)


def test_pooled_product_reads_fp32_maxima(model):
    """gbias = fp16(pooled) . wg^T + folded bias with the fp32 -> fp16 rounding done inside the split-K kernel: the same bits as the conversion pass
    followed by the fp16 split-K kernel and its finish (what the forward ran before), and the config-independent statement of the same product through
    pcd_gemm_f16_out32 within fp32 summation order."""
    _lib, lib = _lib_()
    st = _lib.stream_ptr()
    g = torch.Generator().manual_seed(80)
    x, t = torch.randn(2, 512, 3, generator=g).cuda(), torch.rand(2, generator=g).cuda()
    net = model.model
    net(x, t)
    pooled, gbias = net.tap("pooled", 2, 512).clone(), net.tap("gbias", 2, 512).clone()
    pk = net._ensure_packed()
    wg, b13 = pk["wg"], pk["b13"]
    p16 = torch.empty(2, 4096, dtype=torch.float16, device="cuda")
    _lib.check(lib.pcd_f32_to_f16(pooled.data_ptr(), p16.data_ptr(), pooled.numel(), st))
    assert torch.equal(p16, pooled.clamp(-65504, 65504).half())
    slabs = torch.empty(int(lib.pcd_skinny_slabs(4096, 1024)), 2, 1024, dtype=torch.float32, device="cuda")
    want = torch.empty(2, 1024, dtype=torch.float32, device="cuda")
    _lib.check(lib.pcd_skinny_gemm_f16(p16.data_ptr(), 4096, 0, 0, wg.data_ptr(), 4096, 2, 1024, slabs.data_ptr(), st))
    _lib.check(lib.pcd_skinny_finish(slabs.data_ptr(), slabs.shape[0], 2, 1024, b13.data_ptr(), 0, 2, 8, 0, 0, 0, want.data_ptr(), st))
    d = _lib.GemmDesc()
    d.a1, d.lda1, d.k1 = p16.data_ptr(), 4096, 4096
    d.w, d.ldw, d.bias = wg.data_ptr(), 4096, b13.data_ptr()
    d.relu, d.m, d.c = 0, 2, 1024
    dense = torch.empty(2, 1024, dtype=torch.float32, device="cuda")
    _lib.check(lib.pcd_gemm_f16_out32(C.byref(d), dense.data_ptr(), 1024, st))
    print({"gbias v. conversion pass + fp16 split-K, max abs": float((gbias - want).abs().max()),
           "gbias v. pcd_gemm_f16_out32, max abs": float((gbias - dense).abs().max()), "split-K pair v. out32": float((want - dense).abs().max())})
    assert torch.isfinite(gbias).all() and float(gbias.abs().max()) > 0
    assert torch.equal(gbias, want)
    # the dense kernel sums the same 4096 fp16 products of a row in one fp32 chain, the split-K pair in 8 x 4 partial chains: both within
    # 4096 * 2^-24 of sum |pooled| |w| of the exact value (fp32 accumulation, worst case)
    bound = 2 * 4096 * 2.0 ** -24 * (p16.float().abs() @ wg.float().abs().T + b13.abs())
    assert bool(((gbias - dense).abs() <= bound).all())
    # the entry point on its own, at a row count of each tile count of the kernel (1, 2, 4, 8 tiles of 32 rows) and a ragged one
    for rows in (1, 33, 100, 256):
        a = (torch.randn(rows, 4096, generator=g) * 3).cuda()
        a[0, 0], a[rows - 1, 5] = 1e6, -1e6                               # saturate, like pcd_f32_to_f16
        a16 = torch.empty(rows, 4096, dtype=torch.float16, device="cuda")
        _lib.check(lib.pcd_f32_to_f16(a.data_ptr(), a16.data_ptr(), a.numel(), st))
        s_a = torch.full((slabs.shape[0], rows, 1024), float("nan"), dtype=torch.float32, device="cuda")
        s_b = torch.full_like(s_a, float("nan"))
        _lib.check(lib.pcd_skinny_gemm_f16(a16.data_ptr(), 4096, 0, 0, wg.data_ptr(), 4096, rows, 1024, s_a.data_ptr(), st))
        _lib.check(lib.pcd_skinny_gemm_f32in(a.data_ptr(), 4096, wg.data_ptr(), 4096, rows, 1024, s_b.data_ptr(), st))
        assert torch.isfinite(s_b).all() and torch.equal(s_a, s_b), rows
