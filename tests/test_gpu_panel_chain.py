"""Row-panel chains (csrc/panelchain.hip): enc4.conv1-3 (E4) and dec3.conv2-3 (D3T) of the point U-Net as one launch each, with the activations of
a 128-row panel resident in LDS between the layers.  The chains must give, bit for bit, what one GEMM launch per layer gives: the same fp16 products
summed in fp32 in the same k order, one bias + ReLU + fp16 rounding per layer.

Shapes are the smallest at which the kernel can go wrong: one tile (m = 128); m = 640 with at most 2 workgroups, so that one workgroup walks 3 tiles and
the other 2 (the tile hand-over, the weight look-ahead across it, the panel request behind the last pass, the last-tile path); m = 640 with one
workgroup per tile; m = 384 and 1280 against the per-layer launches."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# [C][K] of the layers of a chain, and the width of its output
SHAPES = {0: [(512, 512), (512, 512), (1024, 512)], 1: [(512, 512), (256, 512)]}


def _lib_():
    from shapegen_amd import _lib
    return _lib, _lib.load()


def _frag(lib, _lib, w):
    """pcd_gemm_pack_wfrag's copy of w [c][k]"""
    out = torch.empty_like(w)
    _lib.check(lib.pcd_gemm_pack_wfrag(w.data_ptr(), w.shape[1], w.shape[1], w.shape[0], out.data_ptr(), _lib.stream_ptr()))
    return out


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


def _chain(lib, _lib, chain, x, frags, biases, cap, hilo=0, m=None, out=None):
    m = x.shape[0] if m is None else m
    if out is None:
        out = torch.full((x.shape[0], SHAPES[chain][-1][0]), -1.0, dtype=torch.float16, device="cuda")
    rc = lib.pcd_panel_chain(chain, x.data_ptr(), m, _ptrs(frags), _ptrs(biases), hilo, out.data_ptr(), out.shape[1], cap, _lib.stream_ptr())
    return rc, out


@pytest.fixture(scope="module")
def integer_chains():
    """Small-integer weights, biases and inputs (the recipe of test_wide_chain_exact_on_integers): every product and sum is exact in fp16 / fp32, so the
    result equals the float64 chain of relu(x W^T + b) exactly.  One 640-row problem per chain; the smaller cases are its leading rows."""
    _lib, lib = _lib_()
    made = {}
    for chain in (0, 1):
        g = torch.Generator().manual_seed(40 + chain)
        ws = [torch.randint(-1, 2, s_, generator=g).float() * (torch.rand(s_, generator=g) < 0.06).float() for s_ in SHAPES[chain]]
        bs = [torch.randint(-2, 3, (s_[0],), generator=g).float() for s_ in SHAPES[chain]]
        x = torch.randint(0, 3, (640, 512), generator=g).float()
        a = x.double()
        for w, b in zip(ws, bs):
            a = torch.relu(a @ w.double().T + b.double())
            assert float(a.max()) < 2048                                   # exactly representable in fp16
        assert 0.2 < float((a > 0).double().mean()) < 0.8
        dw = [w.half().cuda().contiguous() for w in ws]
        made[chain] = (x.half().cuda(), [_frag(lib, _lib, w) for w in dw], [b.cuda().contiguous() for b in bs], a)
    return made


@pytest.mark.parametrize("m,cap", [(128, 256), (640, 2), (640, 256)])
@pytest.mark.parametrize("chain", [0, 1])
def test_panel_chain_exact_on_integers(integer_chains, chain, m, cap):
    _lib, lib = _lib_()
    x, frags, biases, want = integer_chains[chain]
    rc, out = _chain(lib, _lib, chain, x[:m].contiguous(), frags, biases, cap)
    _lib.check(rc)
    assert torch.equal(out.double().cpu(), want[:m])


@pytest.mark.parametrize("m", [384, 1280])
@pytest.mark.parametrize("chain", [0, 1])
def test_panel_chain_bitwise_against_per_layer_launches(chain, m):
    """Unit-variance inputs, weights of the forward's scale (He: std sqrt(2 / K)), biases of a tenth: the chain against the same layers through
    pcd_gemm_f16 with ReLU."""
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(500 + 10 * chain + m)
    ws = [(torch.randn(s_, generator=g) * (2.0 / s_[1]) ** 0.5).half().cuda() for s_ in SHAPES[chain]]
    bs = [(0.1 * torch.randn(s_[0], generator=g)).cuda() for s_ in SHAPES[chain]]
    x = torch.randn(m, 512, generator=g).half().cuda()
    a = x
    for w, b in zip(ws, bs):
        d = _lib.GemmDesc()
        d.a1, d.lda1, d.k1 = a.data_ptr(), a.shape[1], a.shape[1]
        d.w, d.ldw, d.bias, d.relu, d.m, d.c = w.data_ptr(), w.shape[1], b.data_ptr(), 1, m, w.shape[0]
        nxt = torch.empty(m, w.shape[0], dtype=torch.float16, device="cuda")
        _lib.check(lib.pcd_gemm_f16(C.byref(d), nxt.data_ptr(), w.shape[0], _lib.stream_ptr()))
        a = nxt
    rc, out = _chain(lib, _lib, chain, x, [_frag(lib, _lib, w) for w in ws], bs, 256)
    _lib.check(rc)
    assert torch.isfinite(out).all() and float((out > 0).float().mean()) > 0.2
    if chain == 0:                                       # the two passes of enc4.conv3
        assert torch.equal(out[:, :512], a[:, :512])
        assert torch.equal(out[:, 512:], a[:, 512:])
    assert torch.equal(out, a)


@pytest.mark.parametrize("chain", [0, 1])
def test_panel_chain_refusals(integer_chains, chain):
    """m % 128 != 0, a null fragment copy and a hi / lo layer: an error code, and nothing written."""
    _lib, lib = _lib_()
    x, frags, biases, _ = integer_chains[chain]
    out = torch.full((640, SHAPES[chain][-1][0]), -1.0, dtype=torch.float16, device="cuda")
    assert _chain(lib, _lib, chain, x, frags, biases, 256, m=100, out=out)[0] != 0
    assert _chain(lib, _lib, chain, x, [frags[0], None] + frags[2:], biases, 256, out=out)[0] != 0
    assert _chain(lib, _lib, chain, x, frags, biases, 256, hilo=2, out=out)[0] != 0
    torch.cuda.synchronize()
    assert bool((out == -1).all())


@pytest.fixture(scope="module")
def model():
    from helpers import point_sd
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=512)
    m.load_state_dict(point_sd(), strict=True)
    return m.to("cuda").eval()


def _forward(model, x, t, B, N):
    model.model.capture_decoder(B, N)
    try:
        eps = model.model(x, t).clone()
        return eps, model.model.tap("x4", B, N).clone(), model.model.tap("d3", B, N).clone()
    finally:
        model.model.capture_decoder(B, N, on=False)


@pytest.mark.parametrize("B,N", [(2, 512), (5, 512), (3, 100)])
def test_panel_chains_in_the_forward(model, B, N):
    """pcd_unet_forward with the row-panel chains on (default, 3) and off (7: everything else stays on): eps, x4 and dec3's output bit for bit.  B = 3,
    N = 100 is a ragged m: both settings run the per-layer sequence."""
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(B * 1000 + N)
    x = torch.randn(B, N, 3, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    try:
        _lib.check(lib.pcd_unet_config(3))
        on = _forward(model, x, t, B, N)
        plain_on = model.model(x, t).clone()             # without the capture dec2 + dec1.conv1 run as one launch, on the swapped buffers
        _lib.check(lib.pcd_unet_config(7))
        off = _forward(model, x, t, B, N)
        plain_off = model.model(x, t).clone()
    finally:
        _lib.check(lib.pcd_unet_config(3))
    assert torch.isfinite(on[0]).all()
    for a, b, name in zip(on, off, ("eps", "x4", "d3")):
        assert torch.equal(a, b), name
    assert torch.equal(plain_on, plain_off) and torch.equal(plain_on, on[0])
