"""D43 (csrc/panelchain.hip, pcd_panel_chain_dec): dec4.conv3, dec3.conv1-3 (lin 15, 16, 17, 18) of the point U-Net as one launch.  The two K = 1024
layers read K tiles 0-7 from the LDS-resident panel while K tiles 8-15 (columns 512 .. 1023 of the input; x3) roll into the images already read, and the
last pass of a tile rolls the next tile's panel in.  The chain must give, bit for bit, what one GEMM launch per layer gives.

Shapes as in test_gpu_panel_chain.py: one tile (m = 128); m = 640 with at most 2 workgroups (one walks 3 tiles, the other 2: the rolled next-tile panel
across the hand-over, the weight look-ahead, the last-tile path); m = 640 with one workgroup per tile; m = 384 and 1280 against the per-layer launches."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# [C][K] of lin 15, 16, 17, 18
SHAPES = [(512, 1024), (512, 1024), (512, 512), (256, 512)]


def _lib_():
    from shapegen_amd import _lib
    return _lib, _lib.load()


def _frag(lib, _lib, w):
    out = torch.empty_like(w)
    _lib.check(lib.pcd_gemm_pack_wfrag(w.data_ptr(), w.shape[1], w.shape[1], w.shape[0], out.data_ptr(), _lib.stream_ptr()))
    return out


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


def _chain(lib, _lib, x, x3, frags, biases, cap, hilo=0, m=None, out=None):
    m = x.shape[0] if m is None else m
    if out is None:
        out = torch.full((x.shape[0], 256), -1.0, dtype=torch.float16, device="cuda")
    out_ptr = out if isinstance(out, int) else out.data_ptr()
    rc = lib.pcd_panel_chain_dec(x.data_ptr(), x3.data_ptr(), m, _ptrs(frags), _ptrs(biases), hilo, out_ptr, 256, cap, _lib.stream_ptr())
    return rc, out


def _float64_chain(x, x3, ws, bs):
    """relu(. W^T + b) through the four layers in float64; lin 16 reads [lin 15's output | x3].  Returns every layer's output."""
    outs = []
    a = x.double()
    for i, (w, b) in enumerate(zip(ws, bs)):
        if i == 1:
            a = torch.cat([a, x3.double()], dim=1)
        a = torch.relu(a @ w.double().T + b.double())
        outs.append(a)
    return outs


@pytest.fixture(scope="module")
def integer_chains():
    """Small-integer weights (density 0.04), biases and inputs: every product and sum is exact in fp16 / fp32, so the result equals the float64 chain
    exactly.  One 640-row problem per seed; the smaller cases are its leading rows."""
    _lib, lib = _lib_()
    made = {}
    for seed in (42, 43):
        g = torch.Generator().manual_seed(seed)
        ws = [torch.randint(-1, 2, s_, generator=g).float() * (torch.rand(s_, generator=g) < 0.04).float() for s_ in SHAPES]
        bs = [torch.randint(-2, 3, (s_[0],), generator=g).float() for s_ in SHAPES]
        x = torch.randint(0, 3, (640, 1024), generator=g).float()
        x3 = torch.randint(0, 3, (640, 512), generator=g).float()
        outs = _float64_chain(x, x3, ws, bs)
        for a in outs:
            assert float(a.max()) < 2048                                   # exactly representable in fp16
            assert 0.45 < float((a > 0).double().mean()) < 0.52               # about half of every layer's outputs pass its ReLU
        dw = [w.half().cuda().contiguous() for w in ws]
        made[seed] = (x.half().cuda(), x3.half().cuda(), [_frag(lib, _lib, w) for w in dw], [b.cuda().contiguous() for b in bs], outs[-1])
    return made


@pytest.mark.parametrize("m,cap", [(128, 256), (640, 2), (640, 256)])
@pytest.mark.parametrize("seed", [42, 43])
def test_dec_chain_exact_on_integers(integer_chains, seed, m, cap):
    _lib, lib = _lib_()
    x, x3, frags, biases, want = integer_chains[seed]
    rc, out = _chain(lib, _lib, x[:m].contiguous(), x3[:m].contiguous(), frags, biases, cap)
    _lib.check(rc)
    assert torch.equal(out.double().cpu(), want[:m])


@pytest.mark.parametrize("m", [384, 1280])
def test_dec_chain_bitwise_against_per_layer_launches(m):
    """Unit-variance inputs, He-scaled weights, biases of a tenth: the chain against the same layers through pcd_gemm_f16 with ReLU (lin 16 with
    a2 / k2 = x3), and the same launch twice into fresh outputs."""
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(700 + m)
    ws = [(torch.randn(s_, generator=g) * (2.0 / s_[1]) ** 0.5).half().cuda() for s_ in SHAPES]
    bs = [(0.1 * torch.randn(s_[0], generator=g)).cuda() for s_ in SHAPES]
    x = torch.randn(m, 1024, generator=g).half().cuda()
    x3 = torch.randn(m, 512, generator=g).half().cuda()
    a = x
    for i, (w, b) in enumerate(zip(ws, bs)):
        d = _lib.GemmDesc()
        d.a1, d.lda1, d.k1 = a.data_ptr(), a.shape[1], a.shape[1]
        if i == 1:
            d.a2, d.lda2, d.k2 = x3.data_ptr(), 512, 512
        d.w, d.ldw, d.bias, d.relu, d.m, d.c = w.data_ptr(), w.shape[1], b.data_ptr(), 1, m, w.shape[0]
        nxt = torch.empty(m, w.shape[0], dtype=torch.float16, device="cuda")
        _lib.check(lib.pcd_gemm_f16(C.byref(d), nxt.data_ptr(), w.shape[0], _lib.stream_ptr()))
        a = nxt
    frags = [_frag(lib, _lib, w) for w in ws]
    rc, out = _chain(lib, _lib, x, x3, frags, bs, 256)
    _lib.check(rc)
    rc, again = _chain(lib, _lib, x, x3, frags, bs, 256)
    _lib.check(rc)
    assert torch.isfinite(out).all() and float((out > 0).float().mean()) > 0.2
    assert torch.equal(out, a)
    assert torch.equal(again, out)


def test_dec_chain_refusals(integer_chains):
    """m % 128 != 0, a null fragment copy, a hi / lo layer, in == out (either input): an error code, and nothing written."""
    _lib, lib = _lib_()
    x, x3, frags, biases, _ = integer_chains[42]
    x_before, x3_before = x.clone(), x3.clone()
    out = torch.full((640, 256), -1.0, dtype=torch.float16, device="cuda")
    assert _chain(lib, _lib, x, x3, frags, biases, 256, m=100, out=out)[0] != 0
    assert _chain(lib, _lib, x, x3, [frags[0], None] + frags[2:], biases, 256, out=out)[0] != 0
    assert _chain(lib, _lib, x, x3, frags, biases, 256, hilo=2, out=out)[0] != 0
    assert _chain(lib, _lib, x, x3, frags, biases, 256, out=x.data_ptr())[0] != 0
    assert _chain(lib, _lib, x, x3, frags, biases, 256, out=x3.data_ptr())[0] != 0
    torch.cuda.synchronize()
    assert bool((out == -1).all())
    assert torch.equal(x, x_before) and torch.equal(x3, x3_before)


@pytest.fixture(scope="module")
def model():
    from helpers import point_sd
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=512)
    m.load_state_dict(point_sd(), strict=True)
    return m.to("cuda").eval()


def _captured(model, x, t, B, N):
    model.model.capture_decoder(B, N)
    try:
        eps = model.model(x, t).clone()
        return eps, model.model.tap("d4", B, N).clone(), model.model.tap("d3", B, N).clone()
    finally:
        model.model.capture_decoder(B, N, on=False)


@pytest.mark.parametrize("B,N", [(2, 512), (5, 512), (3, 100)])
def test_dec_chain_in_the_forward(model, B, N):
    """pcd_unet_forward with D43 (default, 3) and with bit 3 set (11: lin 15, 16 per layer + D3T): eps bit for bit, without a capture.  With the decoder
    captured (which runs lin 15, 16 per layer: dec4's output exists only inside D43) the d4 and d3 taps and eps equal those of the per-layer sequence
    (7).  B = 3, N = 100 is a ragged m: every setting runs the per-layer sequence."""
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(B * 1000 + N + 7)
    x = torch.randn(B, N, 3, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    try:
        _lib.check(lib.pcd_unet_config(3))
        eps_on = model.model(x, t).clone()
        cap_on = _captured(model, x, t, B, N)
        _lib.check(lib.pcd_unet_config(11))
        eps_off = model.model(x, t).clone()
        _lib.check(lib.pcd_unet_config(7))
        cap_layers = _captured(model, x, t, B, N)
    finally:
        _lib.check(lib.pcd_unet_config(3))
    assert torch.isfinite(eps_on).all()
    assert torch.equal(eps_on, eps_off)
    for a, b, name in zip(cap_on, cap_layers, ("eps", "d4", "d3")):
        assert torch.equal(a, b), name
    assert torch.equal(cap_on[0], eps_on)
