"""Latent path parity: SimpleLatentUNetPointNet, VAE3DLarge encode/decode (implicit-GEMM 3-D
convolutions), LatentDiffusion samplers -- HIP through the C ABI vs reference goldens / oracle.
Tolerances: fp16 operands + fp32 accumulate.  latent eps rel-L2 <= 3e-3; VAE mu/logvar <= 3e-3
(11 conv layers deep), decoded occupancy probabilities max-abs <= 5e-3 on in-distribution latents."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import latent_sd, rel_l2, voxels_from_idx, synth_voxels

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def ldm():
    from shapegen_amd.diffusion import LatentDiffusion
    from shapegen_amd.vae import VAE3DLarge
    m = LatentDiffusion(VAE3DLarge())
    m.load_state_dict(latent_sd(), strict=True)
    return m.to("cuda").eval()


def _int(shape, seed, lo=-2, hi=3):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).float()


def _run_conv(x, w, bias, stride, pad, relu=False, resid=None, split=False):
    """x (B,Cin,D,D,D), w (Cout,Cin,k,k,k) integer valued -> NDHWC result through pcd_conv3d_f16."""
    from shapegen_amd import _lib
    from shapegen_amd.vae import _pack_conv, _taps_regular
    lib = _lib.load()
    b, cin, din = x.shape[0], x.shape[1], x.shape[2]
    k = w.shape[2]
    dout = (din + 2 * pad - k) // stride + 1
    wk, _, kpad = _pack_conv(w.double().numpy(), None)
    dx = x.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    dw = torch.from_numpy(wk).half().cuda()
    taps = torch.from_numpy(_taps_regular(k, pad)).cuda()
    zero = torch.zeros(64, dtype=torch.float16, device="cuda")
    out = torch.empty(b * dout ** 3, w.shape[0], dtype=torch.float16, device="cuda")
    d = _lib.Conv3dDesc()
    d.inp, d.batch, d.in_d, d.in_h, d.in_w, d.cin = dx.data_ptr(), b, din, din, din, cin
    d.rows_d = d.rows_h = d.rows_w = dout
    d.stride, d.taps, d.ntaps, d.kpad = stride, taps.data_ptr(), taps.numel(), kpad
    db = bias.cuda()
    d.w, d.bias, d.relu = dw.data_ptr(), db.data_ptr(), 1 if relu else 0
    dr = None
    if resid is not None:
        dr = resid.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
        d.resid = dr.data_ptr()
    d.out, d.cout = out.data_ptr(), w.shape[0]
    d.out_d = d.out_h = d.out_w = dout
    d.out_scale = 1
    d.zero_page = zero.data_ptr()
    if split:
        need = int(lib.pcd_conv3d_workspace_bytes(d, 1))
        assert need > 0, "this shape is expected to take the split-K path"
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        _lib.check(lib.pcd_conv3d_f16_multi(d, 1, ws.data_ptr(), need, _lib.stream_ptr()))
    else:
        _lib.check(lib.pcd_conv3d_f16(d, _lib.stream_ptr()))
    return out.float().cpu().reshape(b, dout, dout, dout, -1).permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize("cin,cout,k,stride,pad,din", [(8, 16, 3, 1, 1, 6), (32, 72, 3, 1, 1, 5), (64, 136, 4, 2, 1, 8),
                                                       (16, 8, 1, 1, 0, 4), (128, 64, 4, 1, 0, 4)])
def test_conv3d_exact_integers(cin, cout, k, stride, pad, din):
    x, w, bias = _int((2, cin, din, din, din), 1), _int((cout, cin, k, k, k), 2, -1, 2), _int((cout,), 3)
    want = F.conv3d(x.double(), w.double(), bias.double(), stride=stride, padding=pad)
    resid = _int(tuple(want.shape), 4)
    for split in ((False, True) if cin * k ** 3 >= 8 * 64 else (False,)):      # split-K needs >= 8 K tiles
        got = _run_conv(x, w, bias, stride, pad, split=split).double()
        assert torch.equal(got, want.half().double())
        got = _run_conv(x, w, bias, stride, pad, relu=True, resid=resid, split=split).double()
        assert torch.equal(got, (want.half().double() + resid.double()).clamp_min(0).half().double())


@pytest.mark.parametrize("cin,cout,dims,b", [(64, 64, (8, 8, 8), 4), (64, 32, (4, 8, 16), 3), (32, 64, (8, 4, 8), 3),
                                             (32, 32, (4, 4, 8), 8), (64, 24, (4, 4, 8), 3), (32, 72, (4, 8, 8), 3),
                                             (32, 32, (8, 16, 8), 2), (64, 40, (4, 8, 16), 5)])
def test_conv3d_k3s1_halo_exact(cin, cout, dims, b):
    """The LDS-halo kernel (32^3 layers of VAE3DLarge) against F.conv3d on exactly representable integers:
    every border, partial / multiple C_out tiles, non-cubic volumes, residual + ReLU epilogue; block counts that
    are (b = 4, 8) and are not (b = 3) multiples of 8, i.e. with and without the XCD tile remap."""
    from shapegen_amd import _lib
    from shapegen_amd.vae import _pack_conv, _taps_regular
    lib = _lib.load()
    x, w, bias = _int((b, cin) + dims, 11), _int((cout, cin, 3, 3, 3), 12, -1, 2), _int((cout,), 13)
    want = F.conv3d(x.double(), w.double(), bias.double(), padding=1)
    resid = _int(tuple(want.shape), 14)
    wk, _, kpad = _pack_conv(w.double().numpy(), bias.double().numpy())
    dx = x.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    dw, db = torch.from_numpy(wk).half().cuda(), bias.cuda()
    dr = resid.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    taps = torch.from_numpy(_taps_regular(3, 1)).cuda()
    zero = torch.zeros(64, dtype=torch.float16, device="cuda")
    for use_resid in (False, True):
        out = torch.empty(b * dims[0] * dims[1] * dims[2], cout, dtype=torch.float16, device="cuda")
        d = _lib.Conv3dDesc()
        d.inp, d.batch, d.in_d, d.in_h, d.in_w, d.cin = dx.data_ptr(), b, dims[0], dims[1], dims[2], cin
        d.rows_d, d.rows_h, d.rows_w = dims
        d.out_d, d.out_h, d.out_w = dims
        d.stride, d.taps, d.ntaps, d.kpad = 1, taps.data_ptr(), 27, kpad
        d.w, d.bias, d.relu = dw.data_ptr(), db.data_ptr(), 1
        d.resid = dr.data_ptr() if use_resid else 0
        d.out, d.cout, d.out_scale, d.zero_page = out.data_ptr(), cout, 1, zero.data_ptr()
        assert lib.pcd_conv3d_k3s1_supported(d) == 1
        _lib.check(lib.pcd_conv3d_k3s1_f16(d, _lib.stream_ptr()))
        got = out.float().cpu().reshape((b,) + dims + (cout,)).permute(0, 4, 1, 2, 3).double()
        ref = want.half().double()
        ref = (ref + resid.double()).clamp_min(0).half().double() if use_resid else ref.clamp_min(0)
        assert torch.equal(got, ref)
        if dims[1] % 8 == 0:
            # the 256-row workgroups (4 x 8 x 8 voxels, eight waves; what large grids run) on the same descriptor
            out3 = torch.full_like(out, 3.0)
            d.out = out3.data_ptr()
            _lib.check(lib.pcd_conv3d_config(2))
            try:
                _lib.check(lib.pcd_conv3d_k3s1_f16(d, _lib.stream_ptr()))
            finally:
                _lib.check(lib.pcd_conv3d_config(1))
            assert torch.equal(out, out3)
            d.out = out.data_ptr()
        # and the generic implicit-GEMM kernel gives the same bits on the same descriptor
        out2 = torch.empty_like(out)
        d.out = out2.data_ptr()
        _lib.check(lib.pcd_conv3d_f16(d, _lib.stream_ptr()))
        assert torch.equal(out, out2)
    d.in_w = d.rows_w = d.out_w = dims[2] + 4                  # not a multiple of 8: refused, never mis-tiled
    assert lib.pcd_conv3d_k3s1_supported(d) == 0 and lib.pcd_conv3d_k3s1_f16(d, _lib.stream_ptr()) != 0


@pytest.mark.parametrize("cin,cout,cin2,dims,b,split", [(64, 128, 64, (4, 8, 8), 2, False), (128, 256, 128, (4, 4, 4), 1, True),
                                                         (64, 72, 64, (5, 3, 7), 3, False), (64, 64, 32, (4, 8, 16), 4, False),
                                                         (64, 128, 32, (8, 4, 8), 3, False)])
def test_conv3d_second_source_exact(cin, cout, cin2, dims, b, split):
    """ResidualBlock3D's projection shortcut inside conv2's launch (pcd_conv3d_desc_t.in2; reference networks.py:485-490, 500-503):
    relu(conv3(h) + conv1(x) + bias) with x as the second source, on exactly representable integers -- the implicit GEMM (cin2 in whole
    K tiles, split-K too) and the k3s1 halo kernel (cin 64, cin2 32: the extra k step through the weight ring; one and two C_out tiles)."""
    from shapegen_amd import _lib
    from shapegen_amd.vae import _pack_conv, _taps_regular
    lib = _lib.load()
    h, x = _int((b, cin) + dims, 31), _int((b, cin2) + dims, 32)
    w, wd, bias = _int((cout, cin, 3, 3, 3), 33, -1, 2), _int((cout, cin2, 1, 1, 1), 34, -1, 2), _int((cout,), 35)
    want = (F.conv3d(h.double(), w.double(), bias.double(), padding=1) + F.conv3d(x.double(), wd.double())).clamp_min(0).half().double()
    wk = np.concatenate([_pack_conv(w.double().numpy(), None)[0][:, :27 * cin], wd.double().numpy().reshape(cout, cin2)], axis=1)
    kpad = (wk.shape[1] + 63) // 64 * 64
    wp = np.zeros((cout, kpad)); wp[:, :wk.shape[1]] = wk
    dh = h.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    dx = x.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    dw, db = torch.from_numpy(wp).half().cuda(), bias.cuda()
    taps = torch.from_numpy(_taps_regular(3, 1)).cuda()
    zero = torch.zeros(64, dtype=torch.float16, device="cuda")
    out = torch.full((b * dims[0] * dims[1] * dims[2], cout), 9.0, dtype=torch.float16, device="cuda")
    d = _lib.Conv3dDesc()
    d.inp, d.batch, d.in_d, d.in_h, d.in_w, d.cin = dh.data_ptr(), b, dims[0], dims[1], dims[2], cin
    d.rows_d, d.rows_h, d.rows_w = dims
    d.out_d, d.out_h, d.out_w = dims
    d.stride, d.taps, d.ntaps, d.kpad = 1, taps.data_ptr(), 27, kpad
    d.w, d.bias, d.relu = dw.data_ptr(), db.data_ptr(), 1
    d.out, d.cout, d.out_scale, d.zero_page = out.data_ptr(), cout, 1, zero.data_ptr()
    d.in2, d.cin2 = dx.data_ptr(), cin2
    halo = cin2 == 32
    assert lib.pcd_conv3d_k3s1_supported(d) == (1 if halo else 0)
    if halo:
        _lib.check(lib.pcd_conv3d_k3s1_f16(d, _lib.stream_ptr()))
        assert lib.pcd_conv3d_f16(d, _lib.stream_ptr()) != 0            # the implicit GEMM takes whole K tiles only
    elif split:
        need = int(lib.pcd_conv3d_workspace_bytes(d, 1))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        _lib.check(lib.pcd_conv3d_f16_multi(d, 1, ws.data_ptr(), need, _lib.stream_ptr()))
    else:
        _lib.check(lib.pcd_conv3d_f16(d, _lib.stream_ptr()))
    got = out.float().cpu().reshape((b,) + dims + (cout,)).permute(0, 4, 1, 2, 3).double()
    assert torch.equal(got, want)
    d.resid = dh.data_ptr()                                               # a residual on top of a second source is refused
    assert lib.pcd_conv3d_f16(d, _lib.stream_ptr()) != 0 and lib.pcd_conv3d_k3s1_supported(d) == 0


def test_vae_fused_shortcut_matches_the_separate_launches(ldm):
    """The encoder with the projection shortcuts inside conv2 (default) against the same weights run as pointwise launch + residual read:
    same function, one fp16 rounding fewer per block -- mu / logvar agree to 2e-3, and both forms stay inside the golden bound (above)."""
    vox = synth_voxels(8, 5).cuda()
    assert ldm.vae.fuse_shortcut
    mu_f, lv_f = ldm.vae.encode(vox)
    try:
        mu_s, lv_s = ldm.vae.set_fuse_shortcut(False).encode(vox)
    finally:
        ldm.vae.set_fuse_shortcut(True)
    r = rel_l2(mu_f.cpu(), mu_s.cpu()), rel_l2(lv_f.cpu(), lv_s.cpu())
    print(f"fused v. separate shortcut launches: mu {r[0]:.2e} logvar {r[1]:.2e}")
    assert 0 < r[0] < 2e-3 and 0 < r[1] < 2e-3
    mu2, _ = ldm.vae.encode(vox)
    assert torch.equal(mu2, mu_f)


@pytest.mark.parametrize("cin,cout,dims,b", [(64, 64, (4, 8, 8), 1), (64, 64, (8, 16, 8), 3), (64, 128, (4, 8, 16), 2), (64, 192, (4, 8, 8), 4),
                                             (32, 32, (4, 8, 8), 3), (32, 32, (8, 8, 16), 2), (32, 64, (4, 16, 8), 3), (64, 32, (4, 8, 8), 5),
                                             (128, 128, (4, 8, 8), 2), (128, 256, (8, 8, 16), 1)])
def test_conv3d_k3s1_weights_in_registers_exact(cin, cout, dims, b):
    """The weights-in-registers form of the k3 / C_in = 64 layers (256-row workgroups, fragment-order weights loaded straight into the MFMA operand
    registers, no barrier in the tap loop, transposed product with direct stores) against F.conv3d on exactly representable integers, with and
    without the residual + ReLU epilogue, one to three C_out tiles -- and bit-identical to pcd_conv3d_k3s1_f16 on the same descriptor."""
    from shapegen_amd import _lib
    from shapegen_amd.vae import _pack_conv, _taps_regular
    lib = _lib.load()
    x, w, bias = _int((b, cin) + dims, 61), _int((cout, cin, 3, 3, 3), 62, -1, 2), _int((cout,), 63)
    want = F.conv3d(x.double(), w.double(), bias.double(), padding=1)
    resid = _int(tuple(want.shape), 64)
    wk, _, kpad = _pack_conv(w.double().numpy(), None)
    dx = x.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    dw, db = torch.from_numpy(wk).half().cuda(), bias.cuda()
    dr = resid.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    taps = torch.from_numpy(_taps_regular(3, 1)).cuda()
    zero = torch.zeros(64, dtype=torch.float16, device="cuda")
    wfrag = torch.empty(int(lib.pcd_conv3d_wfrag_bytes(cin, cout)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.pcd_conv3d_pack_wfrag(dw.data_ptr(), kpad, cin, cout, 0, wfrag.data_ptr(), _lib.stream_ptr()))
    for use_resid in (False, True):
        out = torch.full((b * dims[0] * dims[1] * dims[2], cout), 3.0, dtype=torch.float16, device="cuda")
        d = _lib.Conv3dDesc()
        d.inp, d.batch, d.in_d, d.in_h, d.in_w, d.cin = dx.data_ptr(), b, dims[0], dims[1], dims[2], cin
        d.rows_d, d.rows_h, d.rows_w = dims
        d.out_d, d.out_h, d.out_w = dims
        d.stride, d.taps, d.ntaps, d.kpad = 1, taps.data_ptr(), 27, kpad
        d.w, d.bias, d.relu = dw.data_ptr(), db.data_ptr(), 1
        d.resid = dr.data_ptr() if use_resid else 0
        d.out, d.cout, d.out_scale, d.zero_page = out.data_ptr(), cout, 1, zero.data_ptr()
        assert lib.pcd_conv3d_k3s1_wreg_supported(d) == 1
        _lib.check(lib.pcd_conv3d_k3s1_wreg_f16(d, wfrag.data_ptr(), _lib.stream_ptr()))
        got = out.float().cpu().reshape((b,) + dims + (cout,)).permute(0, 4, 1, 2, 3).double()
        ref = want.half().double()
        ref = (ref + resid.double()).clamp_min(0).half().double() if use_resid else ref.clamp_min(0)
        assert torch.equal(got, ref), use_resid
        out2 = torch.empty_like(out)
        d.out = out2.data_ptr()
        _lib.check((lib.pcd_conv3d_k3s1_f16 if cin <= 64 else lib.pcd_conv3d_f16)(d, _lib.stream_ptr()))      # (C_in 128: the implicit GEMM, same k order)
        assert torch.equal(out, out2)
    if cin < 64:
        return
    # with a projection shortcut as second source (32 channels, 64 at C_in 128; its weight columns sit behind the 27 taps = the last stage of the fragment copy)
    c2 = 32 if cin == 64 else 64
    x2, wd = _int((b, c2) + dims, 65), _int((cout, c2, 1, 1, 1), 66, -1, 2)
    want2 = (want + F.conv3d(x2.double(), wd.double())).clamp_min(0).half().double()
    wk2 = np.concatenate([wk[:, :27 * cin], wd.double().numpy().reshape(cout, c2)], axis=1)
    kpad2 = (wk2.shape[1] + 63) // 64 * 64
    wp2 = np.zeros((cout, kpad2)); wp2[:, :wk2.shape[1]] = wk2
    dw2 = torch.from_numpy(wp2).half().cuda()
    dx2 = x2.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    _lib.check(lib.pcd_conv3d_pack_wfrag(dw2.data_ptr(), kpad2, cin, cout, c2, wfrag.data_ptr(), _lib.stream_ptr()))
    d.resid, d.w, d.kpad, d.in2, d.cin2, d.out = 0, dw2.data_ptr(), kpad2, dx2.data_ptr(), c2, out.data_ptr()
    assert lib.pcd_conv3d_k3s1_wreg_supported(d) == 1
    _lib.check(lib.pcd_conv3d_k3s1_wreg_f16(d, wfrag.data_ptr(), _lib.stream_ptr()))
    got = out.float().cpu().reshape((b,) + dims + (cout,)).permute(0, 4, 1, 2, 3).double()
    assert torch.equal(got, want2)
    d.in2, d.cin2 = 0, 0
    d.in_h = d.rows_h = d.out_h = dims[1] + 4                  # H not a multiple of 8: refused
    assert lib.pcd_conv3d_k3s1_wreg_supported(d) == 0 and lib.pcd_conv3d_k3s1_wreg_f16(d, wfrag.data_ptr(), _lib.stream_ptr()) != 0


@pytest.mark.parametrize("k,c,ldw,m,relu", [(32, 64, 64, 1000, 0), (32, 64, 32, 77, 1), (64, 128, 64, 4096 + 31, 0),
                                            (128, 256, 128, 515, 0), (128, 256, 192, 128, 1)])
def test_conv1x1_pointwise_exact_integers(k, c, ldw, m, relu):
    """ResidualBlock3D's 1x1x1 shortcut (reference networks.py:485-490) as a pointwise layer with LDS-resident weights:
    small integers make every fp32 partial sum exact, so the result equals the integer product bit for bit; ragged m,
    padded weight rows (ldw > k), with and without ReLU."""
    from shapegen_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(k + m)
    x = torch.randint(-3, 4, (m, k), generator=g).half().cuda()
    w = torch.randint(-3, 4, (c, ldw), generator=g).half().cuda()
    b = torch.randint(-8, 9, (c,), generator=g).float().cuda()
    out = torch.full((m, c), 7.0, dtype=torch.float16, device="cuda")
    assert lib.pcd_conv1x1_supported(k, c) == 1 and lib.pcd_conv1x1_supported(k, c + 64) == 0
    _lib.check(lib.pcd_conv1x1_f16(x.data_ptr(), m, k, w.data_ptr(), ldw, b.data_ptr(), relu, c, out.data_ptr(),
                                   _lib.stream_ptr()))
    want = x.float() @ w[:, :k].float().t() + b
    if relu:
        want = want.clamp_min(0)
    assert torch.equal(out.float(), want)
    assert lib.pcd_conv1x1_f16(x.data_ptr(), m, 48, w.data_ptr(), ldw, b.data_ptr(), relu, c, out.data_ptr(), 0) != 0


@pytest.mark.parametrize("dims,stride", [((8, 8, 8), 1), ((16, 8, 24), 1), ((4, 8, 16), 1), ((6, 5, 7), 1), ((8, 8, 8), 2), ((4, 4, 8), 1)])
def test_conv3d_first_and_last_layers(dims, stride):
    """encoder.0 (Cin = 1, ReLU, fp16 NDHWC out) and decoder.12/13 (Cout = 1, sigmoid) against F.conv3d in fp64:
    the LDS-halo last-layer path (dims multiples of 4, 4, 8), its direct fallback (6, 5, 7), and the cout = 32
    first-layer path at both strides.  (4, 4, 8) is one 4 x 4 x 8 block that no 8-row form divides: with a packed copy
    present the packed entry still has to land on the 4 x 4 x 8 halo form, the first layer on its 4 x 4 x 8 tiles."""
    from shapegen_amd import _lib
    lib = _lib.load()
    b = 2
    g = torch.Generator().manual_seed(5)
    x = torch.rand((b, 1) + dims, generator=g)
    w0, b0 = torch.randn(32, 1, 3, 3, 3, generator=g) * 0.3, torch.randn(32, generator=g) * 0.1
    want = F.conv3d(x.double(), w0.double(), b0.double(), stride=stride, padding=1).clamp_min(0)
    od = tuple((d - 1) // stride + 1 for d in dims)
    out = torch.empty(b * od[0] * od[1] * od[2], 32, dtype=torch.float16, device="cuda")
    dx, dw, db = x.cuda().contiguous(), w0.reshape(32, 27).contiguous().cuda(), b0.cuda()
    _lib.check(lib.pcd_conv3d_first(dx.data_ptr(), b, dims[0], dims[1], dims[2], stride, dw.data_ptr(), db.data_ptr(), 32,
                                    out.data_ptr(), _lib.stream_ptr()))
    got = out.float().cpu().reshape((b,) + od + (32,)).permute(0, 4, 1, 2, 3).double()
    assert (got - want).abs().max() <= 2e-3 * max(1.0, float(want.abs().max()))       # one fp16 rounding
    if stride == 1 and all(d % 8 == 0 for d in dims):                                  # 8 x 8 x 8 tiles (default) against 4 x 4 x 8 tiles: the same bits
        out4 = torch.empty_like(out)
        _lib.check(lib.pcd_conv3d_config(512 + 1))
        try:
            _lib.check(lib.pcd_conv3d_first(dx.data_ptr(), b, dims[0], dims[1], dims[2], stride, dw.data_ptr(), db.data_ptr(), 32,
                                            out4.data_ptr(), _lib.stream_ptr()))
        finally:
            _lib.check(lib.pcd_conv3d_config(1))
        assert torch.equal(out4, out)
    if stride == 1:
        h = out                                                                        # fp16 NDHWC, 32 channels
        wl, bl = torch.randn(1, 32, 3, 3, 3, generator=g) * 0.1, 0.05
        hin = h.float().cpu().reshape((b,) + dims + (32,)).permute(0, 4, 1, 2, 3).double()
        want2 = torch.sigmoid(F.conv3d(hin, wl.double(), torch.tensor([bl]).double(), padding=1))
        dwl = wl[0].permute(1, 2, 3, 0).reshape(27, 32).contiguous().cuda()
        o2 = torch.empty((b, 1) + dims, dtype=torch.float32, device="cuda")
        _lib.check(lib.pcd_conv3d_last_sigmoid(h.data_ptr(), b, dims[0], dims[1], dims[2], 32, dwl.data_ptr(), bl,
                                               o2.data_ptr(), _lib.stream_ptr()))
        assert (o2.cpu().double() - want2).abs().max() <= 2e-6
        # the matrix-pipe form (what pcd_vae_decode launches where the grid divides by 8; elsewhere the call falls back to the kernels above)
        wf = torch.empty(lib.pcd_conv3d_last_packed_bytes(), dtype=torch.uint8, device="cuda")
        _lib.check(lib.pcd_conv3d_last_pack(dwl.data_ptr(), wf.data_ptr(), _lib.stream_ptr()))
        o4 = torch.empty_like(o2)
        _lib.check(lib.pcd_conv3d_last_sigmoid_packed(h.data_ptr(), b, dims[0], dims[1], dims[2], 32, dwl.data_ptr(), wf.data_ptr(), bl,
                                                      o4.data_ptr(), _lib.stream_ptr()))
        assert (o4.cpu().double() - want2).abs().max() <= 2e-6
        # (default where the grid divides by 8: per-tap partial products, conv3d_last_taps_kernel; + 24: one MFMA per tap and 16 voxels from the packed copy)
        _lib.check(lib.pcd_conv3d_config(16384 + 1))                                  # + 16384: a wave per output slice instead of per four
        try:
            o7 = torch.empty_like(o2)
            _lib.check(lib.pcd_conv3d_last_sigmoid_packed(h.data_ptr(), b, dims[0], dims[1], dims[2], 32, dwl.data_ptr(), wf.data_ptr(), bl,
                                                          o7.data_ptr(), _lib.stream_ptr()))
        finally:
            _lib.check(lib.pcd_conv3d_config(1))
        assert (o7.cpu().double() - want2).abs().max() <= 2e-6
        _lib.check(lib.pcd_conv3d_config(24 + 1))
        try:
            o5 = torch.empty_like(o2)
            _lib.check(lib.pcd_conv3d_last_sigmoid_packed(h.data_ptr(), b, dims[0], dims[1], dims[2], 32, dwl.data_ptr(), wf.data_ptr(), bl,
                                                          o5.data_ptr(), _lib.stream_ptr()))
        finally:
            _lib.check(lib.pcd_conv3d_config(1))
        assert (o5.cpu().double() - want2).abs().max() <= 2e-6
        o6 = torch.empty_like(o2)
        _lib.check(lib.pcd_conv3d_last_sigmoid_packed(h.data_ptr(), b, dims[0], dims[1], dims[2], 32, dwl.data_ptr(), wf.data_ptr(), bl,
                                                      o6.data_ptr(), _lib.stream_ptr()))
        assert torch.equal(o6, o4)                                                   # bitwise repeatable
        # the other forms where the grid divides by 8: 8 x 8 x 8 blocks on the matrix pipe (hi / lo / lo2 rows of the fp32 weights); + 16: the same blocks on the VALU;
        # + 8: 4 x 4 x 8 blocks
        for cfg in (16 + 1, 8 + 1):
            _lib.check(lib.pcd_conv3d_config(cfg))
            try:
                o3 = torch.empty_like(o2)
                _lib.check(lib.pcd_conv3d_last_sigmoid(h.data_ptr(), b, dims[0], dims[1], dims[2], 32, dwl.data_ptr(), bl,
                                                       o3.data_ptr(), _lib.stream_ptr()))
            finally:
                _lib.check(lib.pcd_conv3d_config(1))           # the library's default
            assert (o3.cpu().double() - want2).abs().max() <= 2e-6, cfg
        if dims == (8, 8, 8):                                                        # the packed entry without a packed copy: the forms that read the fp32 weights
            o8 = torch.empty_like(o2)
            _lib.check(lib.pcd_conv3d_last_sigmoid_packed(h.data_ptr(), b, dims[0], dims[1], dims[2], 32, dwl.data_ptr(), None, bl,
                                                          o8.data_ptr(), _lib.stream_ptr()))
            assert (o8.cpu().double() - want2).abs().max() <= 2e-6


@pytest.mark.parametrize("stride", [1, 2])
def test_conv3d_first_layer_generic_width(stride):
    """pcd_conv3d_first at a width other than 32 (cout = 16): the generic kernel, weights and bias in dynamic LDS, on a grid that no
    tile divides, against F.conv3d in fp64."""
    from shapegen_amd import _lib
    lib = _lib.load()
    b, dims, cout = 2, (6, 5, 7), 16
    g = torch.Generator().manual_seed(6)
    x = torch.rand((b, 1) + dims, generator=g)
    w0, b0 = torch.randn(cout, 1, 3, 3, 3, generator=g) * 0.3, torch.randn(cout, generator=g) * 0.1
    want = F.conv3d(x.double(), w0.double(), b0.double(), stride=stride, padding=1).clamp_min(0)
    od = tuple((d - 1) // stride + 1 for d in dims)
    out = torch.empty(b * od[0] * od[1] * od[2], cout, dtype=torch.float16, device="cuda")
    dx, dw, db = x.cuda().contiguous(), w0.reshape(cout, 27).contiguous().cuda(), b0.cuda()
    _lib.check(lib.pcd_conv3d_first(dx.data_ptr(), b, dims[0], dims[1], dims[2], stride, dw.data_ptr(), db.data_ptr(), cout,
                                    out.data_ptr(), _lib.stream_ptr()))
    got = out.float().cpu().reshape((b,) + od + (cout,)).permute(0, 4, 1, 2, 3).double()
    assert float(want.max()) > 0.5                                                   # the ReLU leaves something to compare
    assert (got - want).abs().max() <= 2e-3 * max(1.0, float(want.abs().max()))       # one fp16 rounding


def test_conv_transpose3d_classes_exact():
    """ConvTranspose3d(k4,s2,p1) as 8 parity classes of 2x2x2 taps."""
    from shapegen_amd import _lib
    from shapegen_amd.vae import _pack_convT_class
    lib = _lib.load()
    b, cin, cout, din = 2, 64, 24, 3
    x, w, bias = _int((b, cin, din, din, din), 5), _int((cin, cout, 4, 4, 4), 6, -1, 2), _int((cout,), 7)
    want = F.conv_transpose3d(x.double(), w.double(), bias.double(), stride=2, padding=1).clamp_min(0)
    dx = x.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    zero = torch.zeros(64, dtype=torch.float16, device="cuda")
    dout = 2 * din
    out = torch.empty(b * dout ** 3, cout, dtype=torch.float16, device="cuda")
    db = bias.cuda()
    keep, descs = [], []
    for pz in (0, 1):
        for py in (0, 1):
            for px in (0, 1):
                wc, taps = _pack_convT_class(w.double().numpy(), pz, py, px)
                dw, dt = torch.from_numpy(wc).half().cuda(), torch.from_numpy(taps).cuda()
                keep += [dw, dt]
                d = _lib.Conv3dDesc()
                d.inp, d.batch, d.in_d, d.in_h, d.in_w, d.cin = dx.data_ptr(), b, din, din, din, cin
                d.rows_d = d.rows_h = d.rows_w = din
                d.stride, d.taps, d.ntaps, d.kpad = 1, dt.data_ptr(), 8, 8 * cin
                d.w, d.bias, d.relu = dw.data_ptr(), db.data_ptr(), 1
                d.out, d.cout = out.data_ptr(), cout
                d.out_d = d.out_h = d.out_w = dout
                d.out_scale, d.out_off_z, d.out_off_y, d.out_off_x = 2, pz, py, px
                d.zero_page = zero.data_ptr()
                _lib.check(lib.pcd_conv3d_f16(d, _lib.stream_ptr()))
                descs.append(d)
    got = out.float().cpu().reshape(b, dout, dout, dout, cout).permute(0, 4, 1, 2, 3).double()
    assert torch.equal(got, want.half().double())
    # the same 8 classes as ONE launch (blockIdx.y = class), split-K with the finish kernel
    out.zero_()
    arr = (_lib.Conv3dDesc * 8)(*descs)
    need = int(lib.pcd_conv3d_workspace_bytes(arr, 8))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.pcd_conv3d_f16_multi(arr, 8, ws.data_ptr(), need, _lib.stream_ptr()))
    got = out.float().cpu().reshape(b, dout, dout, dout, cout).permute(0, 4, 1, 2, 3).double()
    assert torch.equal(got, want.half().double())
    # classes that do not share a shape are refused, not silently mis-launched
    arr[3].kpad += 64
    assert lib.pcd_conv3d_f16_multi(arr, 8, ws.data_ptr(), need, _lib.stream_ptr()) != 0


@pytest.mark.parametrize("dims,b", [((4, 4, 8), 1), ((8, 4, 16), 3), ((8, 8, 8), 8)])
def test_conv_transpose3d_halo_exact(dims, b):
    """decoder.6's kernel (C_in 128 -> C_out 64; input halo in LDS, all eight parity classes per workgroup, transposed product with
    16-byte direct stores) against F.conv_transpose3d on exactly representable integers: every border, non-cubic grids, block counts that
    are and are not multiples of 8 (XCD remap), and bit-identical to the eight implicit-GEMM class launches."""
    import ctypes as C
    from shapegen_amd import _lib
    from shapegen_amd.vae import _pack_convT_class
    lib = _lib.load()
    cin, cout = 128, 64
    x, w, bias = _int((b, cin) + dims, 41), _int((cin, cout, 4, 4, 4), 42, -1, 2), _int((cout,), 43)
    want = F.conv_transpose3d(x.double(), w.double(), bias.double(), stride=2, padding=1).clamp_min(0).half().double()
    dx = x.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    db = bias.cuda()
    odims = tuple(2 * v for v in dims)
    nvox = b * odims[0] * odims[1] * odims[2]
    out = torch.full((nvox, cout), 5.0, dtype=torch.float16, device="cuda")
    keep, ptrs, descs = [], (C.c_void_p * 8)(), []
    zero = torch.zeros(64, dtype=torch.float16, device="cuda")
    out2 = torch.empty_like(out)
    for pz in (0, 1):
        for py in (0, 1):
            for px in (0, 1):
                wc, taps = _pack_convT_class(w.double().numpy(), pz, py, px)
                dw, dt = torch.from_numpy(wc).half().cuda(), torch.from_numpy(taps).cuda()
                keep += [dw, dt]
                ptrs[4 * pz + 2 * py + px] = dw.data_ptr()
                d = _lib.Conv3dDesc()
                d.inp, d.batch, d.in_d, d.in_h, d.in_w, d.cin = dx.data_ptr(), b, dims[0], dims[1], dims[2], cin
                d.rows_d, d.rows_h, d.rows_w = dims
                d.stride, d.taps, d.ntaps, d.kpad = 1, dt.data_ptr(), 8, 8 * cin
                d.w, d.bias, d.relu = dw.data_ptr(), db.data_ptr(), 1
                d.out, d.cout = out2.data_ptr(), cout
                d.out_d, d.out_h, d.out_w = odims
                d.out_scale, d.out_off_z, d.out_off_y, d.out_off_x = 2, pz, py, px
                d.zero_page = zero.data_ptr()
                descs.append(d)
    assert lib.pcd_convt3d_k4s2_halo_supported(b, dims[0], dims[1], dims[2], cin, cout) == 1
    _lib.check(lib.pcd_convt3d_k4s2_halo_f16(dx.data_ptr(), b, dims[0], dims[1], dims[2], cin, ptrs, db.data_ptr(), cout, out.data_ptr(),
                                             _lib.stream_ptr()))
    got = out.float().cpu().reshape((b,) + odims + (cout,)).permute(0, 4, 1, 2, 3).double()
    assert torch.equal(got, want)
    arr = (_lib.Conv3dDesc * 8)(*descs)
    _lib.check(lib.pcd_conv3d_f16_multi(arr, 8, None, 0, _lib.stream_ptr()))
    assert torch.equal(out, out2)
    assert lib.pcd_convt3d_k4s2_halo_supported(b, dims[0], dims[1], dims[2] + 4, cin, cout) == 0
    assert lib.pcd_convt3d_k4s2_halo_supported(b, dims[0], dims[1], dims[2], 64, cout) == 0
    assert lib.pcd_convt3d_k4s2_halo_f16(dx.data_ptr(), b, dims[0], dims[1], dims[2], 64, ptrs, db.data_ptr(), cout, out.data_ptr(), 0) != 0


@pytest.mark.parametrize("dims,b", [((8, 8, 16), 1), ((16, 8, 32), 3), ((16, 16, 16), 8)])
def test_conv3d_k4s2_halo_exact(dims, b):
    """encoder.3's kernel (Conv3d k4 s2 p1, 64 -> 64: eight input-parity classes of a 4 x 4 x 8 output block from LDS-resident sub-grid halos,
    halo swapped per class, transposed product with 16-byte stores) against F.conv3d on exactly representable integers -- every border, non-cubic
    grids, block counts that are and are not multiples of 8 -- and bit-identical to the implicit-GEMM launch, with and without ReLU."""
    from shapegen_amd import _lib
    from shapegen_amd.vae import _pack_conv
    lib = _lib.load()
    cin = cout = 64
    x, w, bias = _int((b, cin) + dims, 51), _int((cout, cin, 4, 4, 4), 52, -1, 2), _int((cout,), 53)
    want = F.conv3d(x.double(), w.double(), bias.double(), stride=2, padding=1)
    wk, _, kpad = _pack_conv(w.double().numpy(), None)
    dx = x.permute(0, 2, 3, 4, 1).contiguous().half().cuda()
    dw, db = torch.from_numpy(wk).half().cuda(), bias.cuda()
    odims = tuple(v // 2 for v in dims)
    assert lib.pcd_conv3d_k4s2_halo_supported(b, dims[0], dims[1], dims[2], cin, cout, kpad) == 1
    for relu in (1, 0):
        out = torch.full((b * odims[0] * odims[1] * odims[2], cout), 5.0, dtype=torch.float16, device="cuda")
        _lib.check(lib.pcd_conv3d_k4s2_halo_f16(dx.data_ptr(), b, dims[0], dims[1], dims[2], cin, dw.data_ptr(), kpad, db.data_ptr(), relu, cout,
                                                out.data_ptr(), _lib.stream_ptr()))
        got = out.float().cpu().reshape((b,) + odims + (cout,)).permute(0, 4, 1, 2, 3).double()
        ref = (want.clamp_min(0) if relu else want).half().double()
        assert torch.equal(got, ref), relu
    if dims[0] == dims[1] == dims[2]:
        assert torch.equal(got, _run_conv(x, w, bias, 2, 1).double())
    assert lib.pcd_conv3d_k4s2_halo_supported(b, dims[0], dims[1], dims[2] + 8, cin, cout, kpad) == 0
    assert lib.pcd_conv3d_k4s2_halo_supported(b, dims[0], dims[1], dims[2], 128, cout, kpad) == 0
    assert lib.pcd_conv3d_k4s2_halo_f16(dx.data_ptr(), b, dims[0], dims[1], dims[2], cin, dw.data_ptr(), 64, db.data_ptr(), 1, cout, out.data_ptr(), 0) != 0


def test_vae_decode_halo_transposed_convolution_matches_the_class_launches(ldm):
    """The round-4 convolution kernels (default) against the implicit-GEMM / LDS-ring forms they replace (pcd_vae_config(0)) inside the whole decode
    and the whole encode: the same fp16 products summed in fp32, in another order where the old form splits K."""
    from shapegen_amd import _lib
    lib = _lib.load()
    z = torch.randn(8, 256, generator=torch.Generator().manual_seed(77)).cuda()
    a = ldm.vae.decode(z).clone()
    _lib.check(lib.pcd_vae_config(0))
    try:
        c = ldm.vae.decode(z).clone()
    finally:
        _lib.check(lib.pcd_vae_config(1))
    err = (a - c).abs()
    print(f"decode: halo transposed convolution v. class launches: max {float(err.max()):.2e} mean {float(err.mean()):.2e}")
    # (decoder.6's two forms are bitwise equal; the C_in = 128 layers' implicit GEMM splits K at this batch, another fp32 summation order than the
    # weights-in-registers kernel's: the bound is the golden decode test's)
    assert float(err.max()) < 5e-3 and float(err.mean()) < 5e-4 and torch.equal(ldm.vae.decode(z), a)
    # encoder.3 through its LDS kernel (default) against the implicit GEMM inside the whole encode
    vox = synth_voxels(8, 6).cuda()
    mu_a, lv_a = ldm.vae.encode(vox)
    _lib.check(lib.pcd_vae_config(0))
    try:
        mu_c, lv_c = ldm.vae.encode(vox)
    finally:
        _lib.check(lib.pcd_vae_config(1))
    r = rel_l2(mu_a.cpu(), mu_c.cpu()), rel_l2(lv_a.cpu(), lv_c.cpu())
    print(f"encode: k4 s2 LDS kernel v. implicit GEMM: mu {r[0]:.2e} logvar {r[1]:.2e}")
    assert r[0] < 2e-3 and r[1] < 2e-3


def test_latent_unet_forward(ldm, golden):
    g = golden("latent.npz")
    eps = ldm.model(torch.from_numpy(g["lat_z"]).cuda(), torch.from_numpy(g["lat_t"]).cuda()).cpu()
    assert rel_l2(eps, g["lat_eps"]) < 3e-3
    # a single row gives the same answer as the same row inside the batch (GroupNorm is per sample)
    one = ldm.model(torch.from_numpy(g["lat_z"][3:4]).cuda(), torch.from_numpy(g["lat_t"][3:4]).cuda()).cpu()
    assert rel_l2(one, eps[3:4]) < 1e-6


def test_vae_encode_decode(ldm, golden):
    from shapegen_amd.utils import voxel_tensor_to_point_clouds
    g = golden("latent.npz")
    vox = voxels_from_idx([g["vae_occ_idx"], g["vae_occ_idx1"]]).cuda()
    mu, logvar = ldm.vae.encode(vox)
    assert rel_l2(mu.cpu(), g["vae_mu"]) < 3e-3 and rel_l2(logvar.cpu(), g["vae_logvar"]) < 3e-3    # measured 1.1e-3 / 1.0e-3
    dec = ldm.vae.decode(torch.from_numpy(g["vae_mu"]).cuda())
    assert dec.shape == (2, 1, 32, 32, 32)
    err = (dec.cpu() - torch.from_numpy(g["vae_dec"])).abs()
    assert float(err.max()) < 5e-3 and float(err.mean()) < 5e-4                                      # measured 1.4e-3 / 1.9e-4
    # voxel->points on the HIP-decoded grid: the occupied set may differ from the reference only where
    # the probability is within the decode tolerance of the threshold
    want = torch.from_numpy(g["vae_dec"])
    for thr in (0.4, 0.5):
        got_occ, want_occ = dec.cpu() > thr, want > thr
        flips = got_occ != want_occ
        assert bool(((want - thr).abs()[flips] < 2e-2).all())
        assert float(flips.float().mean()) < 5e-3
        pcs = voxel_tensor_to_point_clouds(dec, thr)
        assert [len(p) for p in pcs] == [int(got_occ[i].sum()) for i in range(2)]
    z = ldm.vae.reparameterize(mu, logvar, eps=torch.ones_like(mu))
    np.testing.assert_allclose(z.cpu().numpy(), (mu.cpu() + torch.exp(0.5 * logvar.cpu())).numpy(), rtol=1e-6, atol=1e-7)
    rec, mu2, _ = ldm.vae(vox, eps=torch.zeros_like(mu))
    assert torch.equal(mu2, mu) and rec.shape == (2, 1, 32, 32, 32)


def test_vae_batch_invariance_across_launch_shapes(ldm):
    """B = 16 runs the large-grid forms of the convolution launches (256-row halo workgroups for 32 -> 32, unsplit implicit
    GEMMs, the weight-streaming GEMM for encoder.12 and the fc heads) where B = 1 runs the small-grid forms (128-row
    workgroups, split-K + finish).  Same function: a sample decodes / encodes to the same values inside a batch and alone
    (fp16 activations; split-K changes the order of fp32 partial sums only)."""
    g = torch.Generator().manual_seed(21)
    z = torch.randn(16, 256, generator=g).cuda()
    dec16 = ldm.vae.decode(z)
    assert torch.isfinite(dec16).all() and dec16.shape == (16, 1, 32, 32, 32)
    for i in (0, 7, 15):
        one = ldm.vae.decode(z[i:i + 1])
        err = (one - dec16[i:i + 1]).abs()
        assert float(err.max()) < 2e-2 and float(err.mean()) < 1e-3, i          # the bounds of the golden decode test, halved for the mean
    vox = (dec16 > 0.5).float()
    mu16, lv16 = ldm.vae.encode(vox)
    for i in (0, 9):
        mu1, lv1 = ldm.vae.encode(vox[i:i + 1])
        assert rel_l2(mu1.cpu(), mu16[i:i + 1].cpu()) < 3e-3 and rel_l2(lv1.cpu(), lv16[i:i + 1].cpu()) < 3e-3


def test_vae_is_bitwise_repeatable(ldm):
    """No kernel of the VAE uses atomics or a run-dependent summation order: the same call gives the same bits, at the batch where two workgroups
    share a CU (B = 16: the launch shape at which an LDS-DMA ring refill could overtake a queued fragment read before the round-4 fix -- one encode in
    seven differed by 1e-3..5e-3 then; tools/diag_vae_batch.py is the long form of this test, tests/test_isa_barrier_reads.py the static one)."""
    g = torch.Generator().manual_seed(22)
    z = torch.randn(16, 256, generator=g).cuda()
    dec0 = ldm.vae.decode(z).clone()
    vox = (dec0 > 0.5).float()
    mu0, lv0 = (t.clone() for t in ldm.vae.encode(vox))
    for _ in range(40):
        assert torch.equal(ldm.vae.decode(z), dec0)
        mu, lv = ldm.vae.encode(vox)
        assert torch.equal(mu, mu0) and torch.equal(lv, lv0)


@pytest.mark.parametrize("T", [5, 100])
def test_latent_ddim(ldm, golden, T):
    g = golden("latent.npz")
    pcs, z0 = ldm.sample(2, num_steps=T, z_T=torch.from_numpy(g[f"ldm_T{T}_zT"]).cuda(), return_latent=True)
    assert rel_l2(z0.cpu(), g[f"ldm_T{T}_z0"]) < 5e-3
    counts = np.array([len(p) for p in pcs])
    assert np.all(np.abs(counts - g[f"ldm_T{T}_counts"]) <= 0.02 * g[f"ldm_T{T}_counts"] + 8)
    assert all(p.shape[1] == 3 and float(p.abs().max()) <= 1.0 for p in pcs if len(p))


def test_cfg4_launch_shapes_vs_reference(ldm, golden):
    """BASELINE configs[3] at the launch shapes the bench line quotes (B = 32): encode 32 grids, 1000 latent DDIM steps from
    the recorded z_T, decode, voxel -> points -- against G17, captured from the reference at B = 32, T = 1000
    (diffusion.py:619-653, networks.py:2299-2339)."""
    from shapegen_amd.utils import voxel_tensor_to_point_clouds
    g = golden("cfg4.npz")
    rows = g["dec_rows"]
    vox = synth_voxels(32, 4).cuda()
    mu, logvar = ldm.vae.encode(vox)
    assert mu.shape == (32, 256)
    assert rel_l2(mu.cpu(), g["enc_mu"]) < 3e-3 and rel_l2(logvar.cpu(), g["enc_logvar"]) < 3e-3
    for i in rows:                                                   # per row too: no sample hides behind the batch norm
        assert rel_l2(mu[i].cpu(), g["enc_mu"][i]) < 5e-3, i
    for persistent in (True, False):                       # one persistent launch for the 1000 steps / per-layer launches
        ldm.use_persistent = persistent
        try:
            pcs, z0 = ldm.sample(32, num_steps=1000, z_T=torch.from_numpy(g["zT"]).cuda(), return_latent=True)
        finally:
            ldm.use_persistent = type(ldm).use_persistent
        err = rel_l2(z0.cpu(), g["z0"])
        worst = max(rel_l2(z0[i].cpu(), g["z0"][i]) for i in range(32))
        print(f"latent DDIM T=1000 at B=32 vs reference ({'persistent launch' if persistent else 'per-layer launches'}): rel-L2 {err:.3e}, worst row {worst:.3e}")
        assert err < 5e-3, (persistent, err)
        assert worst < 1e-2
    counts = np.array([len(p) for p in pcs])
    assert np.all(np.abs(counts - g["counts"]) <= 0.02 * g["counts"] + 8)
    # decode at B = 32 of the REFERENCE's latents (so the comparison is of the decoder alone), four rows kept in the fixture.  With
    # random-init weights the 1000-step latents are blown up (|z0| up to 238): the decoder's logits are then hundreds
    # wide and an fp16 activation error of 1e-3 relative moves a voxel in the sigmoid's transition by up to ~0.15 in probability.
    # Stated bound for THOSE inputs: mean 2e-3, 99th percentile 2e-2, occupancy decisions at 0.4 differ for < 0.2 % of the voxels
    # (measured: mean 4.2e-4, p99 1.1e-2, flips 0.05 %, max 0.157 on voxels whose reference probability is 0.03..0.96).
    dec = ldm.vae.decode(torch.from_numpy(g["z0"]).cuda())
    assert dec.shape == (32, 1, 32, 32, 32)
    sel = torch.from_numpy(rows).cuda()
    want_dec = torch.from_numpy(g["dec"]).float()
    derr = (dec[sel].cpu() - want_dec).abs()
    assert float(derr.mean()) < 2e-3 and float(torch.quantile(derr.flatten()[::7].double(), 0.99)) < 2e-2
    assert float(((dec[sel].cpu() > 0.4) != (want_dec > 0.4)).float().mean()) < 2e-3
    occ = (dec > 0.4).float().reshape(32, -1).mean(1).cpu().numpy()
    assert np.abs(occ - g["dec_occ_frac"]).max() < 5e-3
    # the encode -> decode bracket on in-distribution latents (the batch of 32 encoder means, |mu| <= 1.3): the tight bound
    dm = ldm.vae.decode(torch.from_numpy(g["enc_mu"]).cuda())
    merr = (dm[sel].cpu() - torch.from_numpy(g["dec_of_mu"]).float()).abs()
    assert float(merr.max()) < 5e-3 and float(merr.mean()) < 5e-4             # measured 1.9e-3 / 2.0e-4 (the fixture is fp16: 5e-4)
    dm2 = ldm.vae.decode(mu)                                                   # and through this build's own encoder
    merr2 = (dm2[sel].cpu() - torch.from_numpy(g["dec_of_mu"]).float()).abs()
    assert float(merr2.max()) < 3e-2 and float(merr2.mean()) < 3e-3
    got = voxel_tensor_to_point_clouds(dec, 0.4)
    assert [len(p) for p in got] == [int(v) for v in (dec > 0.4).reshape(32, -1).sum(1).cpu()]


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_latent_ddpm_1000_steps_vs_reference(ldm, golden, prec):
    """G23: the latent DDPM loop `LatentDiffusion.sample2(8, num_steps=1000)` (diffusion.py:575-616) with the reference's 999 per-step normal draws
    rebuilt from the integer hash: final latent against the one the reference handed its decoder (|z0| up to 7.9e3: an untrained denoiser under the
    ancestral update is a noise accumulation).  fp16 per-layer launches (the DDPM loop does not run in the persistent kernel): 5e-3; fp32 mode: 5e-5."""
    from shapegen_amd import specs
    g = golden("latent_ddpm.npz")

    class Noises:
        def __getitem__(self, k):
            return torch.from_numpy(specs.hash_normal(f"g23.z{k}", 8 * 256, 0).astype(np.float32).reshape(8, 256))

    ldm.model.set_precision(prec)
    try:
        _, z0 = ldm.sample2(8, num_steps=1000, z_T=torch.from_numpy(g["zT"]).cuda(), noises=Noises(), return_latent=True)
    finally:
        ldm.model.set_precision("fp16")
    r = rel_l2(z0.cpu(), g["z0"])
    print(f"latent DDPM T=1000 [{prec}]: rel-L2 {r:.2e}")
    assert r < (5e-3 if prec == "fp16" else 5e-5)


def test_latent_persistent_forward(ldm):
    """csrc/latent_persist.hip, forward mode: the whole network in ONE launch (weights resident in LDS, layers exchanged
    through self-validating buffers) against the per-layer launches and against the oracle, B = 32 / 5 / 1; repeated
    launches are bitwise identical (fixed summation order, no atomics)."""
    from oracle import torch_oracle as O
    if not ldm.model.persist_supported(32):
        pytest.skip("needs a 256-CU device")
    sd = latent_sd()
    g = torch.Generator().manual_seed(11)
    for b, tval in ((32, 0.73), (5, 0.31), (1, 1.0), (64, 0.5), (41, 0.2)):      # > 32 rows: two interleaved streams (rows 0 .. 31 | the rest)
        z = (torch.randn(b, 256, generator=g) * 1.2).cuda()
        t = torch.full((b,), tval)
        tb = ldm.model.time_bias(t[:1].cuda())
        eps = ldm.model.forward_persist(z, tb[0])
        ldm.model.check_persist_status()
        want_layers = ldm.model.forward_with_bias(z, tb[0], 0)
        want = O.latent_unet(sd, "model.", z.cpu(), t)
        assert torch.isfinite(eps).all()
        assert rel_l2(eps.cpu(), want) < 3e-3, b
        assert rel_l2(eps.cpu(), want_layers.cpu()) < 2e-3, b
        again = ldm.model.forward_persist(z, tb[0])
        assert torch.equal(again, eps)


def test_latent_persistent_ddim_steps(ldm):
    """... DDIM mode: T steps in ONE launch (state and update inside the kernel) against the Stepper over per-layer launches;
    the in-kernel update is pcd_ddim_update's arithmetic, so with the same eps the states would be bitwise equal -- the eps differ
    by fp32 summation order only.  Then 1000 steps twice: bitwise equal (a stale exchange read would show as a difference), and
    B < 32 rows, the linear schedule's per-row rates and `sample3` (last update skipped) take the same path."""
    from shapegen_amd.diffusion import LatentDiffusion
    if not ldm.model.persist_supported(32):
        pytest.skip("needs a 256-CU device")
    g = torch.Generator().manual_seed(12)
    zT = torch.randn(32, 256, generator=g).cuda()
    assert LatentDiffusion.use_persistent or True
    try:
        ldm.use_persistent = True
        _, a = ldm.sample(32, num_steps=20, z_T=zT, return_latent=True)
        _, a1000 = ldm.sample(32, num_steps=1000, z_T=zT, return_latent=True)
        _, b1000 = ldm.sample(32, num_steps=1000, z_T=zT, return_latent=True)
        _, a5 = ldm.sample3(5, z=zT[:5], start_t=torch.ones(5) * 0.4, num_steps=9, return_latent=True)
        ldm.use_persistent = False
        _, want = ldm.sample(32, num_steps=20, z_T=zT, return_latent=True)
        _, want1000 = ldm.sample(32, num_steps=1000, z_T=zT, return_latent=True)
        _, want5 = ldm.sample3(5, z=zT[:5], start_t=torch.ones(5) * 0.4, num_steps=9, return_latent=True)
    finally:
        ldm.use_persistent = LatentDiffusion.use_persistent
    assert torch.isfinite(a).all() and rel_l2(a.cpu(), want.cpu()) < 2e-3
    # 33 .. 64 rows: two streams interleaved by every workgroup in a fixed order; rows 0 .. 31 must come out as a 32-row call's
    g2 = torch.Generator().manual_seed(13)
    z64 = torch.randn(64, 256, generator=g2).cuda()
    try:
        ldm.use_persistent = True
        _, p64 = ldm.sample(64, num_steps=200, z_T=z64, return_latent=True)
        _, p64b = ldm.sample(64, num_steps=200, z_T=z64, return_latent=True)
        _, p45 = ldm.sample(45, num_steps=30, z_T=z64[:45], return_latent=True)
        _, p32 = ldm.sample(32, num_steps=200, z_T=z64[:32], return_latent=True)
        ldm.use_persistent = False
        _, w64 = ldm.sample(64, num_steps=200, z_T=z64, return_latent=True)
        _, w45 = ldm.sample(45, num_steps=30, z_T=z64[:45], return_latent=True)
    finally:
        ldm.use_persistent = LatentDiffusion.use_persistent
    assert torch.equal(p64, p64b)
    assert torch.equal(p64[:32], p32)                     # a stream's rows do not depend on the other stream
    assert rel_l2(p64.cpu(), w64.cpu()) < 3e-3 and rel_l2(p45.cpu(), w45.cpu()) < 2e-3
    assert torch.equal(a1000, b1000)
    assert rel_l2(a1000.cpu(), want1000.cpu()) < 5e-3
    assert rel_l2(a5.cpu(), want5.cpu()) < 2e-3


def test_latent_persistent_launch_fails_soft(ldm):
    """A persistent launch that cannot complete is not an error: with a fault injected -- one workgroup
    leaves at step 3, as a workgroup that never became resident would -- every wait inside gives up within its bound, the
    status word is set, and `LatentDiffusion._run` re-runs the loop from its saved start state on the per-layer launches with
    ONE warning and stays on them.  The result is bitwise the per-layer path's; the caller's z_T is untouched."""
    from shapegen_amd.diffusion import LatentDiffusion
    if not ldm.model.persist_supported(32):
        pytest.skip("needs a 256-CU device")
    g = torch.Generator().manual_seed(21)
    zT = torch.randn(32, 256, generator=g).cuda()
    keep = zT.clone()
    try:
        ldm.use_persistent = False
        _, want = ldm.sample(32, num_steps=40, z_T=zT, return_latent=True)
        for wg, step, batch in ((77, 3, 32), (0, 0, 32), (200, 5, 48)):
            ldm.use_persistent = True
            ldm.model.inject_persist_fault(wg, step)
            with pytest.warns(RuntimeWarning, match="per-layer launches"):
                _, got = ldm.sample(batch, num_steps=40, z_T=zT[:batch] if batch <= 32 else torch.cat([zT, zT[:batch - 32]]), return_latent=True)
            assert ldm.model.persist_status() != 0                      # the abandoned launch said so
            assert ldm.use_persistent is False                          # and the module stays on the per-layer launches
            assert torch.equal(got[:32], want)
        ldm.model.inject_persist_fault(-1, -1)
        ldm.use_persistent = True
        _, ok = ldm.sample(32, num_steps=40, z_T=zT, return_latent=True)      # the kernel itself is fine afterwards
        assert ldm.model.persist_status() == 0 and ldm.use_persistent is True
        assert rel_l2(ok.cpu(), want.cpu()) < 2e-3
    finally:
        ldm.model.inject_persist_fault(-1, -1)
        ldm.use_persistent = LatentDiffusion.use_persistent
    assert torch.equal(zT, keep)


def test_latent_non_finite_rows_stay_in_their_rows(ldm):
    """z_T with an inf row and a NaN row: GroupNorm is per row (networks.py:984-1036), so every other row must come out
    bitwise as if the bad rows were not there.  The persistent kernel's exchange cannot carry non-finite state (a value is its
    own ready flag), so such a call is routed to the per-layer launches up front -- no timeout, no warning."""
    import warnings
    from shapegen_amd.diffusion import LatentDiffusion
    g = torch.Generator().manual_seed(22)
    zT = torch.randn(32, 256, generator=g).cuda()
    bad = zT.clone()
    bad[3, 10] = float("inf")
    bad[17] = float("nan")
    good_rows = [i for i in range(32) if i not in (3, 17)]
    try:
        ldm.use_persistent = False
        _, want = ldm.sample(32, num_steps=25, z_T=zT, return_latent=True)
        ldm.use_persistent = True
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _, got = ldm.sample(32, num_steps=25, z_T=bad, return_latent=True)
        assert ldm.use_persistent is True                                # nothing timed out
    finally:
        ldm.use_persistent = LatentDiffusion.use_persistent
    assert torch.equal(got[good_rows], want[good_rows])
    assert not torch.isfinite(got[3]).all() and not torch.isfinite(got[17]).all()


def test_latent_sample2_sample3_and_errors(ldm):
    from oracle import torch_oracle as O
    from shapegen_amd.diffusion import LatentDiffusion
    sd = latent_sd()
    g = torch.Generator().manual_seed(3)
    zT = torch.randn(3, 256, generator=g)
    zs = torch.randn(7, 3, 256, generator=g)
    model = lambda z, t: O.latent_unet(sd, "model.", z, t)
    want = O.ddpm_sample(model, zT, 8, list(zs))
    _, z0 = ldm.sample2(3, num_steps=8, z_T=zT.cuda(), noises=zs.cuda(), return_latent=True)
    assert rel_l2(z0.cpu(), want) < 5e-3
    want = O.ddim_from_state(model, zT, torch.ones(3) * 0.3, 12)
    _, z0 = ldm.sample3(3, z=zT.cuda(), start_t=torch.ones(3) * 0.3, num_steps=12, return_latent=True)
    assert rel_l2(z0.cpu(), want) < 5e-3
    from shapegen_amd.vae import VAE3DLarge
    bad = LatentDiffusion(VAE3DLarge(), is_voxel_based=False).to("cuda")   # a fresh VAE: construction re-initialises its heads (a16)
    with pytest.raises(UnboundLocalError):      # reference diffusion.py:650-653 behaviour
        bad.sample(1, num_steps=1)


def test_vae3d_small(golden):
    """the small VAE3D on the same implicit-GEMM kernel (stride-2 convs, k3 transposed
    convs as parity classes with 1/2/4/8 taps, Cout=1 transposed last layer)."""
    from helpers import vae3d_small_sd
    from shapegen_amd.vae import VAE3D
    g = golden("vae3d_small.npz")
    vae = VAE3D()
    vae.load_state_dict(vae3d_small_sd(), strict=True)
    vae = vae.to("cuda").eval()
    vox = voxels_from_idx([g["occ_idx0"], g["occ_idx1"]]).cuda()
    mu, logvar = vae.encode(vox)
    assert rel_l2(mu.cpu(), g["mu"]) < 3e-3 and rel_l2(logvar.cpu(), g["logvar"]) < 3e-3
    dec = vae.decode(torch.from_numpy(g["mu"]).cuda())
    err = (dec.cpu() - torch.from_numpy(g["dec"])).abs()
    assert dec.shape == (2, 1, 32, 32, 32) and float(err.max()) < 5e-3 and float(err.mean()) < 5e-4
    pcs = vae.sample(2, threshold=0.4, z=torch.from_numpy(g["mu"]).cuda())
    assert len(pcs) == 2 and all(p.shape[1] == 3 for p in pcs)


@pytest.mark.parametrize("k1,k2,c,mode,m", [(256, 0, 128, 0, 32), (128, 0, 256, 0, 5), (256, 0, 512, 0, 70), (128, 0, 1024, 0, 32),
                                            (512, 256, 256, 0, 33), (256, 128, 128, 0, 32), (128, 0, 128, 1, 32),
                                            (128, 0, 256, 2, 256)])
def test_skinny_fused_layer(k1, k2, c, mode, m):
    """One-launch Linear + bias (+ per-row bias) + GroupNorm(8) + ReLU against torch in fp32 on the same fp16 inputs,
    and against the split-K + finish pair it replaces (same inputs, same math, different summation order)."""
    from shapegen_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(k1 + c + m)
    a1 = torch.randn(m, k1, generator=g).half()
    a2 = torch.randn(m, k2, generator=g).half() if k2 else None
    w = (torch.randn(c, k1 + k2, generator=g) / (k1 + k2) ** 0.5).half()
    bias, rb = torch.randn(c, generator=g) * 0.2, torch.randn(m, c, generator=g) * 0.2
    gamma, beta = 1 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    assert lib.pcd_skinny_fused_supported(k1 + k2, c, mode, 8) == 1
    a = torch.cat([a1, a2], 1) if k2 else a1
    z = a.float() @ w.float().T + bias + rb
    if mode == 0:
        want = torch.relu(F.group_norm(z, 8, gamma, beta, eps=1e-5))
    else:
        want = torch.relu(z) if mode == 1 else z
    d = lambda t: None if t is None else t.cuda().contiguous()
    da1, da2, dw, db, drb, dg, dbt = d(a1), d(a2), d(w), d(bias), d(rb), d(gamma), d(beta)
    o16 = torch.empty(m, c, dtype=torch.float16, device="cuda")
    o32 = torch.empty(m, c, dtype=torch.float32, device="cuda")
    _lib.check(lib.pcd_skinny_fused(da1.data_ptr(), k1, _lib.ptr(da2), k2, dw.data_ptr(), k1 + k2, m, c, db.data_ptr(),
                                    drb.data_ptr(), mode, 8, dg.data_ptr(), dbt.data_ptr(), o16.data_ptr(), o32.data_ptr(),
                                    _lib.stream_ptr()))
    got = (o32 if mode == 2 else o16).float().cpu()
    tol = 2e-6 * float(want.abs().max()) + 1e-5 if mode == 2 else 2e-3 * max(1.0, float(want.abs().max()))
    assert (got - want).abs().max() <= tol
    # the two-launch form on the same operands
    ns = lib.pcd_skinny_slabs(k1 + k2, c)
    slabs = torch.empty(ns, m, c, dtype=torch.float32, device="cuda")
    p16, p32 = torch.empty_like(o16), torch.empty_like(o32)
    _lib.check(lib.pcd_skinny_gemm_f16(da1.data_ptr(), k1, _lib.ptr(da2), k2, dw.data_ptr(), k1 + k2, m, c,
                                       slabs.data_ptr(), _lib.stream_ptr()))
    _lib.check(lib.pcd_skinny_finish(slabs.data_ptr(), ns, m, c, db.data_ptr(), drb.data_ptr(), mode, 8, dg.data_ptr(),
                                     dbt.data_ptr(), p16.data_ptr(), p32.data_ptr(), _lib.stream_ptr()))
    pair = (p32 if mode == 2 else p16).float().cpu()
    assert (got - pair).abs().max() <= (1e-5 if mode == 2 else 2e-3) * max(1.0, float(want.abs().max()))
    # shapes the fused form does not take
    assert lib.pcd_skinny_fused_supported(2048, 4096, 0, 8) == 0 and lib.pcd_skinny_fused_supported(96, 128, 0, 8) == 0


@pytest.mark.parametrize("k1,k2,c,m", [(512, 0, 1024, 32), (2048, 0, 4096, 32), (4096, 1024, 1024, 32), (1024, 512, 512, 7),
                                        (1024, 0, 2048, 1)])
def test_skinny_gemm_lds_dma_is_bitwise_the_register_form(k1, k2, c, m):
    """The split-K weight-streaming GEMM with both operands staged through LDS by LDS-DMA (full 128-byte lines, swizzled
    images) against the register-fragment form it replaces: identical products and summation order, so identical bits."""
    from shapegen_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(k1 + c + m)
    a1 = torch.randn(m, k1, generator=g).half().cuda()
    a2 = torch.randn(m, k2, generator=g).half().cuda() if k2 else None
    w = (torch.randn(c, k1 + k2, generator=g) / (k1 + k2) ** 0.5).half().cuda()
    ns = lib.pcd_skinny_slabs(k1 + k2, c)
    outs = []
    for dma in (1, 0):
        _lib.check(lib.pcd_skinny_config(dma))
        slabs = torch.full((ns, m, c), float("nan"), dtype=torch.float32, device="cuda")
        try:
            _lib.check(lib.pcd_skinny_gemm_f16(a1.data_ptr(), k1, _lib.ptr(a2), k2, w.data_ptr(), k1 + k2, m, c, slabs.data_ptr(),
                                               _lib.stream_ptr()))
        finally:
            _lib.check(lib.pcd_skinny_config(1))
        outs.append(slabs.cpu())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    a = torch.cat([a1, a2], 1) if k2 else a1
    want = a.float().cpu() @ w.float().cpu().T
    assert (outs[0].sum(0) - want).abs().max() <= 2e-3 * max(1.0, float(want.abs().max()))


def test_skinny_fused_fp32_input_equals_converted_input():
    """enc1 of the latent denoiser reads the fp32 state directly: same bits as converting to fp16 first."""
    from shapegen_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    m, k, c = 37, 256, 128
    a = (torch.randn(m, k, generator=g) * 3).cuda()
    a[0, 0], a[1, 5] = 1e6, -1e6                                       # saturate, like pcd_f32_to_f16
    w = (torch.randn(c, k, generator=g) / 16).half().cuda()
    bias, gamma, beta = (torch.randn(c, generator=g).cuda() for _ in range(3))
    a16 = torch.empty(m, k, dtype=torch.float16, device="cuda")
    _lib.check(lib.pcd_f32_to_f16(a.data_ptr(), a16.data_ptr(), a.numel(), _lib.stream_ptr()))
    o1, o2 = (torch.empty(m, c, dtype=torch.float16, device="cuda") for _ in range(2))
    _lib.check(lib.pcd_skinny_fused(a16.data_ptr(), k, 0, 0, w.data_ptr(), k, m, c, bias.data_ptr(), 0, 0, 8,
                                    gamma.data_ptr(), beta.data_ptr(), o1.data_ptr(), 0, _lib.stream_ptr()))
    _lib.check(lib.pcd_skinny_fused_f32in(a.data_ptr(), k, w.data_ptr(), k, m, c, bias.data_ptr(), 0, 0, 8,
                                          gamma.data_ptr(), beta.data_ptr(), o2.data_ptr(), 0, _lib.stream_ptr()))
    assert torch.equal(o1, o2)
