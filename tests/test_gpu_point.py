"""Parity of the point-cloud denoiser and the three samplers (HIP path through the C ABI)
against golden vectors from the reference and against the CPU oracle.

Tolerances (fp16 operands, fp32 accumulation):
  eps of one forward:  rel-L2 <= 3e-3
  sampler outputs:     rel-L2 <= 2e-3 on the cosine schedule (measured 1.5e-4 .. 2.8e-4; 5e-3 on the linear-schedule fixtures), Chamfer delta <= 1e-4 (north_star)
"""
import numpy as np
import pytest
import torch

from helpers import point_sd, rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EPS_TOL = 3e-3


@pytest.fixture(scope="module")
def model():
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=512)
    m.load_state_dict(point_sd(), strict=True)
    return m.to("cuda").eval()


def test_state_dict_contract(model):
    from shapegen_amd import specs
    want = [(k, s) for k, s, _ in specs.unet_pointnet_large_spec(prefix="model.")]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == want


def test_time_embedding(model, golden):
    g = golden("point_unet.npz")
    got = model.model.time_mlp_out(torch.from_numpy(g["temb_t"]).cuda()).cpu()
    np.testing.assert_allclose(got.numpy(), g["temb_mlp"], rtol=2e-5, atol=2e-5)


def test_forward_small_with_taps(model, golden):
    g = golden("point_unet.npz")
    x, t = torch.from_numpy(g["fw_small_x"]).cuda(), torch.from_numpy(g["fw_small_t"]).cuda()
    eps_plain = model.model(x, t).cpu()
    model.model.capture_decoder(2, 64)                  # keep dec4..dec1 (ping-pong buffers / inside the chained tail otherwise)
    try:
        eps = model.model(x, t).cpu()
        for name, ref in (("x1", "enc1"), ("x2", "enc2"), ("x3", "enc3"), ("x4", "enc4"), ("d4", "dec4"), ("d3", "dec3"),
                          ("d2", "dec2"), ("d1", "dec1")):
            tap = model.model.tap(name, 2, 64).float().cpu().transpose(1, 2)   # (B,C,N) like the reference
            assert rel_l2(tap, g["fw_small_" + ref]) < 2e-3, name
    finally:
        model.model.capture_decoder(2, 64, on=False)
    assert torch.equal(eps, eps_plain)                  # the capture changes nothing (the unchained tail is bit-identical)
    assert rel_l2(model.model.tap("pooled", 2, 64).cpu(), g["fw_small_pooled"]) < 2e-3
    assert rel_l2(eps, g["fw_small_eps"]) < EPS_TOL
    with pytest.raises(RuntimeError):
        model.model.tap("d4", 2, 64)


def test_forward_mid_per_shape_time(model, golden):
    g = golden("point_unet.npz")
    eps = model.model(torch.from_numpy(g["fw_mid_x"]).cuda(), torch.from_numpy(g["fw_mid_t"]).cuda()).cpu()
    assert rel_l2(eps, g["fw_mid_eps"]) < EPS_TOL
    assert float((eps - torch.from_numpy(g["fw_mid_eps"])).abs().max()) < 5e-3


@pytest.mark.parametrize("B,N", [(2, 64), (3, 100), (1, 257), (5, 512)])
def test_chained_narrow_layers_match_per_layer_launches(model, B, N):
    """pcd_unet_forward runs enc1, enc2.conv1-2 and dec1.conv2..output.3 as LDS-resident chains (csrc/chain.hip);
    pcd_unet_config(0) selects one GEMM launch per layer.  Both sum the same fp16 products in fp32 in the same k order
    and round once per layer, so eps and the x1 tap agree bit for bit - on whole and on ragged 256-point tiles."""
    from shapegen_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(B * 1000 + N)
    x = torch.randn(B, N, 3, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    default_mask = model.model.hilo_mask
    assert default_mask == _lib.PCD_UNET_HILO_ALLOWED                  # hi / lo weights on the narrow layers are the default
    eps_by_mask = {}
    try:
        for mask in (default_mask, 0):                  # with hi / lo weights (K loop run twice: all hi, then all lo, in both forms) and without
            model.model.set_hilo_mask(mask)
            _lib.check(lib.pcd_unet_config(1))          # narrow chains only (the 256-channel chains sum in another order)
            eps_chain = model.model(x, t).clone()
            x1_chain = model.model.tap("x1", B, N).clone()
            _lib.check(lib.pcd_unet_config(0))
            eps_layers = model.model(x, t).clone()
            x1_layers = model.model.tap("x1", B, N).clone()
            assert torch.isfinite(eps_chain).all()
            assert torch.equal(x1_chain, x1_layers), mask
            assert torch.equal(eps_chain, eps_layers), mask
            eps_by_mask[mask] = eps_chain
    finally:
        _lib.check(lib.pcd_unet_config(3))
        model.model.set_hilo_mask(default_mask)
    r = rel_l2(eps_by_mask[0].cpu(), eps_by_mask[default_mask].cpu())
    assert 1e-6 < r < 3e-3                              # the two weight precisions differ by the fp16 rounding of six narrow layers' weights


@pytest.mark.parametrize("chain", [0, 1])
def test_wide_chain_exact_on_integers(chain):
    """csrc/widechain.hip: enc3 (256 -> 256 -> 256 -> 512) and dec2 ([256 | 256] -> 256 -> 256 -> 128) with the activations in
    registers between the layers.  Small-integer weights, biases and inputs make every product and sum exact in fp16 / fp32,
    so the result must equal the float64 chain of relu(x W^T + b) exactly -- any mistake in the fragment regrouping
    (v_permlane32_swap), the packed stage order or the ring shows as a wrong integer."""
    from shapegen_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(40 + chain)
    m = 1024 + 256
    shapes = [(256, 256), (256, 256), (512, 256)] if chain == 0 else [(256, 512), (256, 256), (128, 256)]
    ws = [torch.randint(-1, 2, s_, generator=g).float() * (torch.rand(s_, generator=g) < 0.06).float() for s_ in shapes]
    bs = [torch.randint(-2, 3, (s_[0],), generator=g).float() for s_ in shapes]
    x1 = torch.randint(0, 3, (m, 256), generator=g).float()
    x2 = torch.randint(0, 3, (m, 256), generator=g).float()
    a = torch.cat([x1, x2], 1).double() if chain == 1 else x1.double()
    for w, b in zip(ws, bs):
        a = torch.relu(a @ w.double().T + b.double())
        assert float(a.max()) < 2048                                   # exactly representable in fp16
    dw = [w.half().cuda().contiguous() for w in ws]
    db = [b.cuda().contiguous() for b in bs]
    packed = torch.empty(int(lib.pcd_pw_wide_packed_bytes(chain)), dtype=torch.uint8, device="cuda")
    import ctypes as C
    wp = (C.c_void_p * 3)(*[t.data_ptr() for t in dw])
    bp = (C.c_void_p * 3)(*[t.data_ptr() for t in db])
    _lib.check(lib.pcd_pw_wide_pack(chain, wp, bp, packed.data_ptr(), _lib.stream_ptr()))
    out = torch.full((m, shapes[2][0]), -1.0, dtype=torch.float16, device="cuda")
    d1, d2 = x1.half().cuda(), x2.half().cuda()
    _lib.check(lib.pcd_pw_wide_chain(chain, d1.data_ptr(), d2.data_ptr() if chain == 1 else 0, m, packed.data_ptr(), out.data_ptr(),
                                     _lib.stream_ptr()))
    assert torch.equal(out.double().cpu(), a)
    assert lib.pcd_pw_wide_chain(chain, d1.data_ptr(), d2.data_ptr(), 100, packed.data_ptr(), out.data_ptr(), _lib.stream_ptr()) != 0


def test_wide_chains_in_the_forward(model):
    """pcd_unet_forward with the 256-channel chains on (default) against one GEMM launch per layer for the same six layers: the same
    fp16 operands, fp32 sums in another order, one fp16 rounding per layer either way."""
    from shapegen_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 512, 3, generator=g).cuda()
    t = torch.rand(2, generator=g).cuda()
    eps_wide = model.model(x, t).clone()
    x3_wide = model.model.tap("x3", 2, 512).clone()
    _lib.check(lib.pcd_unet_config(1))
    try:
        eps_layers = model.model(x, t).clone()
        x3_layers = model.model.tap("x3", 2, 512).clone()
    finally:
        _lib.check(lib.pcd_unet_config(3))
    assert torch.isfinite(eps_wide).all()
    assert rel_l2(x3_wide.float().cpu(), x3_layers.float().cpu()) < 1e-3
    assert rel_l2(eps_wide.cpu(), eps_layers.cpu()) < 1e-3


def test_forward_ragged_sizes(model):
    """N not a multiple of any tile (exercises row masking and the slow column-max path)."""
    from oracle import torch_oracle as O
    sd = point_sd()
    gen = torch.Generator().manual_seed(5)
    for b, n in ((1, 1), (3, 100), (2, 257)):
        x = torch.randn(b, n, 3, generator=gen)
        t = torch.rand(b, generator=gen)
        want = O.unet_pointnet_large(sd, "model.", x, t)
        got = model.model(x.cuda(), t.cuda()).cpu()
        assert rel_l2(got, want) < EPS_TOL, (b, n)


@pytest.mark.parametrize("T", [5, 50, 100])
def test_ddim_sample(model, golden, T):
    from shapegen_amd import metrics as M
    g = golden("point_samplers.npz")
    out = model.sample(4, 512, num_steps=T, x_T=torch.from_numpy(g[f"sample_T{T}_xT"]).cuda())
    want = torch.from_numpy(g[f"sample_T{T}_out"])
    assert rel_l2(out.cpu(), want) < 2e-3
    # north_star quality gate, SURVEY 8(c): |CD_build - CD_ref| <= 1e-4 (scaling 1) against the same
    # third cloud; CD(gpu cloud, reference cloud) itself is reported, not gated at 1e-4
    other = torch.from_numpy(g[f"sample_T{T}_xT"]).cuda()
    cd_build = float(M.chamfer_distance(out, other, 1))
    cd_ref = float(M.chamfer_distance(want.cuda(), other, 1))
    assert abs(cd_build - cd_ref) < 1e-4, (cd_build, cd_ref)
    cd_pair = float(M.chamfer_distance(out, want.cuda(), 1))
    print(f"T={T}: CD(gpu,ref)={cd_pair:.3e}  CD_build={cd_build:.6f} CD_ref={cd_ref:.6f}")
    assert cd_pair < 2e-3


def test_ddim_sample_chamfer_gate_at_2048_points(golden):
    """The north star's quality gate at BASELINE's point count (G18: the reference's `sample(2, 2048, num_steps=50)`):
    |CD_build - CD_ref| <= 1e-4 (scaling 1) against the same third cloud, cloud rel-L2 <= 5e-3; CD(gpu cloud, reference
    cloud) itself is printed (fp16 operands put it at a few 1e-4, above the oracle's own cdist floor of 8e-5)."""
    from shapegen_amd import metrics as M
    from shapegen_amd.diffusion import PointCloudDiffusion
    g = golden("point_n2048.npz")
    m = PointCloudDiffusion(num_points=2048)
    m.load_state_dict(point_sd(), strict=True)
    m = m.to("cuda").eval()
    out = m.sample(2, 2048, num_steps=50, x_T=torch.from_numpy(g["xT"]).cuda())
    want = torch.from_numpy(g["out"])
    assert rel_l2(out.cpu(), want) < 2e-3
    other = torch.from_numpy(g["xT"]).cuda()
    cd_build = float(M.chamfer_distance(out, other, 1))
    cd_ref = float(M.chamfer_distance(want.cuda(), other, 1))
    cd_pair = float(M.chamfer_distance(out, want.cuda(), 1))
    print(f"N=2048 T=50: CD(gpu,ref)={cd_pair:.3e}  CD_build={cd_build:.6f} CD_ref={cd_ref:.6f}")
    assert abs(cd_build - cd_ref) < 1e-4, (cd_build, cd_ref)
    assert cd_pair < 2e-3


def test_ddpm_sample2(model, golden):
    g = golden("point_samplers.npz")
    out = model.sample2(2, 64, num_steps=20, x_T=torch.from_numpy(g["s2_xT"]).cuda(),
                        noises=torch.from_numpy(g["s2_z"]).cuda())
    assert rel_l2(out.cpu(), g["s2_out"]) < 2e-3


class _HashedNoises:
    def __init__(self, tag, shape):
        self.tag, self.shape = tag, tuple(shape)

    def __getitem__(self, k):
        from shapegen_amd import specs
        return torch.from_numpy(specs.hash_normal(f"{self.tag}{k}", int(np.prod(self.shape)), 0).astype(np.float32).reshape(self.shape))


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_baseline_config0_as_ddpm(golden, prec):
    """G22: BASELINE configs[0] read literally -- point-cloud DDPM, 512 points, 100 steps, batch 4 -- through `sample2` (the reference's own script
    runs the DDIM `sample` at this shape: test_ddim_sample[T=100]); the 99 per-step noise tensors are rebuilt from the integer hash; synthetic
    weights at gain 1.0 (tests/test_gpu_point_t1000.py explains why the DDPM fixtures use that scale).  fp16 product path and fp32 parity mode."""
    from helpers import as_torch
    from shapegen_amd import metrics as M, specs
    from shapegen_amd.diffusion import PointCloudDiffusion
    g = golden("point_cfg1_ddpm.npz")
    m = PointCloudDiffusion(num_points=512)
    m.load_state_dict(as_torch(specs.synth_state_dict(specs.unet_pointnet_large_spec(prefix="model."), seed=0, gain=float(g["gain"]))), strict=True)
    m = m.to("cuda").eval()
    m.model.set_precision(prec)
    xT = torch.from_numpy(g["xT"]).cuda()
    out = m.sample2(4, 512, num_steps=100, x_T=xT, noises=_HashedNoises("g22.z", (4, 512, 3)))
    want = torch.from_numpy(g["out"])
    r = rel_l2(out.cpu(), want)
    cd_build, cd_ref = float(M.chamfer_distance(out, xT, 1)), float(M.chamfer_distance(want.cuda(), xT, 1))
    print(f"configs[0] as DDPM [{prec}]: rel-L2 {r:.2e}  |dCD| {abs(cd_build - cd_ref):.2e}")
    assert r < (2e-3 if prec == "fp16" else 5e-5)
    assert abs(cd_build - cd_ref) < 1e-4


def test_sample3_reconstruction(model, golden):
    """test_point_ddpm.py:78-80: add_noise at t=0.01 then 1000 DDIM steps back."""
    g = golden("point_samplers.npz")
    x0 = torch.from_numpy(g["s3_x0"]).cuda()
    t = torch.ones(2, device="cuda") * 0.01
    noisy, noise, n, s = model.add_noise(x0, t, noise=torch.from_numpy(g["s3_noise"]).cuda())
    assert torch.equal(noisy.cpu(), torch.from_numpy(g["s3_noisy"]))          # elementwise: bit exact
    out = model.sample3(2, 64, x=noisy, start_t=t)
    assert rel_l2(out.cpu(), g["s3_out"]) < 2e-3
    out = model.sample3(2, 64, x=noisy, start_t=torch.ones(2), num_steps=20)
    assert rel_l2(out.cpu(), g["s3_T20_from1_out"]) < 2e-3


def test_step_tables_bit_exact(model, golden):
    """Per-step constants: bit-identical to the oracle's reference-order torch ops evaluated on this
    host, and within 1 ulp of the golden tables captured on the build container (libm/ISA of the
    host CPU decides the last bit of sin/cos/sqrt, exactly as it would for the reference)."""
    from oracle import torch_oracle as O
    g = golden("schedule.npz")
    dummy = lambda x, t: torch.zeros_like(x)

    def rows(tab):
        return torch.stack([tab.t, tab.n[:, 0], tab.s[:, 0], tab.a[:, 0], tab.b[:, 0]], 1).cpu().numpy()

    for T in (50, 100, 1000):
        tr = []
        O.ddim_sample(dummy, torch.zeros(1, 1, 3), T, trace=tr)
        got = rows(model.ddim_table(T))
        assert np.array_equal(got, np.asarray(tr, np.float32))
        np.testing.assert_allclose(got, g[f"sample_T{T}"], rtol=2.5e-7, atol=1e-9)
        tr = []
        O.ddpm_sample(dummy, torch.zeros(1, 1, 3), T, [torch.zeros(1, 1, 3)] * (T - 1), trace=tr)
        tr = np.asarray(tr, np.float32)
        got = rows(model.ddpm_table(T))
        assert np.array_equal(got[:, :3], tr[:, :3]) and np.array_equal(got[:-1, 4], tr[:-1, 4])
        np.testing.assert_allclose(got[:-1, 3], np.sqrt(tr[:-1, 3] / tr[:-1, 1]), rtol=2.5e-7)   # sqrt(n_prev/n)
        np.testing.assert_allclose(got[:-1], g[f"sample2_T{T}"][:-1], rtol=2.5e-7, atol=1e-9)
    tr = []
    O.ddim_from_state(dummy, torch.zeros(2, 1, 3), torch.ones(2) * 0.01, 1000, trace=tr)
    got = rows(model.from_state_table(0.01, 1000))
    assert np.array_equal(got[:-1], np.asarray(tr, np.float32)[:-1])
    np.testing.assert_allclose(got[:-1], g["sample3_T1000_from0.01"][:-1], rtol=2.5e-7, atol=1e-9)


def test_full_size_properties(model):
    """BASELINE config 2 size (B=64, N=2048): properties that need no CPU run."""
    gen = torch.Generator().manual_seed(24)
    x = torch.randn(64, 2048, 3, generator=gen).cuda()
    t = torch.full((64,), 0.5, device="cuda")
    eps = model.model(x, t)
    assert torch.isfinite(eps).all()
    # shapes are independent: a batch slice gives the same answer
    sub = model.model(x[5:9].contiguous(), t[5:9].contiguous())
    assert rel_l2(sub.cpu(), eps[5:9].cpu()) < 1e-6
    # permutation equivariance over points (pointwise net + symmetric max-pool)
    perm = torch.randperm(2048, generator=gen).cuda()
    eps_p = model.model(x[:2, perm].contiguous(), t[:2].contiguous())
    assert rel_l2(eps_p.cpu(), eps[:2, perm].cpu()) < 1e-6


def test_full_size_forward_next_to_the_oracle(model):
    """The launch bench.py times (B = 64, N = 2048: `gemm_xp_kernel` on 512 whole tiles per layer with the XCD patch map,
    the wide chains at full grid, the fused column max over 64 shapes) checked against the ORACLE, not against itself:
    shapes are independent, so rows 5..8 of the full batch must equal the oracle on those four shapes --
    eps and the x3 / x4 / pooled / d4 / d2 taps."""
    from oracle import torch_oracle as O
    sd = point_sd()
    gen = torch.Generator().manual_seed(64)
    x = torch.randn(64, 2048, 3, generator=gen)
    t = torch.rand(64, generator=gen)
    model.model.capture_decoder(64, 2048)
    try:
        eps = model.model(x.cuda(), t.cuda()).cpu()
        taps_hip = {k: model.model.tap(k, 64, 2048)[5:9].float().cpu() for k in ("x3", "x4", "d4", "d2")}
        pooled = model.model.tap("pooled", 64, 2048)[5:9].cpu()
    finally:
        model.model.capture_decoder(64, 2048, on=False)
    taps = {}
    want = O.unet_pointnet_large(sd, "model.", x[5:9], t[5:9], taps=taps)
    assert rel_l2(eps[5:9], want) < EPS_TOL
    assert rel_l2(pooled, taps["pooled"]) < 2e-3
    for k, v in taps_hip.items():
        assert rel_l2(v.transpose(1, 2), taps[k]) < 2.5e-3, k
    # and two more shapes at the far end of the batch (last XCD patch, last tiles)
    want = O.unet_pointnet_large(sd, "model.", x[62:64], t[62:64])
    assert rel_l2(eps[62:64], want) < EPS_TOL


def _forward_with_taps(model, x, t, shapes):
    """eps of the whole batch, and the x3 / x4 / d4 / d2 / pooled taps of `shapes`, on the host."""
    b, n = x.shape[:2]
    model.model.capture_decoder(b, n)
    try:
        eps = model.model(x.cuda(), t.cuda()).cpu()
        taps = {k: model.model.tap(k, b, n)[shapes].float().cpu() for k in ("x3", "x4", "d4", "d2")}
        taps["pooled"] = model.model.tap("pooled", b, n)[shapes].cpu()
    finally:
        model.model.capture_decoder(b, n, on=False)
    return eps, taps


def _assert_next_to_the_oracle(eps, taps_hip, x, t, shapes):
    from oracle import torch_oracle as O
    taps = {}
    want = O.unet_pointnet_large(point_sd(), "model.", x[shapes], t[shapes], taps=taps)      # shapes are independent
    assert rel_l2(eps[shapes], want) < EPS_TOL
    assert rel_l2(taps_hip["pooled"], taps["pooled"]) < 2e-3
    for k in ("x3", "x4", "d4", "d2"):
        assert rel_l2(taps_hip[k].transpose(1, 2), taps[k]) < 2.5e-3, k


def test_ragged_batch_forward_next_to_the_oracle(model):
    """B = 9, N = 2000: m = 18000 rows is past the 256 x 256 tile's threshold and no multiple of 256, so the wide chains are dropped and enc3, enc4,
    global_feat, dec4 and dec3 run on the ragged generic 256 x 256 tile -- the column max with 2000-row shapes (every maximum an atomic), dec4.conv1
    with a per-row per-shape bias.  Shapes 0, 1 and 8 (the last one owns the ragged rows) against the oracle; and the same three shapes as their own
    small batches (m <= 4000: 128 x 128 tiles), which must give what the big batch gave -- the bound is test_full_size_properties' for a batch slice."""
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(9, 2000, 3, generator=gen)
    t = torch.rand(9, generator=gen)
    shapes = [0, 1, 8]
    eps, taps = _forward_with_taps(model, x, t, shapes)
    assert torch.isfinite(eps).all()
    _assert_next_to_the_oracle(eps, taps, x, t, shapes)
    for sl in (slice(0, 2), slice(8, 9)):
        sub = model.model(x[sl].contiguous().cuda(), t[sl].contiguous().cuda()).cpu()
        print(f"B=9 N=2000, shapes {sl.start}..{sl.stop - 1} alone: rel-L2 to the big batch {rel_l2(sub, eps[sl]):.3e}, bitwise {torch.equal(sub, eps[sl])}")
        assert rel_l2(sub, eps[sl]) < 1e-6, sl


def test_straddling_batch_forward_next_to_the_oracle(model):
    """B = 32, N = 640: m = 20480 rows is whole 256-row tiles, but a shape is 2.5 of them, so tiles straddle shapes: global_feat.3 goes to
    gemm_xw_kernel (80 x 16 tiles, patches of 8 x 2) with the two wave tiles of one output tile in different shapes, the per-shape biases take the
    per-row path.  Shapes 0, 1, 30 and 31 against the oracle; then the forward with gemm_xw_kernel off and with gemm_xp_kernel off (checked at
    N = 2048 elsewhere), each bitwise the default."""
    from shapegen_amd import _lib
    lib = _lib.load()
    d = _lib.GemmDesc()                                                     # global_feat.3 at this batch: the plan reads no address
    d.a1 = d.w = d.bias = 64
    d.k1, d.lda1, d.ldw, d.relu, d.m, d.c = 2048, 2048, 2048, 1, 32 * 640, 4096
    plan = _lib.GemmPlan()
    _lib.check(lib.pcd_gemm_plan(d, 6, 640, 0, 1, plan), "gemm_plan")
    assert (plan.family, plan.tiles_m, plan.tiles_n, plan.patch_pn, plan.patch_xn) == (6, 80, 16, 8, 2)
    gen = torch.Generator().manual_seed(32)
    x = torch.randn(32, 640, 3, generator=gen)
    t = torch.rand(32, generator=gen)
    shapes = [0, 1, 30, 31]
    eps, taps = _forward_with_taps(model, x, t, shapes)
    assert torch.isfinite(eps).all()
    _assert_next_to_the_oracle(eps, taps, x, t, shapes)
    xd, td = x.cuda(), t.cuda()
    for off, on, name in ((8, 9, "gemm_xw_kernel"), (5, 7, "gemm_xp_kernel")):
        try:
            assert lib.pcd_gemm_set_config(off) == 0
            other = model.model(xd, td).cpu()
            pooled = model.model.tap("pooled", 32, 640)[shapes].cpu()
        finally:
            assert lib.pcd_gemm_set_config(on) == 0
        assert torch.equal(pooled, taps["pooled"]), name
        assert torch.equal(other, eps), name


def test_cpu_module_fails_loudly():
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=16)
    with pytest.raises(RuntimeError):
        m.sample(1, 16, num_steps=1)
    with pytest.raises(RuntimeError):
        m.model(torch.zeros(1, 16, 3), torch.zeros(1))


# ------------------------------------------------------------------ a2: the linear schedule on the GPU
@pytest.fixture(scope="module")
def linear_model():
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=128, noise_schedule="linear")
    m.load_state_dict(point_sd(), strict=True)
    return m.to("cuda").eval()


def test_linear_schedule_samplers(linear_model, golden):
    """`noise_schedule='linear'` (diffusion.py:189-205): the batch-axis cumprod gives every shape its own rates, so
    the step tables are (T, batch) and the update kernels run with per-shape rate stride 1.  The three samplers at
    (4, 128), T = 8 against the reference's outputs (G16) and the rate tables bit-exact on the device."""
    g = golden("linear.npz")
    m = linear_model
    tab = m.ddim_table(8, 4)
    assert tab.width == 4 and tab.stride == 1
    assert np.array_equal(torch.stack([tab.n, tab.s, tab.a, tab.b], dim=1).cpu().numpy(), g["sample_rates"])
    # sample2's table has a sqrt and a division: bit-identical to the oracle's reference-order torch ops on THIS host,
    # and within 1 ulp of the table captured on the build container (same convention as test_step_tables_bit_exact)
    from oracle import torch_oracle as O
    tab = m.ddpm_table(8, 4)
    got = torch.stack([tab.n, tab.s, tab.a, tab.b], dim=1).cpu().numpy()
    np.testing.assert_allclose(got, g["sample2_rates"], rtol=2.5e-7, atol=1e-9)
    for k, i in enumerate(reversed(range(8))):
        n, s = O.linear_schedule(torch.ones(4) * i / 8)
        want = [n, s, torch.zeros(4), torch.zeros(4)]
        if i > 0:
            npv, sp = O.linear_schedule(torch.ones(4) * (i - 1) / 8)
            want = [n, s, torch.sqrt(npv / n), sp]
        assert np.array_equal(got[k], torch.stack(want).numpy()), k
    out = m.sample(4, 128, num_steps=8, x_T=torch.from_numpy(g["sample_xT"]).cuda())
    assert rel_l2(out.cpu(), g["sample_out"]) < 5e-3
    out = m.sample2(4, 128, num_steps=8, x_T=torch.from_numpy(g["s2_xT"]).cuda(), noises=torch.from_numpy(g["s2_z"]).cuda())
    assert rel_l2(out.cpu(), g["s2_out"]) < 5e-3
    x0 = torch.from_numpy(g["s3_x0"]).cuda()
    t = torch.ones(4, device="cuda") * 0.3
    noisy, _, nr, sr = m.add_noise(x0, t, noise=torch.from_numpy(g["s3_noise"]).cuda())
    assert np.array_equal(torch.stack([nr, sr]).cpu().numpy(), g["s3_add_rates"])
    assert torch.equal(noisy.cpu(), torch.from_numpy(g["s3_noisy"]))                  # per-shape rates, bit exact
    out = m.sample3(4, 128, x=noisy, start_t=t, num_steps=8)
    assert rel_l2(out.cpu(), g["s3_out"]) < 5e-3


def test_linear_schedule_long_run_uses_graph_replay(linear_model):
    """T = 20 > GRAPH_MIN_STEPS: the (T, batch) tables go through the device-side step select inside replayed HIP
    graphs; against the oracle with `sched=linear_schedule`."""
    from oracle import torch_oracle as O
    sd = point_sd()
    g = torch.Generator().manual_seed(8)
    xT = torch.randn(3, 128, 3, generator=g)
    want = O.ddim_sample(lambda x, t: O.unet_pointnet_large(sd, "model.", x, t), xT, 20, sched=O.linear_schedule)
    assert linear_model.use_graphs and 20 - 1 >= linear_model.GRAPH_MIN_STEPS
    got = linear_model.sample(3, 128, num_steps=20, x_T=xT.cuda())
    assert rel_l2(got.cpu(), want) < 5e-3


def test_philox_stream_positions_across_graph_replays(model):
    """On-device noise of `sample2`: step k draws the counter block [base + k*stride, base + (k+1)*stride) whether it
    runs eagerly or inside a replayed graph (the draw reads k from the device-side counter), no block is used twice,
    and the owner's stream position advances by T*stride.  A zero-eps denoiser makes the final state a known function
    of every draw, recomputed here from pcd_randn at the expected offsets."""
    from shapegen_amd import _lib
    lib = _lib.load()
    B, N, T = 2, 64, 29                      # 1 eager + 3 graphs of 8 + 3 eager + the final no-update step
    torch.manual_seed(99)
    seed = int(torch.initial_seed())
    model._philox_offset = 1000
    g = torch.Generator().manual_seed(1)
    xT = torch.randn(B, N, 3, generator=g).cuda()
    tab = model.ddpm_table(T, B)
    zero_eps = lambda x, tb, eps: eps.zero_()
    assert model.use_graphs and T - 2 >= model.GRAPH_MIN_STEPS
    out = model._run(xT.clone(), tab, torch.zeros(T, 64, device="cuda"), zero_eps, "ddpm")
    stride = B * N * 3 // 4
    assert model._philox_offset == 1000 + stride * T
    x = xT.clone()
    draws = []
    for k in range(T):
        n, s, a, b = (float(v[k, 0]) for v in (tab.n, tab.s, tab.a, tab.b))
        x0 = x / torch.tensor(s)                                # remove_noise with eps = 0
        if k < T - 1:
            z = torch.empty_like(x)
            _lib.check(lib.pcd_randn(z.data_ptr(), z.numel(), seed, 1000 + k * stride, _lib.stream_ptr()))
            draws.append(z.clone())
            x = b * x0 + (a * n) * z
    assert rel_l2(out.cpu(), x0.cpu()) < 1e-5
    flat = torch.stack(draws).reshape(len(draws), -1)
    assert len({tuple(r[:8].tolist()) for r in flat.cpu()}) == len(draws)      # no counter block drawn twice
    # a sharded run reads the sub-block of its samples out of the same global draw (dist.shard_context)
    model._philox_offset = 1000
    from shapegen_amd import dist as D
    with D.shard_context(model, 1, B):
        part = model._randn_like(torch.empty(1, N, 3, device="cuda"))
    model._philox_offset = 1000
    whole = model._randn_like(torch.empty(B, N, 3, device="cuda"))
    assert torch.equal(part[0], whole[1])


def test_full_size_ddpm_on_device_noise_is_shard_invariant(model):
    """BASELINE config 2 size (B=64, N=2048) through `sample2` WITH the on-device Philox noise (graph replay): the
    noise of sample i is addressed by its global index (dist.shard_context), so running samples [40, 44) alone, as a
    rank of a sharded job would, reproduces rows 40..43 of the full-batch run -- a size-independent check of the
    whole loop (step select, forward, Philox draw, fused update) at the size bench.py times."""
    from shapegen_amd import dist as D
    torch.manual_seed(2024)
    model._philox_offset = 0
    full = model.sample2(64, 2048, num_steps=12)
    assert torch.isfinite(full).all() and float(full.abs().max()) < 1e3
    torch.manual_seed(2024)
    model._philox_offset = 0
    with D.shard_context(model, 40, 64):
        part = model.sample2(4, 2048, num_steps=12)
    assert rel_l2(part.cpu(), full[40:44].cpu()) < 1e-5
    assert not torch.equal(full[0], full[1])                       # samples really draw different noise
