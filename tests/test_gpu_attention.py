"""Set attention (flash-style HIP kernel + LN + FFN GEMMs) vs goldens from the reference's
nn.MultiheadAttention path and vs the CPU oracle at the BASELINE length N=2048.
Tolerance: fp16 operands / fp32 accumulation and softmax -> rel-L2 <= 3e-3 per block."""
import pytest
import torch

from helpers import sab_sd, una_sd, rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.mark.parametrize("C", [64, 128, 256])
def test_set_attention_block_golden(golden, C):
    from shapegen_amd.networks import SetAttentionBlock
    g = golden("attention.npz")
    blk = SetAttentionBlock(C, 4)
    blk.load_state_dict(sab_sd(C), strict=True)
    blk = blk.to("cuda").eval()
    out = blk(torch.from_numpy(g[f"sab{C}_x"]).cuda()).cpu()
    assert rel_l2(out, g[f"sab{C}_out"]) < 3e-3


@pytest.mark.parametrize("C,N,B", [(256, 2048, 2), (64, 2048, 1), (128, 333, 3), (256, 50, 2)])
def test_set_attention_block_vs_oracle(C, N, B):
    """Full BASELINE length and ragged lengths (N not a multiple of the 64-key tile / 128-query block)."""
    from shapegen_amd.networks import SetAttentionBlock
    from oracle import torch_oracle as O
    sd = sab_sd(C)
    blk = SetAttentionBlock(C, 4)
    blk.load_state_dict(sd, strict=True)
    blk = blk.to("cuda").eval()
    x = torch.randn(B, N, C, generator=torch.Generator().manual_seed(C + N)) * 1.5
    want = O.set_attention_block(sd, "", x, 4)
    assert rel_l2(blk(x.cuda()).cpu(), want) < 3e-3


def test_attention_kernel_softmax_rescale_path():
    """Online-softmax rescale branch: one key far larger than the rest, placed late, so the running
    max jumps in the last tile (cdna guide rule 26: force the data-dependent branch)."""
    from shapegen_amd import ops
    B, N, C, H = 1, 256, 64, 4
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B * N, 3 * C, generator=g) * 0.5
    qkv[200, C:2 * C] *= 12.0            # spike key 200 (third 64-key tile)
    q, k, v = qkv.half().float().split(C, dim=1)
    d = C // H
    qh, kh, vh = (z.reshape(N, H, d).permute(1, 0, 2).double() for z in (q, k, v))
    w = torch.softmax(qh @ kh.transpose(1, 2) / d ** 0.5, dim=-1)
    want = (w @ vh).permute(1, 0, 2).reshape(N, C)
    got = ops.set_attention_f16(qkv.half().cuda(), B, N, C, H).float().cpu()
    assert rel_l2(got, want) < 2e-3


def _attention_fp64(qkv16, B, N, C, H):
    q, k, v = qkv16.float().split(C, dim=1)
    d = C // H
    qh, kh, vh = (z.reshape(B, N, H, d).permute(0, 2, 1, 3).double() for z in (q, k, v))
    w = torch.softmax(qh @ kh.transpose(2, 3) / d ** 0.5, dim=-1)
    return (w @ vh).permute(0, 2, 1, 3).reshape(B * N, C)


@pytest.mark.parametrize("pattern", ["plain", "late_spike", "rising", "falling", "huge_first"])
def test_attention_pipelined_kernel_d64(pattern):
    """The software-pipelined d = 64 kernel (N % 256 == 0) runs its softmax without tracking the row max per tile:
    force its rare path (a tile whose scores overflow the optimistic bound) in every position, rows that never
    take it, score ranges that move up or down along the keys, and compare with fp64 and with the generic kernel."""
    from shapegen_amd import _lib, ops
    B, N, C, H = 2, 512, 256, 4
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * N, 3 * C, generator=g)
    k = qkv[:, C:2 * C]
    if pattern == "late_spike":
        k[N + 400] *= 14.0                       # shape 1, key 400: far above the running max, in tile 6
        k[37] *= 9.0                             # shape 0, key 37: second sub-tile
    elif pattern == "rising":                    # key norms grow along the sequence: the max moves at many tiles
        k *= torch.linspace(0.2, 6.0, N).repeat(B)[:, None]
    elif pattern == "falling":                   # the first tile holds the max: later P underflow towards 0
        k *= torch.linspace(8.0, 0.1, N).repeat(B)[:, None]
    elif pattern == "huge_first":
        k[:32] *= 20.0
    qkv16 = qkv.half()
    want = _attention_fp64(qkv16, B, N, C, H)
    got = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()
    assert torch.isfinite(got).all()
    assert rel_l2(got, want) < 2e-3, pattern
    lib = _lib.load()
    _lib.check(lib.pcd_set_attention_config(6))                  # the same kernel as workgroups of eight waves (512 queries share a K/V ring): same bits
    try:
        got8 = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()
    finally:
        _lib.check(lib.pcd_set_attention_config(5))
    assert torch.equal(got8, got)
    _lib.check(lib.pcd_set_attention_config(1))                  # the generic kernel on the same input
    try:
        gen = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()
    finally:
        _lib.check(lib.pcd_set_attention_config(0))
    assert rel_l2(gen, want) < 2e-3
    assert rel_l2(got, gen) < 2e-3


@pytest.mark.parametrize("pattern", ["plain", "late_spike", "rising", "falling", "huge_first"])
@pytest.mark.parametrize("C,N", [(64, 512), (128, 512), (256, 448), (128, 333)])
def test_attention_max_free_generic_kernel(pattern, C, N):
    """d = 16 / 32 (and d = 64 at lengths the pipelined kernel does not take) run the generic structure with the same max-free
    softmax: the same five score patterns at d = 16, 32, 64 and at a ragged length (masked last tile), against fp64 and against
    the round-1 kernel that tracks the running max per tile."""
    from shapegen_amd import _lib, ops
    B, H = 2, 4
    g = torch.Generator().manual_seed(3 + C + N)
    qkv = torch.randn(B * N, 3 * C, generator=g)
    k = qkv[:, C:2 * C]
    if pattern == "late_spike":
        k[N + N - 40] *= 14.0                    # shape 1, one of the last keys (inside the masked tile when N is ragged)
        k[37] *= 9.0
    elif pattern == "rising":
        k *= torch.linspace(0.2, 6.0, N).repeat(B)[:, None]
    elif pattern == "falling":
        k *= torch.linspace(8.0, 0.1, N).repeat(B)[:, None]
    elif pattern == "huge_first":
        k[:32] *= 20.0
    qkv16 = qkv.half()
    want = _attention_fp64(qkv16, B, N, C, H)
    lib = _lib.load()
    outs = {}
    for mode in (2, 1):                                         # 2: max-free generic kernel, 1: round-1 generic kernel
        _lib.check(lib.pcd_set_attention_config(mode))
        try:
            outs[mode] = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()
        finally:
            _lib.check(lib.pcd_set_attention_config(0))
    assert torch.isfinite(outs[2]).all()
    assert rel_l2(outs[2], want) < 2e-3, (pattern, C, N)
    assert rel_l2(outs[2], outs[1]) < 2e-3
    if N % 256 != 0:                                            # the default dispatch is this kernel for ragged lengths
        assert torch.equal(ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu(), outs[2])


@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 65, 129])
def test_attention_generic_frame_at_its_edges(N, d):
    """The one generic frame (set_attention_generic_kernel: staging, K / V fragment reads, masked last tile, ring loop, epilogue) under both of its
    softmax forms, at the lengths where the frame can go wrong: the first 32-key sub-tile partly masked (N = 1, 31), a whole sub-tile masked (32, 33),
    exactly one full tile (64), one key into the second and third tile (65, 129); Q rows past N are clamped at every one of them.  Against fp64, whole
    tensor and row by row; the default dispatch at these lengths is the max-free form, bit for bit."""
    from shapegen_amd import _lib, ops
    B, H = 2, 4
    C = H * d
    g = torch.Generator().manual_seed(1000 * d + N)
    qkv16 = torch.randn(B * N, 3 * C, generator=g).half()
    want = _attention_fp64(qkv16, B, N, C, H)
    lib = _lib.load()
    outs = {}
    for mode, name in ((2, f"set_attention_om_kernel<{d}>"), (1, f"set_attention_kernel<{d}>")):
        _lib.check(lib.pcd_set_attention_config(mode))
        try:
            outs[mode] = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()
            assert lib.pcd_set_attention_last_kernel().decode() == name
        finally:
            _lib.check(lib.pcd_set_attention_config(0))
        got = outs[mode]
        assert got.shape == want.shape and torch.isfinite(got).all(), (mode, N, d)
        rows = ((got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-3))
        print(f"generic frame, config({mode}), N = {N}, d = {d}: rel-L2 {rel_l2(got, want):.2e}, worst row {float(rows.max()):.2e}")
        assert rel_l2(got, want) < 2e-3, (mode, N, d)
        assert float(rows.max()) < 2e-2, (mode, N, d, int(rows.argmax()))
    default = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()      # N % 256 != 0 at every one of these lengths
    assert lib.pcd_set_attention_last_kernel().decode() == f"set_attention_om_kernel<{d}>"
    assert torch.equal(default, outs[2])


# what pcd_set_attention_last_kernel reports per (config code, d, N): the dispatch ladder of the library before it became one plan, written out
_SP, _ABL = "set_attention_sp_kernel", "set_attention_spn_kernel (timing ablation)"
_DISPATCH = {
    # code: {(d, N): name}
    0: {(16, 256): "set_attention_spn_kernel<16>", (32, 256): "set_attention_spn_kernel<32>", (64, 256): _SP,
        (16, 333): "set_attention_om_kernel<16>", (32, 333): "set_attention_om_kernel<32>", (64, 333): "set_attention_om_kernel<64>"},
    1: {(16, 256): "set_attention_kernel<16>", (32, 256): "set_attention_kernel<32>", (64, 256): "set_attention_kernel<64>",
        (16, 333): "set_attention_kernel<16>", (32, 333): "set_attention_kernel<32>", (64, 333): "set_attention_kernel<64>"},
    2: {(16, 256): "set_attention_om_kernel<16>", (32, 256): "set_attention_om_kernel<32>", (64, 256): "set_attention_om_kernel<64>",
        (16, 333): "set_attention_om_kernel<16>", (32, 333): "set_attention_om_kernel<32>", (64, 333): "set_attention_om_kernel<64>"},
    3: {(16, 256): "set_attention_om_kernel<16>", (32, 256): "set_attention_om_kernel<32>", (64, 256): _SP,                    # d <= 32 off the pipeline
        (16, 333): "set_attention_om_kernel<16>", (32, 333): "set_attention_om_kernel<32>", (64, 333): "set_attention_om_kernel<64>"},
    6: {(16, 256): "set_attention_spn_kernel<16>", (32, 256): "set_attention_spn_kernel<32>", (64, 256): _SP,                  # eight waves need N % 512 == 0: four
        (16, 333): "set_attention_om_kernel<16>", (32, 333): "set_attention_om_kernel<32>", (64, 333): "set_attention_om_kernel<64>"},
}
_RESTORE = {0: 0, 1: 0, 2: 0, 3: 4, 6: 5}


@pytest.mark.parametrize("code", [0, 1, 2, 3, 6])
@pytest.mark.parametrize("d,N", [(16, 256), (32, 256), (64, 256), (16, 333), (32, 333), (64, 333)])
def test_attention_dispatch_table(d, N, code):
    """The plan is the ladder: for every (d, N) on either side of N % 256 == 0 and every pcd_set_attention_config code that selects a kernel (0 default,
    1 round-1 generic, 2 max-free generic, 3 d <= 32 off the pipelined kernel [4 restores], 6 eight-wave workgroups [5 restores]) the name reported
    for the launch is the one written out above, and the launch computes attention."""
    from shapegen_amd import _lib, ops
    B, H = 1, 4
    C = H * d
    qkv16 = torch.randn(B * N, 3 * C, generator=torch.Generator().manual_seed(d + N)).half()
    lib = _lib.load()
    _lib.check(lib.pcd_set_attention_config(code))
    try:
        got = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()
        name = lib.pcd_set_attention_last_kernel().decode()
    finally:
        _lib.check(lib.pcd_set_attention_config(_RESTORE[code]))
    assert name == _DISPATCH[code][(d, N)], (code, d, N)
    assert rel_l2(got, _attention_fp64(qkv16, B, N, C, H)) < 2e-3
    ops.set_attention_f16(qkv16.cuda(), B, N, C, H)                               # and the hook is back at its default
    assert lib.pcd_set_attention_last_kernel().decode() == _DISPATCH[0][(d, N)]


@pytest.mark.parametrize("pattern", ["plain", "late_spike", "rising", "falling", "huge_first"])
@pytest.mark.parametrize("C,N", [(64, 256), (64, 512), (128, 512), (128, 768), (64, 2048)])
def test_attention_pipelined_kernel_d32_d16(pattern, C, N):
    """d = 32 / 16 at N % 256 == 0 run the two-block software pipeline of the d = 64 kernel (set_attention_spn_kernel): one ring group only
    (N = 256), several, the rare path in every position, against fp64 and against the one-block kernel it replaces."""
    from shapegen_amd import _lib, ops
    B, H = 2, 4
    g = torch.Generator().manual_seed(11 + C + N)
    qkv = torch.randn(B * N, 3 * C, generator=g)
    k = qkv[:, C:2 * C]
    if pattern == "late_spike":
        k[N + N - 40] *= 14.0                    # shape 1, one of the last keys
        k[37] *= 9.0                             # shape 0, second sub-tile
        k[N + 64] *= 11.0                        # shape 1, first key of tile 1
    elif pattern == "rising":
        k *= torch.linspace(0.2, 6.0, N).repeat(B)[:, None]
    elif pattern == "falling":
        k *= torch.linspace(8.0, 0.1, N).repeat(B)[:, None]
    elif pattern == "huge_first":
        k[:32] *= 20.0
    qkv16 = qkv.half()
    want = _attention_fp64(qkv16, B, N, C, H)
    lib = _lib.load()
    got = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()
    assert lib.pcd_set_attention_last_kernel().decode() == f"set_attention_spn_kernel<{C // H}>"
    for _ in range(3):                                          # race screen: the ring, its barriers and the in-place score tiles give the same bits every launch
        assert torch.equal(ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu(), got)
    assert torch.isfinite(got).all()
    assert rel_l2(got, want) < 2e-3, (pattern, C, N)
    _lib.check(lib.pcd_set_attention_config(3))                  # the one-block kernel on the same input
    try:
        one = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()
        assert lib.pcd_set_attention_last_kernel().decode() == f"set_attention_om_kernel<{C // H}>"
    finally:
        _lib.check(lib.pcd_set_attention_config(4))
    assert rel_l2(got, one) < 1e-3
    # per-row check: no query row may be off (a wrong row hides in a whole-tensor norm)
    rows = ((got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-3))
    assert float(rows.max()) < 2e-2, (pattern, C, N, int(rows.argmax()))


@pytest.mark.parametrize("C,H", [(256, 8), (128, 8), (512, 16), (1024, 16)])
def test_attention_pipelined_kernels_other_head_counts(C, H):
    """Head widths 32 / 16 / 64 reached with other head counts (row stride 3 C up to 3072 halfs, 8 / 16 heads): the staging offsets and the head slices of the
    pipelined kernels against fp64."""
    from shapegen_amd import _lib, ops
    B, N = 2, 512
    g = torch.Generator().manual_seed(7 + C + H)
    qkv16 = (torch.randn(B * N, 3 * C, generator=g) * 0.9).half()
    want = _attention_fp64(qkv16, B, N, C, H)
    got = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()
    d = C // H
    name = _lib.load().pcd_set_attention_last_kernel().decode()
    assert name == ("set_attention_sp_kernel" if d == 64 else f"set_attention_spn_kernel<{d}>")
    rows = ((got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-3))
    assert torch.isfinite(got).all() and float(rows.max()) < 2e-2 and rel_l2(got, want) < 2e-3


@pytest.mark.parametrize("C", [64, 128, 256])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_attention_pipelined_kernels_block_map(B, C):
    """The pipelined kernels deal (shape, head) pairs to XCDs when batch x heads is a multiple of 8 and fall back to the plain block order otherwise
    (B = 1, 3, 5 with 4 heads: 4, 12, 20 pairs): every query block of every pair is computed exactly once either way."""
    from shapegen_amd import ops
    N, H = 768, 4
    g = torch.Generator().manual_seed(100 + B + C)
    qkv16 = (torch.randn(B * N, 3 * C, generator=g) * 0.8).half()
    want = _attention_fp64(qkv16, B, N, C, H)
    got = ops.set_attention_f16(qkv16.cuda(), B, N, C, H).float().cpu()
    rows = ((got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-3))
    assert torch.isfinite(got).all() and float(rows.max()) < 2e-2, (B, C, int(rows.argmax()))
    assert rel_l2(got, want) < 2e-3


@pytest.mark.parametrize("rows,c", [(4096 + 5, 64), (1000, 128), (777, 256), (64, 96), (3, 256)])
def test_layernorm_rows(rows, c):
    """nn.LayerNorm over the channel axis (reference networks.py:66-67, eps 1e-5, biased variance) on fp16 rows: the vectorised
    kernel for C = 64 / 128 / 256 (several rows per wave, ragged row counts) and the generic one (C = 96) against fp64."""
    from shapegen_amd import ops
    g = torch.Generator().manual_seed(rows + c)
    x = (torch.randn(rows, c, generator=g) * 2 + 0.5).half()
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    want = torch.nn.functional.layer_norm(x.double(), (c,), gamma.double(), beta.double(), 1e-5)
    got = ops.layernorm_f16(x.cuda(), gamma.cuda(), beta.cuda()).cpu()
    assert got.shape == x.shape and got.dtype == torch.float16
    assert float((got.double() - want).abs().max()) <= 2e-3 * max(1.0, float(want.abs().max()))      # one fp16 rounding


@pytest.mark.parametrize("c", [64, 128, 256])
@pytest.mark.parametrize("which", ["one_row", "block_plus_one"])
def test_layernorm_forward_forms_bitwise_at_launch_edges(which, c):
    """pcd_layernorm_f16 and pcd_layernorm_train_f16 are one row kernel behind one launcher (2048 / c rows per block): a single row (every other
    row group of the block clamped) and one full block plus one row (a second block with one live row), the two forms bit for bit, against fp64,
    and nothing written past the last row."""
    from shapegen_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr()
    rows = 1 if which == "one_row" else 2048 // c + 1
    g = torch.Generator().manual_seed(7 * c + rows)
    x = (torch.randn(rows, c, generator=g) * 2 + 0.5).half()
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    want = torch.nn.functional.layer_norm(x.double(), (c,), gamma.double(), beta.double(), 1e-5)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    guard = 8                                                    # rows behind the last one that must stay as they are
    y0 = torch.full((rows + guard, c), float("nan"), dtype=torch.float16, device="cuda")
    y1 = torch.full_like(y0, float("nan"))
    mu, rs = torch.full((rows + guard,), float("nan"), device="cuda"), torch.full((rows + guard,), float("nan"), device="cuda")
    _lib.check(lib.pcd_layernorm_f16(xd.data_ptr(), rows, c, gd.data_ptr(), bd.data_ptr(), y0.data_ptr(), st), "ln")
    _lib.check(lib.pcd_layernorm_train_f16(xd.data_ptr(), rows, c, gd.data_ptr(), bd.data_ptr(), y1.data_ptr(), mu.data_ptr(), rs.data_ptr(), st), "ln_train")
    torch.cuda.synchronize()
    y0, y1, mu, rs = y0.cpu(), y1.cpu(), mu.cpu(), rs.cpu()
    assert torch.isnan(y0[rows:]).all() and torch.isnan(y1[rows:]).all() and torch.isnan(mu[rows:]).all() and torch.isnan(rs[rows:]).all()
    assert torch.isfinite(y0[:rows]).all() and torch.equal(y0[:rows], y1[:rows])
    assert float((y0[:rows].double() - want).abs().max()) <= 2e-3 * max(1.0, float(want.abs().max()))      # one fp16 rounding, as test_layernorm_rows
    m64 = x.double().mean(dim=1)
    r64 = (x.double().var(dim=1, unbiased=False) + 1e-5).rsqrt()
    assert float((mu[:rows].double() - m64).abs().max()) <= 1e-6 * float(x.double().abs().max())          # the bounds of test_gpu_layernorm_rows.py
    assert float((rs[:rows].double() / r64 - 1).abs().max()) <= 1e-6


def test_unet_attention_golden(golden):
    from shapegen_amd.networks import UNetAttentionPointExperimental
    g = golden("attention.npz")
    net = UNetAttentionPointExperimental(128)
    net.load_state_dict(una_sd(), strict=True)
    net = net.to("cuda").eval()
    eps = net(torch.from_numpy(g["una_x"]).cuda(), torch.from_numpy(g["una_t"]).cuda()).cpu()
    assert rel_l2(eps, g["una_eps"]) < 5e-3   # 7 attention blocks + 15 GEMMs deep in fp16: measured 2.2e-3 (tools/measure_bounds.py)


@pytest.mark.parametrize("N", [128, 2048])
def test_unet_attention_skip_taps(N):
    """Where the error enters: the three skip tensors of the attention U-Net (x1 = att1 + emb2, x2 = att2 + emb3, x3 = att3,
    reference networks.py:663-672) against the oracle's, at the golden length and at the BASELINE length -- each within 2e-3
    (measured 6e-4 / 8e-4 / 1e-3), so no block hides behind the 5e-3 of the whole network."""
    from shapegen_amd.networks import UNetAttentionPointExperimental
    from oracle import torch_oracle as O
    sd = una_sd()
    net = UNetAttentionPointExperimental(N)
    net.load_state_dict(sd, strict=True)
    net = net.to("cuda").eval()
    gen = torch.Generator().manual_seed(9 + N)
    x, t = torch.randn(2, N, 3, generator=gen) * 1.2, torch.rand(2, generator=gen)
    eps = net(x.cuda(), t.cuda()).cpu()
    taps = {}
    want = O.unet_attention(sd, "", x, t, taps=taps)
    for name in ("x1", "x2", "x3"):
        assert rel_l2(net.tap(name, 2, N).float().cpu(), taps[name]) < 2e-3, name
    assert rel_l2(eps, want) < 5e-3


def test_attention_backbone_under_the_samplers():
    """the attention U-Net as an alternative backbone selectable at construction, driven by the same
    sampler loops (device-side step select of its 704-float time-bias rows, HIP-graph replay).  DDIM `sample` (T = 12,
    graph path) and DDPM `sample2` (injected noise) against the oracle; state_dict keys = `model.*` of the class."""
    from oracle import torch_oracle as O
    from shapegen_amd import specs
    from shapegen_amd.diffusion import PointCloudDiffusion
    sd = {"model." + k: v for k, v in una_sd().items()}
    m = PointCloudDiffusion(num_points=128, backbone="attention")
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, s) for k, s, _ in specs.unet_attention_spec(prefix="model.")]
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    model = lambda x, t: O.unet_attention(sd, "model.", x, t)
    g = torch.Generator().manual_seed(4)
    xT = torch.randn(2, 128, 3, generator=g)
    want = O.ddim_sample(model, xT, 12)
    got = m.sample(2, 128, num_steps=12, x_T=xT.cuda())
    r12 = rel_l2(got.cpu(), want)
    zs = torch.randn(5, 2, 128, 3, generator=g)
    want = O.ddpm_sample(model, xT, 6, list(zs))
    got = m.sample2(2, 128, num_steps=6, x_T=xT.cuda(), noises=zs.cuda())
    r6 = rel_l2(got.cpu(), want)
    # a longer horizon through replayed graphs: 100 DDIM steps (the horizon of BASELINE configs[0]) against the oracle
    want = O.ddim_sample(model, xT, 100)
    got = m.sample(2, 128, num_steps=100, x_T=xT.cuda())
    r100 = rel_l2(got.cpu(), want)
    print(f"attention backbone vs oracle: DDIM T=12 {r12:.2e}, DDPM T=6 {r6:.2e}, DDIM T=100 {r100:.2e}")
    assert r12 < 5e-3 and r6 < 5e-3 and r100 < 5e-3            # the point path's sampler bound (measured 8.0e-4 / 6.2e-4 / 5.5e-4)
    with pytest.raises(ValueError):
        PointCloudDiffusion(num_points=128, backbone="transformer")


def test_sab_c_entry_rejects_bad_arguments():
    from shapegen_amd import _lib
    import ctypes as C
    lib = _lib.load()
    d = _lib.SabDesc()
    d.dim = 96
    x = torch.zeros(256, 96, dtype=torch.float16, device="cuda")
    assert lib.pcd_sab_forward(C.byref(d), x.data_ptr(), 1, 256, 4, x.data_ptr(), x.data_ptr(), 1 << 20, 0) != 0
    assert b"bad argument" in lib.pcd_last_error()


def test_full_size_attention_next_to_the_oracle():
    """The launches bench.py times (B = 64, N = 2048: `set_attention_sp_kernel` at C = 256 with its XCD-aware block map over
    64 shapes x 4 heads, the whole attention U-Net at full grid) checked against the ORACLE, not against a smaller launch of
    themselves: shapes are independent, so rows of the full batch must equal the oracle on those shapes."""
    from shapegen_amd.networks import SetAttentionBlock, UNetAttentionPointExperimental
    from oracle import torch_oracle as O
    gen = torch.Generator().manual_seed(6464)
    sd = sab_sd(256)
    blk = SetAttentionBlock(256, 4)
    blk.load_state_dict(sd, strict=True)
    blk = blk.to("cuda").eval()
    x = torch.randn(64, 2048, 256, generator=gen) * 1.5
    out = blk(x.cuda()).cpu()
    for rows in ((9, 10), (63, 64)):                       # one shape from the middle, the last one (last XCD group)
        want = O.set_attention_block(sd, "", x[rows[0]:rows[1]], 4)
        assert rel_l2(out[rows[0]:rows[1]], want) < 3e-3, rows
    del blk, out, x
    usd = una_sd()
    net = UNetAttentionPointExperimental(2048)
    net.load_state_dict(usd, strict=True)
    net = net.to("cuda").eval()
    xp, t = torch.randn(64, 2048, 3, generator=gen) * 1.2, torch.rand(64, generator=gen)
    eps = net(xp.cuda(), t.cuda()).cpu()
    for rows in ((20, 21), (63, 64)):
        want = O.unet_attention(usd, "", xp[rows[0]:rows[1]], t[rows[0]:rows[1]])
        assert rel_l2(eps[rows[0]:rows[1]], want) < 5e-3, rows


def test_attention_at_2048_points_against_the_reference(golden):
    """G24: `SetAttentionBlock(256, 4)` on (1, 2048, 256) and `UNetAttentionPointExperimental` on (2, 2048, 3) captured from the REFERENCE at BASELINE's
    point count (the other goldens of this file are at N = 128; N = 2048 was oracle-only): inputs rebuilt from the integer hash."""
    import numpy as np
    from shapegen_amd import specs
    from shapegen_amd.networks import SetAttentionBlock, UNetAttentionPointExperimental
    g = golden("attention_n2048.npz")
    blk = SetAttentionBlock(256, 4)
    blk.load_state_dict(sab_sd(256), strict=True)
    blk = blk.to("cuda").eval()
    xa = torch.from_numpy(specs.hash_uniform("xa2048", 2048 * 256, 0).reshape(1, 2048, 256).astype(np.float32)) * 2
    out = blk(xa.cuda()).cpu()
    assert rel_l2(out[0, ::8], g["sab256_out_rows"].astype(np.float32)) < 3e-3
    net = UNetAttentionPointExperimental(2048)
    net.load_state_dict(una_sd(), strict=True)
    net = net.to("cuda").eval()
    xu = torch.from_numpy(specs.hash_uniform("xu2048", 2 * 2048 * 3, 0).reshape(2, 2048, 3).astype(np.float32)) * 1.5
    eps = net(xu.cuda(), torch.from_numpy(g["una_t"]).cuda()).cpu()
    r = rel_l2(eps, g["una_eps"])
    print(f"attention U-Net at (2, 2048) vs the reference: rel-L2 {r:.2e}")
    assert r < 5e-3


def _tail_fp64(a, x, sd):
    """x1 = x + out_proj(a); y = x1 + ff.2(relu(ff.0(LN2(x1)))) in float64 from the fp16-rounded operands (reference networks.py:78-83)."""
    f = lambda k: sd[k].double()
    h = lambda k: sd[k].half().double()
    x1 = x + a @ h("attention.out_proj.weight").T + f("attention.out_proj.bias")
    ln = torch.nn.functional.layer_norm(x1, (x1.shape[1],), f("ln2.weight"), f("ln2.bias"), 1e-5)
    hid = torch.relu(ln.half().double() @ h("ff.0.weight").T + f("ff.0.bias"))
    return x1 + hid.half().double() @ h("ff.2.weight").T + f("ff.2.bias")


@pytest.mark.parametrize("C,rows", [(64, 256), (128, 256), (64, 256 * 7), (128, 256 * 300)])
def test_sab_tail_one_launch_against_fp64(C, rows):
    """pcd_sab_tail_f16 (out_proj + residual + LN2 + FFN + residual in one launch, activations in registers) against the same arithmetic in
    float64: one tile of points, several tiles per workgroup (300 tiles on 256 workgroups: the ring runs across tile boundaries)."""
    import ctypes as C_
    from shapegen_amd import _lib
    from shapegen_amd.networks import _PackedSAB
    lib = _lib.load()
    sd = sab_sd(C)
    g = torch.Generator().manual_seed(C + rows)
    a = (torch.randn(rows, C, generator=g) * 0.7).half()
    x = (torch.randn(rows, C, generator=g) * 1.5).half()
    pk = _PackedSAB(sd, "", C, torch.device("cuda"))
    desc = pk.fill(_lib.SabDesc())
    assert desc.tail_packed and lib.pcd_sab_tail_supported(C, rows) == 1 and lib.pcd_sab_tail_supported(C, rows + 64) == 0
    ad, xd = a.cuda(), x.cuda()
    y = torch.full((rows, C), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.pcd_sab_tail_f16(C, desc.tail_packed, ad.data_ptr(), xd.data_ptr(), rows, y.data_ptr(), _lib.stream_ptr()))
    pick = slice(0, rows) if rows <= 4096 else torch.cat([torch.arange(0, 512), torch.arange(rows // 2 - 256, rows // 2 + 256), torch.arange(rows - 512, rows)])
    want = _tail_fp64(a.double()[pick], x.double()[pick], sd)
    got = y.cpu().double()
    assert torch.isfinite(got).all()
    assert rel_l2(got[pick], want) < 1e-3
    # bitwise repeatable (no atomics, fixed summation order; a ring race would show here)
    y2 = torch.empty_like(y)
    for _ in range(5):
        _lib.check(lib.pcd_sab_tail_f16(C, desc.tail_packed, ad.data_ptr(), xd.data_ptr(), rows, y2.data_ptr(), _lib.stream_ptr()))
        assert torch.equal(y, y2)
    # argument checks of the C entry
    assert lib.pcd_sab_tail_f16(C, desc.tail_packed, ad.data_ptr(), xd.data_ptr(), rows + 1, y.data_ptr(), _lib.stream_ptr()) != 0
    assert lib.pcd_sab_tail_f16(256, desc.tail_packed, ad.data_ptr(), xd.data_ptr(), rows, y.data_ptr(), _lib.stream_ptr()) != 0
    assert lib.pcd_sab_tail_f16(C, desc.tail_packed, ad.data_ptr(), xd.data_ptr(), rows, xd.data_ptr(), _lib.stream_ptr()) != 0
    assert lib.pcd_sab_tail_packed_bytes(256) == 0


@pytest.mark.parametrize("C", [64, 128])
def test_set_attention_block_tail_fused_against_the_four_launches(C):
    """The block with its tail as one launch (default where rows % 256 == 0) against the four launches it replaces (pcd_sab_tail_config(0)) and the oracle."""
    from shapegen_amd import _lib
    from shapegen_amd.networks import SetAttentionBlock
    from oracle import torch_oracle as O
    lib = _lib.load()
    sd = sab_sd(C)
    blk = SetAttentionBlock(C, 4)
    blk.load_state_dict(sd, strict=True)
    blk = blk.to("cuda").eval()
    x = torch.randn(2, 1024, C, generator=torch.Generator().manual_seed(3 * C)) * 1.5
    assert lib.pcd_sab_tail_enabled() == 1
    fused = blk(x.cuda()).cpu()
    _lib.check(lib.pcd_sab_tail_config(0))
    try:
        four = blk(x.cuda()).cpu()
    finally:
        _lib.check(lib.pcd_sab_tail_config(1))
    want = O.set_attention_block(sd, "", x, 4)
    assert not torch.equal(fused, four)                       # (x1 and LN2(x1) stay fp32 in the one-launch form: the two are not the same bits)
    assert rel_l2(fused, four) < 1.5e-3
    assert rel_l2(fused, want) < 3e-3 and rel_l2(four, want) < 3e-3
    assert rel_l2(fused, want) <= rel_l2(four, want) * 1.05  # and the one-launch form is not the less accurate one


@pytest.mark.parametrize("passes,relu,rows", [(3, 0, 256), (4, 1, 256), (3, 0, 256 * 300), (1, 1, 512)])
def test_wide_chain_layernorm_linear_against_fp64(passes, relu, rows):
    """pcd_pw_wide_ln_linear: LayerNorm(256) + Linear(256, 256 passes) [+ ReLU] in one launch (B fragments normalised as they are loaded) against float64
    from the fp16-rounded operands; the LayerNorm result is rounded to fp16 in both, as pcd_layernorm_f16 does."""
    from shapegen_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(11 * passes + rows)
    x = (torch.randn(rows, 256, generator=g) * 1.7 + 0.4).half()
    w = (torch.randn(256 * passes, 256, generator=g) / 16).half()
    b = torch.randn(256 * passes, generator=g) * 0.1
    ga, be = 1 + 0.2 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    dev = lambda t: t.cuda().contiguous()
    xd, wd, bd, gd, bed = dev(x), dev(w), dev(b), dev(ga), dev(be)
    packed = torch.empty(lib.pcd_pw_wide_ln_linear_packed_bytes(passes), dtype=torch.uint8, device="cuda")
    _lib.check(lib.pcd_pw_wide_ln_linear_pack(wd.data_ptr(), bd.data_ptr(), passes, gd.data_ptr(), bed.data_ptr(), packed.data_ptr(), _lib.stream_ptr()))
    out = torch.full((rows, 256 * passes), float("nan"), dtype=torch.float16, device="cuda")
    assert lib.pcd_pw_wide_ln_linear_supported(256, rows) == 1 and lib.pcd_pw_wide_ln_linear_supported(128, rows) == 0
    _lib.check(lib.pcd_pw_wide_ln_linear(packed.data_ptr(), passes, relu, xd.data_ptr(), rows, out.data_ptr(), _lib.stream_ptr()))
    pick = torch.arange(rows) if rows <= 4096 else torch.cat([torch.arange(0, 512), torch.arange(rows // 2 - 256, rows // 2 + 256), torch.arange(rows - 512, rows)])
    ln = torch.nn.functional.layer_norm(x.double()[pick], (256,), ga.double(), be.double(), 1e-5).half().double()
    want = ln @ w.double().T + b.double()
    want = torch.relu(want) if relu else want
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    assert rel_l2(got[pick], want) < 1e-3
    if not relu:
        assert float(got.min()) < 0                             # a plain Linear keeps its negative outputs
    out2 = torch.empty_like(out)
    for _ in range(3):
        _lib.check(lib.pcd_pw_wide_ln_linear(packed.data_ptr(), passes, relu, xd.data_ptr(), rows, out2.data_ptr(), _lib.stream_ptr()))
        assert torch.equal(out, out2)
    assert lib.pcd_pw_wide_ln_linear(packed.data_ptr(), passes, relu, xd.data_ptr(), rows + 8, out.data_ptr(), _lib.stream_ptr()) != 0
    assert lib.pcd_pw_wide_ln_linear(packed.data_ptr(), 5, relu, xd.data_ptr(), rows, out.data_ptr(), _lib.stream_ptr()) != 0


@pytest.mark.parametrize("C", [64, 128, 256])
def test_fused_layernorm_rows_with_a_large_mean(C):
    """rows with |mean| >> std (x = 50 + 0.1 randn, as post-ReLU activations near the fp16 range are): a one-pass variance
    sum(x^2) - C mean^2 cancels in fp32 and rstd is badly wrong.  The fused LayerNorm + Linear launches (C = 256: pcd_pw_wide_ln_linear; C <= 128:
    pcd_sab_head_f16) compute the variance about the mean; against float64 from the fp16-rounded operands, with pcd_layernorm_f16 beside it."""
    from shapegen_amd import _lib, ops
    from shapegen_amd.networks import _PackedSAB
    lib = _lib.load()
    rows = 512
    g = torch.Generator().manual_seed(1000 + C)
    x = (50.0 + 0.1 * torch.randn(rows, C, generator=g)).half()
    x[7] = (-300.0 + 0.5 * torch.randn(C, generator=g)).half()
    x[8] = (0.02 * torch.randn(C, generator=g)).half()
    sd = sab_sd(C)
    w, b = sd["attention.in_proj_weight"].half(), sd["attention.in_proj_bias"]
    ga, be = sd["ln1.weight"], sd["ln1.bias"]
    xd = x.cuda()
    if C == 256:
        w, b = w[:256].contiguous(), b[:256].contiguous()
        dev = lambda t: t.cuda().contiguous()
        wd, bd, gd, bed = dev(w), dev(b), dev(ga), dev(be)
        out = torch.full((rows, 256), float("nan"), dtype=torch.float16, device="cuda")
        packed = torch.empty(lib.pcd_pw_wide_ln_linear_packed_bytes(1), dtype=torch.uint8, device="cuda")
        _lib.check(lib.pcd_pw_wide_ln_linear_pack(wd.data_ptr(), bd.data_ptr(), 1, gd.data_ptr(), bed.data_ptr(), packed.data_ptr(), _lib.stream_ptr()))
        _lib.check(lib.pcd_pw_wide_ln_linear(packed.data_ptr(), 1, 0, xd.data_ptr(), rows, out.data_ptr(), _lib.stream_ptr()))
    else:
        pk = _PackedSAB(sd, "", C, torch.device("cuda"))
        desc = pk.fill(_lib.SabDesc())
        out = torch.full((rows, 3 * C), float("nan"), dtype=torch.float16, device="cuda")
        _lib.check(lib.pcd_sab_head_f16(C, desc.tail_packed, xd.data_ptr(), rows, out.data_ptr(), _lib.stream_ptr()))
    ln = torch.nn.functional.layer_norm(x.double(), (C,), ga.double(), be.double(), 1e-5)
    want = ln.half().double() @ w.double().T + b.double()
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    err = rel_l2(got, want)
    err_ln = rel_l2(ops.layernorm_f16(xd, ga.cuda(), be.cuda()).cpu().double(), ln)          # the unfused kernel on the same rows
    print(f"C = {C}: fused LayerNorm + Linear on large-mean rows rel-L2 {err:.2e} (pcd_layernorm_f16 alone {err_ln:.2e})")
    assert err < 2e-3 and err_ln < 2e-3
    # the two special rows on their own: inside the bound over 512 rows a row that is 3 % wrong adds 1.3e-3 and passes
    for r in (7, 8):
        row = float((got[r] - want[r]).norm() / want[r].norm())
        assert row <= 1e-3, (C, r, row)


@pytest.mark.parametrize("rows", [128, 128 * 7, 128 * 600])
def test_wide_ffn_one_launch_against_fp64(rows):
    """pcd_wide_ffn_f16 (round 5, csrc/wideffn.hip): y = x1 + W2 relu(W1 LN2(x1) + b1) + b2 at C = 256 as ONE launch -- wave pairs share 32 points and split the
    channels of both products, the 1024-wide hidden row exists 128 channels at a time in registers / LDS -- against float64 from the fp16-rounded operands with the
    kernel's own rounding points (LayerNorm result, hidden activations and the FFN output rounded to fp16, then the fp16 residual add).  One to five tiles per
    workgroup (600 tiles on 256 workgroups: uneven), bitwise repeatable, arguments checked."""
    from shapegen_amd import _lib
    lib = _lib.load()
    sd = sab_sd(256)
    g = torch.Generator().manual_seed(31 + rows)
    x = (torch.randn(rows, 256, generator=g) * 1.4 + 0.2).half()
    x[3] = (40.0 + 0.2 * torch.randn(256, generator=g)).half()                 # a row with |mean| >> std (two-pass variance)
    w1, b1 = sd["ff.0.weight"].half(), sd["ff.0.bias"].float()
    w2, b2 = sd["ff.2.weight"].half(), sd["ff.2.bias"].float()
    ga, be = sd["ln2.weight"].float(), sd["ln2.bias"].float()
    dev = lambda t: t.cuda().contiguous()
    xd, w1d, b1d, w2d, b2d, gd, bd = dev(x), dev(w1), dev(b1), dev(w2), dev(b2), dev(ga), dev(be)
    assert lib.pcd_wide_ffn_supported(256, rows) == 1 and lib.pcd_wide_ffn_supported(128, rows) == 0 and lib.pcd_wide_ffn_supported(256, rows + 64) == 0
    packed = torch.empty(lib.pcd_wide_ffn_packed_bytes(), dtype=torch.uint8, device="cuda")
    _lib.check(lib.pcd_wide_ffn_pack(w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), gd.data_ptr(), bd.data_ptr(), packed.data_ptr(), _lib.stream_ptr()))
    y = torch.full((rows, 256), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.pcd_wide_ffn_f16(packed.data_ptr(), xd.data_ptr(), rows, y.data_ptr(), _lib.stream_ptr()), "wide_ffn")
    pick = torch.arange(rows) if rows <= 4096 else torch.cat([torch.arange(0, 512), torch.arange(rows // 2 - 256, rows // 2 + 256), torch.arange(rows - 512, rows)])
    xp = x[pick].double()
    ln = torch.nn.functional.layer_norm(xp, (256,), ga.double(), be.double(), 1e-5).half().double()
    hid = torch.relu(ln @ w1.double().T + b1.double()).half().double()
    want = ((hid @ w2.double().T + b2.double()).half().double() + xp).half().double()
    got = y.cpu().double()
    assert torch.isfinite(got).all()
    err = rel_l2(got[pick] - xp, want - xp)                                     # on the FFN's own contribution, not on x1 + it
    print(f"wide FFN, {rows} rows: rel-L2 of the FFN term {err:.2e}, of y {rel_l2(got[pick], want):.2e}")
    assert err < 2e-3 and rel_l2(got[pick], want) < 1e-3
    y2 = torch.empty_like(y)
    for _ in range(3):
        _lib.check(lib.pcd_wide_ffn_f16(packed.data_ptr(), xd.data_ptr(), rows, y2.data_ptr(), _lib.stream_ptr()))
        assert torch.equal(y, y2)
    assert lib.pcd_wide_ffn_f16(packed.data_ptr(), xd.data_ptr(), rows + 8, y.data_ptr(), _lib.stream_ptr()) != 0
    assert lib.pcd_wide_ffn_f16(None, xd.data_ptr(), rows, y.data_ptr(), _lib.stream_ptr()) != 0
    # the per-shape rows behind the block (networks.py:688) on the way out of the same launch: bitwise the FFN launch + pcd_add_shape_bias_strided_f16
    rps = 128 if rows > 128 else 64
    shapes = rows // rps
    for estride in (704, 0):
        e = (torch.randn(max(1, shapes if estride else 1), 704, generator=g) * 0.7).float().cuda()
        ev = e[:, 256:]                                                          # an offset view, as the time-bias table hands it over (16-byte aligned)
        eptr = e.data_ptr() + 256 * 4
        two = torch.empty_like(y)
        _lib.check(lib.pcd_add_shape_bias_strided_f16(y.data_ptr(), rows, 256, rps, eptr, estride, two.data_ptr(), _lib.stream_ptr()))
        one = torch.full_like(y, float("nan"))
        _lib.check(lib.pcd_wide_ffn_bias_f16(packed.data_ptr(), xd.data_ptr(), rows, rps, eptr, estride, one.data_ptr(), _lib.stream_ptr()), "wide_ffn_bias")
        assert torch.equal(one, two), estride
        assert not torch.equal(one, y) and ev.shape[1] == 448
    assert lib.pcd_wide_ffn_bias_f16(packed.data_ptr(), xd.data_ptr(), rows, 0, eptr, 704, y2.data_ptr(), _lib.stream_ptr()) != 0        # rows per shape
    assert lib.pcd_wide_ffn_bias_f16(packed.data_ptr(), xd.data_ptr(), rows, rps, eptr + 4, 704, y2.data_ptr(), _lib.stream_ptr()) != 0   # alignment


def test_set_attention_block_256_layernorm_in_the_linear_launches():
    """C = 256: LN1 + in_proj and LN2 + ff.0 as one launch each (default where rows % 256 == 0) against the separate launches and the oracle."""
    from shapegen_amd import _lib
    from shapegen_amd.networks import SetAttentionBlock
    from oracle import torch_oracle as O
    lib = _lib.load()
    sd = sab_sd(256)
    blk = SetAttentionBlock(256, 4)
    blk.load_state_dict(sd, strict=True)
    blk = blk.to("cuda").eval()
    x = torch.randn(2, 1024, 256, generator=torch.Generator().manual_seed(77)) * 1.5
    fused = blk(x.cuda()).cpu()
    _lib.check(lib.pcd_sab_tail_config(0))
    try:
        sep = blk(x.cuda()).cpu()
    finally:
        _lib.check(lib.pcd_sab_tail_config(1))
    want = O.set_attention_block(sd, "", x, 4)
    assert rel_l2(fused, sep) < 1e-3
    assert rel_l2(fused, want) < 3e-3 and rel_l2(sep, want) < 3e-3


@pytest.mark.parametrize("C,rows", [(64, 256), (128, 256), (64, 256 * 300), (128, 256 * 7)])
def test_sab_head_one_launch_against_fp64(C, rows):
    """pcd_sab_head_f16: qkv = in_proj(LN1(x)) in one launch (B fragments normalised as they are loaded, three C-wide output passes) against float64 from the
    fp16-rounded operands, the LayerNorm result rounded to fp16 in both."""
    from shapegen_amd import _lib
    from shapegen_amd.networks import _PackedSAB
    lib = _lib.load()
    sd = sab_sd(C)
    g = torch.Generator().manual_seed(5 * C + rows)
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.3).half()
    pk = _PackedSAB(sd, "", C, torch.device("cuda"))
    desc = pk.fill(_lib.SabDesc())
    xd = x.cuda()
    qkv = torch.full((rows, 3 * C), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.pcd_sab_head_f16(C, desc.tail_packed, xd.data_ptr(), rows, qkv.data_ptr(), _lib.stream_ptr()))
    pick = torch.arange(rows) if rows <= 4096 else torch.cat([torch.arange(0, 512), torch.arange(rows // 2 - 256, rows // 2 + 256), torch.arange(rows - 512, rows)])
    ln = torch.nn.functional.layer_norm(x.double()[pick], (C,), sd["ln1.weight"].double(), sd["ln1.bias"].double(), 1e-5).half().double()
    want = ln @ sd["attention.in_proj_weight"].half().double().T + sd["attention.in_proj_bias"].double()
    got = qkv.cpu().double()
    assert torch.isfinite(got).all()
    assert rel_l2(got[pick], want) < 1e-3
    q2 = torch.empty_like(qkv)
    for _ in range(3):
        _lib.check(lib.pcd_sab_head_f16(C, desc.tail_packed, xd.data_ptr(), rows, q2.data_ptr(), _lib.stream_ptr()))
        assert torch.equal(qkv, q2)
    assert lib.pcd_sab_head_f16(C, desc.tail_packed, xd.data_ptr(), rows + 1, qkv.data_ptr(), _lib.stream_ptr()) != 0
    assert lib.pcd_sab_head_f16(C, desc.tail_packed, xd.data_ptr(), rows, xd.data_ptr(), _lib.stream_ptr()) != 0


@pytest.mark.parametrize("C,shared", [(64, False), (128, False), (128, True)])
def test_sab_head_tail_with_folded_time_embeddings_bitwise(C, shared):
    """The per-level time embeddings inside the head / tail launches (x read as fp16(x + pre_e[shape]), y leaving as fp16(y + post_e[shape])) give the
    BITS of the explicit pcd_add_shape_bias_strided_f16 launches around the plain head / tail: rows of e 704 floats apart (the attention U-Net's time-bias
    rows) or one shared row."""
    from shapegen_amd import _lib
    from shapegen_amd.networks import _PackedSAB
    lib = _lib.load()
    rows, rps = 256 * 6, 512
    sd = sab_sd(C)
    g = torch.Generator().manual_seed(9 * C + shared)
    a = (torch.randn(rows, C, generator=g) * 0.7).half().cuda()
    x = (torch.randn(rows, C, generator=g) * 1.5).half().cuda()
    nshape, stride = rows // rps, 0 if shared else 704
    e = (torch.randn(max(nshape * stride, 704) + 704, generator=g) * 0.5).cuda()
    pre, post = e[64:], e[128:]                                  # 256-byte aligned views into one buffer, like the U-Net's tbias offsets
    pk = _PackedSAB(sd, "", C, torch.device("cuda"))
    desc = pk.fill(_lib.SabDesc())
    st = _lib.stream_ptr()
    rps_arg = rows if shared else rps
    # explicit: xe = x + pre; y = tail(a, xe); ye = y + post; qkv = head(xe)
    xe, y, ye = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    qkv, qkv_f = torch.empty(rows, 3 * C, dtype=torch.float16, device="cuda"), torch.empty(rows, 3 * C, dtype=torch.float16, device="cuda")
    _lib.check(lib.pcd_add_shape_bias_strided_f16(x.data_ptr(), rows, C, rps_arg, pre.data_ptr(), stride, xe.data_ptr(), st))
    _lib.check(lib.pcd_sab_tail_f16(C, desc.tail_packed, a.data_ptr(), xe.data_ptr(), rows, y.data_ptr(), st))
    _lib.check(lib.pcd_add_shape_bias_strided_f16(y.data_ptr(), rows, C, rps_arg, post.data_ptr(), stride, ye.data_ptr(), st))
    _lib.check(lib.pcd_sab_head_f16(C, desc.tail_packed, xe.data_ptr(), rows, qkv.data_ptr(), st))
    # folded
    yf = torch.empty_like(x)
    _lib.check(lib.pcd_sab_tail_bias_f16(C, desc.tail_packed, a.data_ptr(), x.data_ptr(), rows, rps_arg, pre.data_ptr(), post.data_ptr(), stride, yf.data_ptr(), st))
    _lib.check(lib.pcd_sab_head_bias_f16(C, desc.tail_packed, x.data_ptr(), rows, rps_arg, pre.data_ptr(), stride, qkv_f.data_ptr(), st))
    assert not torch.equal(xe, x) and not torch.equal(ye, y)
    assert torch.equal(yf, ye)
    assert torch.equal(qkv_f, qkv)
    # one of the two only
    y1 = torch.empty_like(x)
    _lib.check(lib.pcd_sab_tail_bias_f16(C, desc.tail_packed, a.data_ptr(), x.data_ptr(), rows, rps_arg, pre.data_ptr(), None, stride, y1.data_ptr(), st))
    assert torch.equal(y1, y)
    # misaligned / bad stride is refused
    assert lib.pcd_sab_tail_bias_f16(C, desc.tail_packed, a.data_ptr(), x.data_ptr(), rows, rps_arg, e[1:].data_ptr(), None, stride, y1.data_ptr(), st) != 0
    assert lib.pcd_sab_head_bias_f16(C, desc.tail_packed, x.data_ptr(), rows, rps_arg, pre.data_ptr(), 702, qkv_f.data_ptr(), st) != 0


def _ring_kernel(kernel):
    """(config entry, default, other, rows per tile, grid cap, inputs(rows), run(inputs) -> output) of one kernel that streams its weights through the
    three-slot LDS-DMA ring; the cap is the launch code's (csrc/widechain.hip, wideffn.hip, sab_tail.hip)."""
    import ctypes as C_
    from shapegen_amd import _lib
    from shapegen_amd.networks import _PackedSAB
    lib = _lib.load()
    st = _lib.stream_ptr()
    g = torch.Generator().manual_seed(sum(map(ord, kernel)))
    dev = lambda t: t.cuda().contiguous()
    rnd = lambda rows, c, scale=1.0, shift=0.0: dev((torch.randn(rows, c, generator=g) * scale + shift).half())
    nan = lambda rows, c: torch.full((rows, c), float("nan"), dtype=torch.float16, device="cuda")
    if kernel in ("chain0", "chain1"):
        chain = int(kernel[-1])
        shapes = [(256, 256), (256, 256), (512, 256)] if chain == 0 else [(256, 512), (256, 256), (128, 256)]
        ws = [dev((torch.randn(s, generator=g) / s[1] ** 0.5).half()) for s in shapes]
        bs = [dev(torch.randn(s[0], generator=g) * 0.1) for s in shapes]
        packed = torch.empty(int(lib.pcd_pw_wide_packed_bytes(chain)), dtype=torch.uint8, device="cuda")
        wp = (C_.c_void_p * 3)(*[t.data_ptr() for t in ws])
        bp = (C_.c_void_p * 3)(*[t.data_ptr() for t in bs])
        _lib.check(lib.pcd_pw_wide_pack(chain, wp, bp, packed.data_ptr(), st))

        def run(xs):
            out = nan(xs[0].shape[0], shapes[2][0])
            _lib.check(lib.pcd_pw_wide_chain(chain, xs[0].data_ptr(), xs[1].data_ptr() if chain else 0, xs[0].shape[0], packed.data_ptr(), out.data_ptr(), st))
            return out
        return lib.pcd_pw_wide_config, 1, 0, 256, 256, lambda rows: (rnd(rows, 256).clamp_min(0), rnd(rows, 256).clamp_min(0)), run
    if kernel == "ln_linear":
        passes = 3
        w, b = dev((torch.randn(256 * passes, 256, generator=g) / 16).half()), dev(torch.randn(256 * passes, generator=g) * 0.1)
        ga, be = dev(1 + 0.2 * torch.randn(256, generator=g)), dev(0.1 * torch.randn(256, generator=g))
        packed = torch.empty(lib.pcd_pw_wide_ln_linear_packed_bytes(passes), dtype=torch.uint8, device="cuda")
        _lib.check(lib.pcd_pw_wide_ln_linear_pack(w.data_ptr(), b.data_ptr(), passes, ga.data_ptr(), be.data_ptr(), packed.data_ptr(), st))

        def run(x):
            out = nan(x.shape[0], 256 * passes)
            _lib.check(lib.pcd_pw_wide_ln_linear(packed.data_ptr(), passes, 0, x.data_ptr(), x.shape[0], out.data_ptr(), st))
            return out
        return lib.pcd_pw_wide_config, 1, 2, 256, 256, lambda rows: rnd(rows, 256, 1.7, 0.4), run
    if kernel == "wide_ffn":
        sd = sab_sd(256)
        t = [dev(sd["ff.0.weight"].half()), dev(sd["ff.0.bias"].float()), dev(sd["ff.2.weight"].half()), dev(sd["ff.2.bias"].float()),
             dev(sd["ln2.weight"].float()), dev(sd["ln2.bias"].float())]
        packed = torch.empty(lib.pcd_wide_ffn_packed_bytes(), dtype=torch.uint8, device="cuda")
        _lib.check(lib.pcd_wide_ffn_pack(*[v.data_ptr() for v in t], packed.data_ptr(), st))

        def run(x):
            y = nan(x.shape[0], 256)
            _lib.check(lib.pcd_wide_ffn_f16(packed.data_ptr(), x.data_ptr(), x.shape[0], y.data_ptr(), st))
            return y
        return lib.pcd_wide_ffn_config, 1, 0, 128, 256, lambda rows: rnd(rows, 256, 1.4, 0.2), run
    part, C = kernel.rsplit("_", 1)
    C = int(C)
    pk = _PackedSAB(sab_sd(C), "", C, torch.device("cuda"))
    desc = pk.fill(_lib.SabDesc())
    assert desc.tail_packed

    def run(ax, pk=pk):                                        # (pk owns the packed image behind desc)
        a, x = ax
        if part == "sab_tail":
            y = nan(x.shape[0], C)
            _lib.check(lib.pcd_sab_tail_f16(C, desc.tail_packed, a.data_ptr(), x.data_ptr(), x.shape[0], y.data_ptr(), st))
        else:
            y = nan(x.shape[0], 3 * C)
            _lib.check(lib.pcd_sab_head_f16(C, desc.tail_packed, x.data_ptr(), x.shape[0], y.data_ptr(), st))
        return y
    cap = 256 if C == 128 else (512 if part == "sab_tail" else 768)
    return lib.pcd_sab_tail_config, 1, 3, 256, cap, lambda rows: (rnd(rows, C, 0.7), rnd(rows, C, 1.5, 0.3)), run


@pytest.mark.parametrize("kernel", ["chain0", "chain1", "ln_linear", "wide_ffn", "sab_tail_64", "sab_tail_128", "sab_head_64", "sab_head_128"])
def test_weight_ring_request_forms_bitwise(kernel):
    """Who requests an LDS-DMA piece of a weight image (every wave its share, or one wave of each SIMD the whole of it) does not enter the arithmetic: the
    same seeded input under the default request form and under the other one gives the same BITS.  At one tile, and at grid cap + 1 tiles: exactly one
    workgroup runs a second tile, so the ring wraps across a tile boundary, the last stage takes the vmcnt(0) branch and the workgroups' tile counts differ."""
    from shapegen_amd import _lib
    config, default, other, tile, cap, inputs, run = _ring_kernel(kernel)
    for rows in (tile, (cap + 1) * tile):
        x = inputs(rows)
        try:
            _lib.check(config(default))
            a = run(x)
            _lib.check(config(other))
            b = run(x)
        finally:
            _lib.check(config(default))
        assert torch.isfinite(a).all() and a.float().abs().max() > 0
        assert torch.equal(a, b), (kernel, rows)
