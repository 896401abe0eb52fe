"""CPU-side checks of the boundary: the shared library loads, exports every symbol the
header declares, the ctypes table covers them, and the host logic that needs no GPU."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "pcd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pcd_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_header_symbols():
    from shapegen_amd import _lib
    _lib.build()
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/pcd_hip.h but not exported"
        assert n in _lib._SIGS, f"{n} has no ctypes prototype"
    assert set(_lib._SIGS) == set(names)
    assert "pcd_gemm_plan" in names and "pcd_gemm_set_config" in names
    assert lib.pcd_abi_version() == _lib.ABI_VERSION == 2


def test_arg_validation_without_gpu():
    """Argument errors are reported before any device work."""
    from shapegen_amd import _lib
    lib = _lib.load()
    d = _lib.GemmDesc()
    assert lib.pcd_gemm_f16(d, 0, 0, 0) == -1
    assert b"bad argument" in lib.pcd_last_error()
    assert lib.pcd_unet_workspace_bytes(64, 2048) == lib.pcd_unet_workspace_bytes(64, 2048) > 1 << 30
    assert lib.pcd_unet_workspace_bytes(0, 5) == 0
    # conv3d: shape logic is host side -- the LDS-halo path is offered only for k3 / s1 / p1, C_in 32 or 64 and
    # volumes that tile by (4, 4, 8); split-K scratch is asked for exactly when the launch would be small
    c = _lib.Conv3dDesc()
    assert lib.pcd_conv3d_k3s1_supported(c) == 0 and lib.pcd_conv3d_workspace_bytes(c, 1) == 0
    assert lib.pcd_conv3d_f16(c, 0) == -1 and lib.pcd_conv3d_k3s1_f16(c, 0) == -1
    c.inp = c.w = c.out = c.taps = c.zero_page = 64                       # never dereferenced on the host
    c.batch, c.in_d, c.in_h, c.in_w, c.cin, c.cout = 32, 32, 32, 32, 64, 64
    c.rows_d = c.rows_h = c.rows_w = c.out_d = c.out_h = c.out_w = 32
    c.stride, c.out_scale, c.ntaps, c.kpad = 1, 1, 27, 27 * 64
    assert lib.pcd_conv3d_k3s1_supported(c) == 1
    assert lib.pcd_conv3d_workspace_bytes(c, 1) == 0                         # 8192 output tiles: no split
    c.in_w = c.rows_w = c.out_w = 36
    assert lib.pcd_conv3d_k3s1_supported(c) == 0
    c.in_d = c.in_h = c.in_w = c.rows_d = c.rows_h = c.rows_w = c.out_d = c.out_h = c.out_w = 4
    c.cin, c.cout, c.kpad = 512, 512, 27 * 512                               # encoder.11: 16 x 4 tiles, 216 K tiles
    ws = lib.pcd_conv3d_workspace_bytes(c, 1)
    assert ws > 0 and ws % (32 * 64 * 512 * 4) == 0                          # whole fp32 slabs [M][C_out]
    assert lib.pcd_conv3d_workspace_bytes(c, 9) == 0                         # more than 8 variants: refused


def test_packing_is_exact_algebra():
    """BN folding + refine folding + hoisting reproduce the oracle forward in float64."""
    from shapegen_amd import packing, specs
    from oracle import torch_oracle as O
    from helpers import point_sd, rel_l2
    sd = point_sd("")
    lin, ex = packing.pack_point_unet(sd, "", 256, 256)
    g = torch.Generator().manual_seed(0)
    x, t = torch.randn(2, 32, 3, generator=g), torch.tensor([0.3, 0.8])
    want = O.unet_pointnet_large(sd, "", x, t)
    temb = O.time_mlp(sd, "", O.timestep_embedding(t, 256)).double().numpy()
    relu = lambda v: np.maximum(v, 0)
    tb = temb @ ex["e1w_t"].T + ex["e1b"]
    h = relu(x.double().numpy() @ ex["e1w_xyz"].T + tb[:, None, :])
    f = lambda i, v: relu(v @ lin[i][0].T + lin[i][1])
    h = f(1, f(0, h)); x1 = h
    h = f(4, f(3, f(2, h))); x2 = h
    h = f(7, f(6, f(5, h))); x3 = h
    h = f(10, f(9, f(8, h))); x4 = h
    pooled = f(12, f(11, h)).max(axis=1)
    gb = pooled @ ex["wg"].T + lin[13][1]
    h = relu(x4 @ lin[13][0].T + gb[:, None, :])
    h = f(15, f(14, h))
    h = f(18, f(17, f(16, np.concatenate([h, x3], -1))))
    h = f(21, f(20, f(19, np.concatenate([h, x2], -1))))
    h = f(24, f(23, f(22, np.concatenate([h, x1], -1))))
    h = f(25, h)
    eps = h @ ex["head_w"].T + ex["head_b"]
    assert rel_l2(eps, want) < 1e-5
    with pytest.raises(RuntimeError):
        packing.pack_point_unet(sd, "", 256, 512)


def test_hi_lo_weight_split_and_the_forward_it_implies():
    """`packing.split_hilo`: [C][2 K] fp16 = hi | lo with hi + lo = w to ~2^-22; and a float64 emulation of the product path's WEIGHT
    precision on (2, 32): folded weights rounded to fp16 everywhere, against the same with the narrow layers (the library's
    PCD_UNET_HILO_ALLOWED mask) carried as hi + lo -- the second is closer to the oracle on eps (activations stay float64 here, so
    this isolates what the hi / lo weights change; the measured 1000-step effect is in profiles/r04_f)."""
    from shapegen_amd import _lib, packing
    from oracle import torch_oracle as O
    from helpers import point_sd, rel_l2
    g = np.random.default_rng(0)
    w = g.standard_normal((64, 128)) / 11.3
    hl = packing.split_hilo(w)
    assert hl.dtype == np.float16 and hl.shape == (64, 256)
    back = hl[:, :128].astype(np.float64) + hl[:, 128:].astype(np.float64)
    assert np.abs(back - w).max() <= 2.0 ** -21 * np.abs(w).max()
    assert np.abs(hl[:, :128].astype(np.float64) - w).max() > 2.0 ** -14 * np.abs(w).max()      # what plain fp16 rounding loses
    assert _lib.PCD_UNET_HILO_ALLOWED == sum(1 << i for i in (0, 1, 4, 22, 23, 24, 25))
    sd = point_sd("")
    lin, ex = packing.pack_point_unet(sd, "", 256, 256)
    gen = torch.Generator().manual_seed(1)
    x, t = torch.randn(2, 32, 3, generator=gen), torch.tensor([0.4, 0.7])
    want = O.unet_pointnet_large(sd, "", x, t)
    temb = O.time_mlp(sd, "", O.timestep_embedding(t, 256)).double().numpy()
    relu = lambda v: np.maximum(v, 0)
    r16 = lambda a: a.astype(np.float16).astype(np.float64)

    def forward(mask):
        def wq(i):
            if (mask >> i) & 1:
                h = packing.split_hilo(lin[i][0]).astype(np.float64)
                return h[:, :lin[i][0].shape[1]] + h[:, lin[i][0].shape[1]:]
            return r16(lin[i][0])
        f = lambda i, v: relu(v @ wq(i).T + lin[i][1])
        tb = temb @ ex["e1w_t"].T + ex["e1b"]
        h = relu(x.double().numpy() @ ex["e1w_xyz"].T + tb[:, None, :])
        h = f(1, f(0, h)); x1 = h
        h = f(4, f(3, f(2, h))); x2 = h
        h = f(7, f(6, f(5, h))); x3 = h
        h = f(10, f(9, f(8, h))); x4 = h
        pooled = f(12, f(11, h)).max(axis=1)
        gb = pooled @ r16(ex["wg"]).T + lin[13][1]
        h = relu(x4 @ wq(13).T + gb[:, None, :])
        h = f(15, f(14, h))
        h = f(18, f(17, f(16, np.concatenate([h, x3], -1))))
        h = f(21, f(20, f(19, np.concatenate([h, x2], -1))))
        h = f(24, f(23, f(22, np.concatenate([h, x1], -1))))
        return f(25, h) @ ex["head_w"].T + ex["head_b"]

    e_plain, e_hilo = rel_l2(forward(0), want), rel_l2(forward(_lib.PCD_UNET_HILO_ALLOWED), want)
    assert e_hilo < 0.6 * e_plain and e_plain < 3e-3, (e_plain, e_hilo)


def test_module_state_dict_and_cpu_failure():
    from shapegen_amd import specs
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=32)
    want = [(k, s) for k, s, _ in specs.unet_pointnet_large_spec(prefix="model.")]
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert m.hparams.num_points == 32 and m.hparams["noise_schedule"] == "cosine"
    n, s = m.diffusion_schedule(torch.tensor([0.0, 0.5, 1.0]))
    np.testing.assert_allclose(s.numpy(), [0.95, 0.5944798, 0.02000003], rtol=1e-6)
    with pytest.raises(RuntimeError):
        m.sample(1, 32, num_steps=1)     # no CPU path: fail loudly


def test_linear_schedule_bug_for_bug():
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=8, noise_schedule="linear")
    n, s = m.diffusion_schedule(torch.tensor([0.5, 0.5, 0.5]))
    np.testing.assert_allclose(s.numpy(), [0.98995, 0.98000, 0.97015], atol=1e-5)   # SURVEY a2 probe


@pytest.mark.parametrize("T", [1, 2, 7, 100, 1000])
def test_vectorized_step_tables_equal_the_per_step_loop(T):
    """The step tables are built with one set of elementwise ops over all T steps and the whole width; the literal
    per-step transcription of the reference loops (diffusion.py:241-255, 277-286, 323-335; tests/table_statement.py, over
    the oracle's schedules) must give the same bits: cosine (width 1 whatever the batch) and linear (width = batch, each
    row the batch-axis cumprod the reference's loop saw; a 0-d time, hence width 1, from a state)."""
    import table_statement as S
    from oracle import torch_oracle as O
    from shapegen_amd.diffusion import PointCloudDiffusion
    for schedule, batches in (("cosine", (4,)), ("linear", (1, 3, 4, 64))):
        m = PointCloudDiffusion(num_points=8, noise_schedule=schedule)
        sched = O.schedule_fn(schedule)
        pairs = [(m.from_state_table(st, T), S.from_state(st, T, sched), 1) for st in (torch.tensor(0.37), 1.0, torch.tensor(0.3))]
        for B in batches:
            w = 1 if schedule == "cosine" else B
            pairs += [(m.ddim_table(T, B), S.ddim(T, w, sched), w), (m.ddpm_table(T, B), S.ddpm(T, w, sched), w)]
        for a, b, w in pairs:
            assert a.steps == T and a.width == w and a.stride == (0 if w == 1 else 1)
            for f in ("t", "n", "s", "a", "b"):
                assert torch.equal(getattr(a, f), b[f]), (schedule, w, f)


def test_stepper_refuses_an_unknown_kind_before_touching_the_device():
    """A kind is looked up once, at construction: a misspelt one raises and names the four, before the library is loaded or
    anything is allocated (a CPU state and a two-row table get that far)."""
    from shapegen_amd import _lib
    from shapegen_amd.diffusion import PointCloudDiffusion, Stepper
    m = PointCloudDiffusion(num_points=8)
    tab = m.ddim_table(2, 1)
    x, bias = torch.zeros(1, 8, 3), torch.zeros(2, 64)
    loaded = _lib.load
    _lib.load = lambda: pytest.fail("the library was loaded before the kind was checked")
    try:
        with pytest.raises(ValueError, match="'ddim', 'ddpm', 'dpm', 'complete'.*'dim'"):
            Stepper(m, x, tab, bias, m._forward_fn(), "dim")
        with pytest.raises(ValueError, match="'ddim', 'ddpm', 'dpm', 'complete'"):
            m._run(x, tab, bias, m._forward_fn(), "DDPM")
    finally:
        _lib.load = loaded


def test_persistent_latent_plan_is_a_partition():
    """csrc/latent_persist.hip's static work assignment, checked on the host without a device: every (layer, 32-column tile,
    64-k chunk) belongs to exactly one gemm unit, every (GroupNorm group, row) of a layer with partial slabs to exactly one
    finish unit, unit lists are in phase order and every workgroup's LDS plan fits 160 KB."""
    from shapegen_amd import _lib
    set_bytes = _lib.load().pcd_latent_persist_plan_check()
    assert set_bytes > 0 and set_bytes % 4096 == 0 and set_bytes < 8 << 20


def test_pair_metrics_workspace_layout_without_gpu():
    """`pcd_pair_metrics_workspace_layout` is host arithmetic: the stage buffers come in the header's PCD_PAIR_WS_* order, every one
    256-byte aligned and large enough for its documented shape, and the last field is `pcd_pair_metrics_workspace_bytes`."""
    import ctypes as C
    from shapegen_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pcd_hip.h")).read()
    enum = re.search(r"enum\s*\{\s*(PCD_PAIR_WS_AN[^}]*)\}", header).group(1)
    names = [n.split("=")[0].strip()[len("PCD_PAIR_WS_"):].lower() for n in enum.split(",")]
    assert names[-1] == "fields" and tuple(names[:-1]) == _lib.PCD_PAIR_WS
    for P, na, nb in ((1, 1, 1), (6, 1300, 1300), (3, 96, 80), (256, 1100, 1300), (512, 8, 7)):
        lay = _lib.pair_metrics_workspace_layout(P, na, nb)
        assert list(lay) == list(_lib.PCD_PAIR_WS) and lay["an"] == 0
        assert lay["total"] == lib.pcd_pair_metrics_workspace_bytes(P, na, nb)
        nq = max(na, nb)
        need = dict(an=P * na * 12, bn=P * nb * 12, mins=P * 2 * nq * 4, alpha=P * na * 4, beta=P * nb * 4, rowc=P * na * 4,
                    cmax=P * 4, err=2 * P * 2 * 4, bits=P * 2 * 1024 * 4)
        order = list(_lib.PCD_PAIR_WS)
        for k, nxt in zip(order[:-1], order[1:]):
            assert lay[k] % 256 == 0 and lay[nxt] - lay[k] >= need[k], (P, na, nb, k)
    off = (C.c_size_t * len(_lib.PCD_PAIR_WS))()
    assert lib.pcd_pair_metrics_workspace_layout(0, 4, 4, off) == -1 and lib.pcd_pair_metrics_workspace_layout(1, 4, 4, None) == -1


def _conv_desc(_lib, B, dims, cin, cout, k, stride, cin2):
    """A descriptor as the VAE runner builds it: rows = dims // stride (k4 / stride 1 / pad 0: one row), out = rows."""
    dims = (dims,) * 3 if isinstance(dims, int) else dims
    rows = (1, 1, 1) if (k == 4 and stride == 1) else tuple(d // stride for d in dims)
    c = _lib.Conv3dDesc()
    c.inp = c.w = c.out = c.taps = c.zero_page = 64                       # never dereferenced on the host
    c.batch, (c.in_d, c.in_h, c.in_w), c.cin, c.cout = B, dims, cin, cout
    c.rows_d, c.rows_h, c.rows_w = c.out_d, c.out_h, c.out_w = rows
    c.stride, c.out_scale, c.ntaps = stride, 1, k ** 3
    c.kpad = (k ** 3 * cin + cin2 + 63) // 64 * 64
    c.in2, c.cin2 = (64 if cin2 > 0 else None), cin2
    return c


def test_conv3d_and_vae_host_plan_is_the_recorded_one():
    """What the convolution and VAE entry points decide on the host, for the layers of VAE3DLarge and some awkward shapes, as recorded from
    the library before the convolution code was split by kernel family (no GPU): which forms support a layer, the split-K scratch a launch asks for under each
    split target, which configuration codes are valid, and the sizes of the packed copies and of the VAE workspace."""
    from shapegen_amd import _lib
    lib = _lib.load()
    # (B, dims, cin, cout, k, stride, cin2) -> k3s1_supported, wreg_supported, workspace_bytes(n = 1), workspace_bytes(n = 8)
    plan = [((32, 32, 32, 64, 3, 1, 0), (1, 1, 0, 0)),
            ((32, 32, 64, 64, 3, 1, 32), (1, 1, 0, 0)),
            ((32, 32, 64, 64, 4, 2, 0), (0, 0, 0, 0)),
            ((32, 16, 64, 128, 3, 1, 0), (1, 1, 0, 0)),
            ((32, 16, 128, 128, 3, 1, 64), (0, 1, 0, 0)),
            ((32, 16, 128, 128, 4, 2, 0), (0, 0, 33554432, 0)),
            ((32, 8, 128, 256, 3, 1, 0), (0, 1, 33554432, 0)),
            ((4, 8, 256, 256, 3, 1, 128), (0, 0, 33554432, 33554432)),
            ((4, 8, 256, 256, 4, 2, 0), (0, 0, 16777216, 33554432)),
            ((1, 4, 256, 512, 3, 1, 0), (0, 0, 3538944, 16777216)),
            ((32, 4, 512, 512, 3, 1, 0), (0, 0, 33554432, 0)),
            ((32, 4, 512, 512, 4, 1, 0), (0, 0, 4194304, 8388608)),
            ((2, 32, 64, 32, 3, 1, 0), (1, 1, 0, 0)),
            ((2, 32, 32, 32, 3, 1, 0), (1, 1, 0, 0)),
            ((3, (5, 3, 7), 64, 72, 3, 1, 0), (0, 0, 544320, 4354560)),
            ((2, (4, 12, 8), 32, 32, 3, 1, 0), (1, 0, 294912, 2359296)),
            ((2, (4, 8, 4), 64, 64, 3, 1, 0), (0, 0, 393216, 3145728))]
    for layer, want in plan:
        c = _conv_desc(_lib, *layer)
        got = (lib.pcd_conv3d_k3s1_supported(c), lib.pcd_conv3d_k3s1_wreg_supported(c),
               lib.pcd_conv3d_workspace_bytes(c, 1), lib.pcd_conv3d_workspace_bytes(c, 8))
        assert got == want, (layer, got, want)
    # the configuration code is decoded field by field: the split-K target, seen through the scratch of encoder.11
    c = _conv_desc(_lib, 32, 4, 512, 512, 3, 1, 0)
    try:
        for code, want in ((1, 33554432), (65, 25165824), (33, 50331648), (97, 67108864)):
            assert lib.pcd_conv3d_config(code) == 0
            assert lib.pcd_conv3d_workspace_bytes(c, 1) == want, code
    finally:
        assert lib.pcd_conv3d_config(1) == 0
    try:
        for code in (0, 1, 2, 8, 9, 25, 513, 16385):
            assert lib.pcd_conv3d_config(code) == 0, code
        for code in (-1, 3, 4, 7, 11, 262143, 262144, 262145):
            assert lib.pcd_conv3d_config(code) == -1, code
    finally:
        assert lib.pcd_conv3d_config(1) == 0
    try:
        for code in (0, 1, 2, 14, 15):
            assert lib.pcd_vae_config(code) == 0, code
        for code in (-1, 16):
            assert lib.pcd_vae_config(code) == -1, code
    finally:
        assert lib.pcd_vae_config(1) == 0
    wfrag = {(32, 32): 57344, (32, 64): 114688, (64, 32): 114688, (64, 64): 229376, (64, 192): 688128, (128, 128): 901120,
             (128, 256): 1802240, (64, 72): 0, (128, 192): 0, (256, 256): 0, (16, 32): 0}
    for (cin, cout), want in wfrag.items():
        assert lib.pcd_conv3d_wfrag_bytes(cin, cout) == want, (cin, cout)
    for args, want in (((32, 32, 32, 32, 64, 64, 4096), 1), ((1, 8, 8, 16, 64, 64, 4096), 1), ((1, 8, 8, 8, 64, 64, 4096), 0),
                       ((1, 16, 16, 16, 128, 128, 8192), 0), ((1, 8, 8, 16, 64, 64, 4032), 0)):
        assert lib.pcd_conv3d_k4s2_halo_supported(*args) == want, args
    for args, want in (((32, 16, 16, 16, 128, 64), 1), ((1, 4, 4, 8, 128, 64), 1), ((1, 4, 4, 4, 128, 64), 0), ((1, 8, 8, 8, 256, 128), 0)):
        assert lib.pcd_convt3d_k4s2_halo_supported(*args) == want, args
    assert lib.pcd_conv3d_last_packed_bytes() == 27648
    for batch, want in ((0, 0), (1, 46141440), (4, 83902464), (5, 104878080), (32, 671219712)):
        assert lib.pcd_vae_workspace_bytes(batch) == want, batch


def test_gemm_host_plan():
    """What the GEMM entry points decide on the host (`pcd_gemm_plan`: the plan the entry point itself launches from, no GPU), row by row against
    expectations worked out by hand from the conditions of the code before it had one planner: the generic tile, the three 256 x 256 kernel families and
    each conjunct that refuses them, the template instance, grid and block, the XCD patch map, the zero-row needs, and every configuration code."""
    import ctypes as C
    from shapegen_amd import _lib
    lib = _lib.load()
    F16, HILO, OUT32, SPLITK, RESID, COLMAX, CMW, WFRAG = range(8)
    XP, XW, XS = 5, 6, 7
    DEFAULTS = (-1, 7, 9, 11, 12, 15, 16)

    def P(family, instance, grid, block, tiles_m, tiles_n, pn=0, xn=0, xp_depth=0, abl=0, zb=0, zsb=0, nz=0):
        return (family, instance, grid, block, tiles_m, tiles_n, pn, xn, xp_depth, abl, zb, zsb, nz)

    def plan(entry, m, k1, k2, c, same_lda=True, bias=True, sb_rows=0, rps=0, splits=0, wfrag=False):
        d = _lib.GemmDesc()
        d.a1 = d.w = 64                                                       # never dereferenced on the host
        d.a2 = 64 if k2 else None
        d.k1, d.k2, d.lda1, d.lda2 = k1, k2, k1, (k1 if same_lda else k1 + k2) if k2 else 0
        d.ldw = (k1 + k2) * (2 if entry == HILO else 1)
        d.bias = 64 if bias else None
        d.shape_bias, d.rows_per_shape = (64 if sb_rows else None), sb_rows
        d.relu, d.m, d.c = (0 if entry == SPLITK else 1), m, c
        out = _lib.GemmPlan()
        if lib.pcd_gemm_plan(d, entry, rps, splits, int(wfrag), C.byref(out)) != 0:
            return None
        return tuple(getattr(out, f) for f, _ in _lib.GemmPlan._fields_)

    xp512 = P(XP, 0, 256, 512, 256, 2, 2, 1, xp_depth=1, zsb=1)               # 65536 x 256 x 512: 512 tiles, two per workgroup, patches of 16 x 2 tiles
    g512 = P(3, 0, 256, 512, 256, 2, 2, 1)                                    # the same launch shape on the generic 256 x 256 kernel
    xp1 = lambda tiles_m, grid, patched: P(XP, 0, grid, 512, tiles_m, 1, int(patched), int(patched), xp_depth=1, zsb=1)
    rows = [
        # the heuristic's generic tiles
        ((F16, 1000, 256, 0, 64), {}, P(0, 0, 8, 256, 8, 1)),                                  # c <= 64: 128 x 64
        ((F16, 16128, 256, 0, 512), {}, P(1, 0, 504, 256, 126, 4)),                            # m < 16384: 128 x 128, 504 tiles under the 512 resident
        ((F16, 65536, 128, 0, 512), {}, P(1, 0, 512, 256, 512, 4)),                            # k < 256: 128 x 128, 2048 tiles capped at 2 per CU
        ((OUT32, 65536, 256, 0, 512), {}, g512),                                               # the 256 x 256 tile; the fp32 epilogue has no xp form
        # gemm_xp_kernel taken, and refused by each conjunct in turn
        ((F16, 65536, 256, 0, 512), {}, xp512),                                                # taken; the missing per-shape bias is the zero row
        ((F16, 65536, 256, 0, 512), dict(bias=False, sb_rows=2048), P(XP, 0, 256, 512, 256, 2, 2, 1, xp_depth=1, zb=1)),   # ... the missing bias
        ((RESID, 65536, 256, 0, 512), {}, xp512),                                              # residual epilogue: taken
        ((COLMAX, 65536, 256, 0, 512), dict(rps=2048), xp512),                                 # column max: taken
        ((F16, 65536, 128, 128, 512), {}, xp512),                                              # two sources with one row stride: taken
        ((HILO, 65536, 256, 0, 512), {}, g512),                                                # krep == 2
        ((F16, 65544, 256, 0, 512), {}, P(3, 0, 256, 512, 257, 2)),                            # ragged m (514 tiles: no patch map either)
        ((F16, 65536, 256, 0, 520), {}, P(3, 0, 256, 512, 256, 3)),                            # ragged c (3 column tiles: no patch map)
        ((F16, 65536, 64, 0, 512), dict(code=3), g512),                                        # nk = 1 (tile 3 forced: the heuristic would not pick it)
        ((F16, 65536, 128, 128, 512), dict(same_lda=False), g512),                             # lda2 != lda1
        ((F16, 65536, 256, 0, 512), dict(sb_rows=128), g512),                                  # per-shape rows not a multiple of 256
        ((COLMAX, 65536, 256, 0, 512), dict(rps=64), g512),                                    # cm_rps % 128
        # gemm_xs_kernel (pcd_gemm_f16_wfrag): R = 1 from 12 K tiles, R = 2 for 6 .. 11, pcd_gemm_f16's choice otherwise
        ((WFRAG, 65536, 768, 0, 256), dict(wfrag=True), P(XS, 0, 256, 512, 256, 1, 1, 1, zsb=1, nz=1)),          # nk 12: R = 1
        ((WFRAG, 65536, 384, 0, 256), dict(wfrag=True), P(XS, 4, 256, 512, 256, 1, 1, 1, zsb=1, nz=1)),          # nk 6: R = 2
        ((WFRAG, 65536, 704, 0, 256), dict(wfrag=True), P(XS, 4, 256, 512, 256, 1, 1, 1, zsb=1, nz=1)),          # nk 11: R = 2
        ((WFRAG, 65536, 384, 0, 256), dict(wfrag=True, bias=False, sb_rows=2048), P(XS, 4, 256, 512, 256, 1, 1, 1, zb=1, nz=1)),   # zero row for the bias
        ((WFRAG, 65536, 320, 0, 256), dict(wfrag=True), xp1(256, 256, True)),                  # nk 5: refused
        ((WFRAG, 65280, 384, 0, 256), dict(wfrag=True), xp1(255, 255, False)),                 # 255 tiles: refused
        ((WFRAG, 65792, 384, 0, 256), dict(wfrag=True), xp1(257, 256, False)),                 # 257 tiles: refused
        ((WFRAG, 65536, 384, 0, 256), {}, xp1(256, 256, True)),                                # no fragment copy passed
        ((WFRAG, 65536, 192, 192, 256), dict(wfrag=True, same_lda=False), P(3, 0, 256, 512, 256, 1, 1, 1)),      # lda2 != lda1: neither xs nor xp
        # gemm_xw_kernel (pcd_gemm_f16_colmax_wfrag): taken, or the entry point refuses
        ((CMW, 65536, 128, 0, 256), dict(wfrag=True, rps=2048), P(XW, 0, 256, 512, 256, 1, 1, 1, zsb=1, nz=2)),
        ((CMW, 16384, 2048, 0, 4096), dict(wfrag=True, rps=2048), P(XW, 0, 256, 512, 64, 16, 8, 2, zsb=1, nz=2)),   # global_feat.3 at batch 8
        ((CMW, 8192, 128, 0, 256), dict(wfrag=True, rps=2048), None),                          # 32 tiles
        ((CMW, 65536, 64, 0, 256), dict(wfrag=True, rps=2048), None),                          # nk = 1
        ((CMW, 65536, 128, 0, 256), dict(wfrag=True, rps=64), None),                           # shapes of half a wave tile
        ((CMW, 65536, 128, 0, 256), dict(wfrag=True, rps=2048, bias=False), None),             # no bias
        ((CMW, 65536, 128, 0, 256), dict(wfrag=True, rps=2048, sb_rows=2048), None),           # a per-shape bias
        ((CMW, 65536, 128, 0, 256), dict(rps=2048), None),                                     # no fragment copy
        # the XCD patch map: 1, 2, 4, 8, 16 column tiles, and a tiles_m that fails the divisibility although the tiles fill whole rounds
        ((F16, 65536, 256, 0, 256), {}, xp1(256, 256, True)),
        ((F16, 16384, 256, 0, 1024), {}, P(XP, 0, 256, 512, 64, 4, 4, 1, xp_depth=1, zsb=1)),
        ((F16, 16384, 256, 0, 2048), {}, P(XP, 0, 256, 512, 64, 8, 8, 1, xp_depth=1, zsb=1)),
        ((F16, 16384, 256, 0, 4096), {}, P(XP, 0, 256, 512, 64, 16, 8, 2, xp_depth=1, zsb=1)),
        ((F16, 18432, 256, 0, 8192), {}, P(XP, 0, 256, 512, 72, 32, 0, 0, xp_depth=1, zsb=1)),                   # 2304 tiles = 9 rounds, 72 % 16 != 0
        # split-K: tiles x splits, capped at the resident blocks; never a patch map, also at 256 blocks and whole rounds
        ((SPLITK, 1024, 8192, 0, 512), dict(bias=False, splits=4), P(1, 0, 128, 256, 8, 4)),
        ((SPLITK, 1024, 8192, 0, 512), dict(bias=False, splits=32), P(1, 0, 512, 256, 8, 4)),
        ((SPLITK, 1024, 8192, 0, 1024), dict(bias=False, splits=4, code=3), P(3, 0, 64, 512, 4, 4)),
        ((SPLITK, 2048, 8192, 0, 1024), dict(bias=False, splits=8, code=3), P(3, 0, 256, 512, 8, 4)),
        ((SPLITK, 1024, 8192, 0, 512), dict(bias=False, splits=3), None),                      # K / splits not a multiple of 64
        # configuration codes, one field each
        ((F16, 65536, 256, 0, 512), dict(code=5), g512),                                       # 5: gemm_xp_kernel off
        ((F16, 65536, 256, 0, 512), dict(code=6), P(XP, 0, 256, 512, 256, 2, 2, 1, xp_depth=2, zsb=1)),          # 6: two K tiles ahead
        ((COLMAX, 65536, 256, 0, 512), dict(code=6, rps=2048), xp512),                         # ... store epilogue only
        ((F16, 65536, 256, 0, 512), dict(code=7), xp512),                                      # 7: the default
        ((CMW, 65536, 128, 0, 256), dict(code=8, wfrag=True, rps=2048), P(XW, 0, 256, 512, 256, 1, 1, 1, zsb=1, nz=2)),   # 8: asked by callers only
        ((WFRAG, 65536, 768, 0, 256), dict(code=10, wfrag=True), xp1(256, 256, True)),         # 10: gemm_xs_kernel off
        ((WFRAG, 65536, 768, 0, 256), dict(code=13, wfrag=True), P(XS, 2, 256, 512, 256, 1, 1, 1, zsb=1, nz=1)),          # 13: request position
        ((WFRAG, 65536, 384, 0, 256), dict(code=13, wfrag=True), P(XS, 6, 256, 512, 256, 1, 1, 1, zsb=1, nz=1)),
        ((CMW, 65536, 128, 0, 256), dict(code=13, wfrag=True, rps=2048), P(XW, 2, 256, 512, 256, 1, 1, 1, zsb=1, nz=2)),
        ((WFRAG, 65536, 768, 0, 256), dict(code=14, wfrag=True), P(XS, 1, 256, 512, 256, 1, 1, 1, zsb=1, nz=1)),          # 14: every wave requests
        ((WFRAG, 65536, 384, 0, 256), dict(code=14, wfrag=True), P(XS, 5, 256, 512, 256, 1, 1, 1, zsb=1, nz=1)),
        ((CMW, 65536, 128, 0, 256), dict(code=14, wfrag=True, rps=2048), P(XW, 1, 256, 512, 256, 1, 1, 1, zsb=1, nz=2)),
        ((CMW, 65536, 128, 0, 256), dict(code=(14, 13), wfrag=True, rps=2048), P(XW, 2, 256, 512, 256, 1, 1, 1, zsb=1, nz=2)),   # the position wins
        ((CMW, 65536, 128, 0, 256), dict(code=33, wfrag=True, rps=2048), P(XW, 3, 256, 512, 256, 1, 1, 1, zsb=1, nz=2)),  # 33: late weights ...
        ((WFRAG, 65536, 768, 0, 256), dict(code=33, wfrag=True), P(XS, 2, 256, 512, 256, 1, 1, 1, zsb=1, nz=1)),          # ... and the store kernel as under 13
        ((WFRAG, 65536, 768, 0, 256), dict(code=17, wfrag=True), P(XS, 3, 256, 512, 256, 1, 1, 1, abl=1, zsb=1, nz=1)),   # 16 + 1: ablation instance
        ((WFRAG, 65536, 384, 0, 256), dict(code=(13, 14, 18), wfrag=True), P(XS, 7, 256, 512, 256, 1, 1, 1, abl=2, zsb=1, nz=1)),   # ... before the others
        ((F16, 65536, 256, 0, 512), dict(code=17), xp512),                                     # ... and of that kernel alone
        # forced tiles 0 .. 4 (blocks per CU 3, 2, 1, 1, 1): a generic kernel at 256 blocks and whole rounds takes the patch map too
        ((F16, 16384, 128, 0, 1024), dict(code=0), P(0, 0, 768, 256, 128, 16)),
        ((F16, 16384, 128, 0, 1024), dict(code=1), P(1, 0, 512, 256, 128, 8)),
        ((F16, 16384, 128, 0, 1024), dict(code=2), P(2, 0, 256, 512, 64, 8, 8, 1)),
        ((F16, 16384, 128, 0, 1024), dict(code=3), P(XP, 0, 256, 512, 64, 4, 4, 1, xp_depth=1, zsb=1)),
        ((F16, 16384, 128, 0, 1024), dict(code=4), P(4, 0, 256, 256, 128, 8, 8, 1)),
        ((F16, 1000, 256, 0, 64), dict(code=3), P(3, 0, 4, 512, 4, 1)),
    ]
    for args, kw, want in rows:
        kw = dict(kw)
        code = kw.pop("code", ())
        try:
            for cfg in (code if isinstance(code, tuple) else (code,)):
                assert lib.pcd_gemm_set_config(cfg) == 0, cfg
            got = plan(*args, **kw)
        finally:
            for cfg in DEFAULTS:
                assert lib.pcd_gemm_set_config(cfg) == 0
        assert got == want, (args, kw, code, got, want)
    # the two switches that callers read back
    try:
        assert lib.pcd_gemm_wfrag_enabled() == 1 and lib.pcd_gemm_store_wfrag_enabled() == 1
        assert lib.pcd_gemm_set_config(8) == 0 and lib.pcd_gemm_wfrag_enabled() == 0 and lib.pcd_gemm_store_wfrag_enabled() == 1
        assert lib.pcd_gemm_set_config(10) == 0 and lib.pcd_gemm_store_wfrag_enabled() == 0
    finally:
        assert lib.pcd_gemm_set_config(9) == 0 and lib.pcd_gemm_set_config(11) == 0
    assert lib.pcd_gemm_wfrag_enabled() == 1 and lib.pcd_gemm_store_wfrag_enabled() == 1
    # accepted and refused codes
    try:
        for cfg in list(range(-1, 32)) + [33]:
            assert lib.pcd_gemm_set_config(cfg) == 0, cfg
        for cfg in (-2, 32, 34):
            assert lib.pcd_gemm_set_config(cfg) == -1, cfg
    finally:
        for cfg in DEFAULTS:
            assert lib.pcd_gemm_set_config(cfg) == 0
    assert plan(F16, 65536, 256, 0, 512) == xp512
    # pcd_gemm_f16_colmax_wfrag itself refuses a shape gemm_xw_kernel does not take (nothing is launched, so no device is needed): 32 tiles
    d = _lib.GemmDesc()
    d.a1 = d.w = d.bias = 64
    d.k1, d.lda1, d.ldw, d.relu, d.m, d.c = 128, 128, 128, 1, 8192, 256
    assert lib.pcd_gemm_f16_colmax_wfrag(d, 64, 64, 2048, 0) == -1 and b"gemm_xw_kernel" in lib.pcd_last_error()
