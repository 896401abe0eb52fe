"""tests/latent_cases.py held to account on the CPU, so that tests/test_gpu_latent_kernels.py can judge csrc/skinny.hip, csrc/latent.hip and
csrc/latent_persist.hip by it:
  1. the restated launch geometry is the library's (pcd_skinny_slabs, pcd_skinny_fused_supported: host functions);
  2. an fp32 statement in the kernels' own order stays inside every bound on every case, and the integer cases are exact: correct fp32 code can
     meet the bounds (the largest error / bound is printed; latent_cases' docstring quotes it);
  3. the bounds bite: each mutant of an fp32 statement leaves its bound, or breaks the bitwise equality, on a case named here;
  4. the whole network per row and per column: each of three fp32 summation orders lies inside the bounds formed from the other two, three
     corruptions of the network lie outside."""
import functools

import pytest
import torch

import latent_cases as C
import train_cases as T

torch.set_grad_enabled(False)


def _worst(r):
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------ 1. geometry
def test_restated_geometry_is_the_librarys():
    from shapegen_amd import _lib
    lib = _lib.load()
    for c in (8, 32, 48, 128, 256, 512, 1024, 2048, 4096):
        for k in range(64, 5120 + 1, 64):
            assert lib.pcd_skinny_slabs(k, c) == C.slab_count(k, c), (k, c)
            assert k % C.pick_ks(k, c) == 0 and C.pick_ks(k, c) % 64 == 0
            for mode, groups in ((0, 1), (0, 2), (0, 3), (0, 8), (1, 8), (2, 8)):
                assert lib.pcd_skinny_fused_supported(k, c, mode, groups) == int(C.fused_supported(k, c, mode, groups)), (k, c, mode, groups)
    assert lib.pcd_skinny_slabs(96, 128) == 0 == C.slab_count(96, 128)
    # what the case tables say they reach
    assert [C.pick_ks(k1 + k2, c) for k1, k2, c in C.GEMM_SHAPES] == [64, 64, 128, 256, 256, 512, 256]
    assert [C.slab_count(k1 + k2, c) for k1, k2, c in C.GEMM_SHAPES] == [1, 3, 3, 1, 4, 10, 1]
    assert [C.fused_tiles(c, 0, g)[1:] for _, _, c, g in C.FUSED_SHAPES] == [(1, 16), (1, 16), (2, 8), (4, 4)]
    assert all(C.fused_supported(k1 + k2, c, 0, g) for k1, k2, c, g in C.FUSED_SHAPES) and C.fused_supported(128, 128, 1, 8)
    assert C.gemm_chain(5120, 1024) == 130 and C.fused_chain(320, 512, 0, 8) == 74 and C.finish_gn_chain(1024) == 12 and C.gn_chain(100) == 8
    assert C.finish_split(200, 1, 2) == 8 and C.finish_split(12, 2, 1) == 1 and C.finish_split(200, 0, 2) == 2


# ------------------------------------------------------------------------------------------------------------ 2. fp32 statements within bounds
@pytest.mark.parametrize("k1,k2,c", C.GEMM_SHAPES)
def test_slabs32_within_bound_and_integers_exact(k1, k2, c):
    worst = 0.0
    for m in C.gemm_ms(k1, k2, c):
        k = C.gemm_case(m, k1, k2, c, "int")
        want, bound = C.slab_statement(k["a"], k["w"], c)
        mag = k["a"].double().abs() @ k["w"].double().abs().t()
        assert float(mag.max()) < 2 ** 24 and torch.equal(want.float().double(), want)          # every partial sum is an integer below 2^24
        if m in (1, 33) or k1 + k2 <= 384:
            assert torch.equal(C.slabs32(k["a"], k["w"], c).double(), want), m
        if m in (1, 33, 256) or k1 + k2 <= 384:
            k = C.gemm_case(m, k1, k2, c, "fam")
            want, bound = C.slab_statement(k["a"], k["w"], c)
            worst = max(worst, _worst(C.ratio((C.slabs32(k["a"], k["w"], c).double() - want).abs(), bound)))
    print(f"slabs32 / bound, ({k1}, {k2}, {c}): {worst:.3f}")
    assert worst <= 1


def _finish_operands(c, groups, nslabs, with_bias, kind, rot=0):
    base = C.gn_family_case(C.FINISH_ROWS, c, groups, rot) if kind == "fam" else C.gn_plain_case(C.FINISH_ROWS, c, groups)
    g = C._gen(c, groups, nslabs, with_bias, kind == "fam")
    bias = 0.5 * torch.randn(c, generator=g) if with_bias else None
    rb = 0.5 * torch.randn(C.FINISH_ROWS, c, generator=g) if with_bias else None
    return base, C.split_into_slabs(base["x"], nslabs, bias, rb, g), bias, rb


@pytest.mark.parametrize("c,groups", C.FINISH_SHAPES[:4])
def test_finish32_mode0_within_bound(c, groups):
    worst = 0.0
    for nslabs in C.FINISH_NSLABS:
        for with_bias in (False, True):
            for kind in ("fam", "plain"):
                base, slabs, bias, rb = _finish_operands(c, groups, nslabs, with_bias, kind, rot=nslabs)
                pre = C.finish32(slabs, bias, rb, 0, pre=True)
                want, bound = C.gn_relu_statement(pre, base["gamma"], base["beta"], groups, C.finish_gn_chain(c // groups))
                got = C.gn32(pre, base["gamma"], base["beta"], groups, "finish")
                assert torch.isfinite(got.float()).all()
                r = C.ratio(C.out16_error(got, want), bound)
                worst = max(worst, _worst(r))
                assert C.first_bad(r, groups) is None, (c, groups, nslabs, with_bias, kind, C.first_bad(r, groups))
                if kind == "fam":
                    over = want[:, 1] > T.F16_MAX + bound[:, 1]
                    assert bool((got[:, 1].double()[over] == T.F16_MAX).all())
    print(f"finish mode 0 fp32 / bound, ({c}, {groups}): {worst:.3f}")


def test_plain_cases_keep_the_relu_margin():
    for c, groups in C.FINISH_SHAPES[:4]:
        assert not bool(T.gn_in_band(C.gn_plain_case(C.FINISH_ROWS, c, groups)).any())
    for groups in C.GN_GROUPS:
        for gsz in C.GN_GSZ:
            assert not bool(T.gn_in_band(C.gn_plain_case(C.GN_ROWS, groups * gsz, groups)).any())


def test_groupnorm32_within_bound():
    worst = 0.0
    saturated = 0
    for groups in C.GN_GROUPS:
        for gsz in C.GN_GSZ:
            c = groups * gsz
            for base in (C.gn_family_case(C.GN_ROWS, c, groups, rot=groups), C.gn_plain_case(C.GN_ROWS, c, groups)):
                want, bound = C.gn_relu_statement(base["x"], base["gamma"], base["beta"], groups, C.gn_chain(gsz))
                got = C.gn32(base["x"], base["gamma"], base["beta"], groups, "wave")
                r = C.ratio(C.out16_error(got, want), bound)
                worst = max(worst, _worst(r))
                assert C.first_bad(r, groups) is None, (groups, gsz, C.first_bad(r, groups))
                saturated += int((want > T.F16_MAX + bound).sum())
                # the statement is train_cases' own where both exist
                st = T.gn_stats_statement(base["x"], groups)
                y, _ = T.gn_y_statement(base["x"], st["mean"], st["rstd"], base["gamma"], base["beta"], groups, True)
                assert float((y - want).abs().max()) <= 1e-9 * float(want.abs().max())
    print(f"pcd_groupnorm_relu_f16 fp32 / bound: {worst:.3f}; {saturated} saturated elements")
    assert saturated > 0


@pytest.mark.parametrize("k1,k2,c,groups", C.FUSED_SHAPES)
def test_fused32_within_bound(k1, k2, c, groups):
    worst, cond = {}, 0.0
    for m in C.FUSED_MS:
        for kind in ("int", "rowbias", "groupbias"):
            k = C.fused_case(m, k1, k2, c, groups, kind)
            exact = kind != "groupbias"
            want, bound, z, d = C.fused_statement(k["a"], k["w"], k["bias"], k["row_bias"], 0, groups, k["gamma"], k["beta"], exact_z=exact)
            cond = max(cond, C.first_order_ok(z, groups, d))
            if m in (1, 33, 256):
                got = C.fused32(k["a"], k["w"], k["bias"], k["row_bias"], 0, groups, k["gamma"], k["beta"])
                r = C.ratio(C.out16_error(got, want), bound)
                worst[kind] = max(worst.get(kind, 0.0), _worst(r))
                assert C.first_bad(r, groups) is None, (m, kind, C.first_bad(r, groups))
            if kind == "int":
                assert torch.equal(z.float().double(), z) and float(z.abs().max()) < 2 ** 24
    print(f"fused mode 0 fp32 / bound, ({k1}, {k2}, {c}, {groups}): {worst}; max(d) rstd {cond:.2e}")
    assert cond <= 0.05          # the condition on the inputs under which the first-order bound holds


def test_fused32_plain_modes_within_bound():
    k1, k2, c = C.FUSED_PLAIN
    worst = 0.0
    for m in (1, 33, 256):
        for mode in (1, 2):
            k = C.fused_case(m, k1, k2, c, 8, "groupbias")
            want, bound, _, _ = C.fused_statement(k["a"], k["w"], k["bias"], k["row_bias"], mode, 8)
            got = C.fused32(k["a"], k["w"], k["bias"], k["row_bias"], mode, 8)
            err = C.out16_error(got, want) if mode == 1 else (got.double() - want).abs()
            worst = max(worst, _worst(C.ratio(err, bound)))
            k = C.fused_case(m, k1, k2, c, 8, "int")
            want, _, z, _ = C.fused_statement(k["a"], k["w"], k["bias"], k["row_bias"], mode, 8, exact_z=True)
            got = C.fused32(k["a"], k["w"], k["bias"], k["row_bias"], mode, 8)
            assert torch.equal(got.double(), want.clamp(max=T.F16_MAX) if mode == 1 else want)
    print(f"fused modes 1 / 2 fp32 / bound: {worst:.3f}")
    assert worst <= 1


# ------------------------------------------------------------------------------------------------------------ 3. mutants
def test_mutant_last_slab_dropped():
    """nslabs = 5 on (128, 8), mode 2."""
    base, slabs, bias, rb = _finish_operands(128, 8, 5, True, "fam")
    assert not torch.equal(C.finish32(slabs, bias, rb, 2, drop_last_of_4k1=True), C.finish32(slabs, bias, rb, 2))
    base, slabs, bias, rb = _finish_operands(128, 8, 4, True, "fam")
    assert torch.equal(C.finish32(slabs, bias, rb, 2, drop_last_of_4k1=True), C.finish32(slabs, bias, rb, 2))


def test_mutant_slice_boundary_moved_by_one_chunk():
    """(320, 64, 48) at m = 33, integers: the slab sums differ, their total does not (what the old summed check saw)."""
    k = C.gemm_case(33, 320, 64, 48, "int")
    want, _ = C.slab_statement(k["a"], k["w"], 48)
    moved, _ = C.slab_statement(k["a"], k["w"], 48, shift_chunks=1)
    assert not torch.equal(moved, want) and torch.equal(moved.sum(0), want.sum(0))


def test_mutant_second_source_with_k1_as_row_stride():
    """(64, 192, 128) at m = 33, integers; row 0 is the same either way, the others are not."""
    k = C.gemm_case(33, 64, 192, 128, "int")
    want, _ = C.slab_statement(k["a"], k["w"], 128)
    a = C.concat_sources(k["a1"], k["a2"], k1_stride_mutant=True)
    got, _ = C.slab_statement(a, k["w"], 128)
    assert torch.equal(C.concat_sources(k["a1"], k["a2"]), k["a"])
    assert torch.equal(got[:, 0, :], want[:, 0, :]) and not torch.equal(got[:, 1:], want[:, 1:])


def _gn_mutant_ratio(base, groups, chain, L, **mut):
    want, bound = C.gn_relu_statement(base["x"], base["gamma"], base["beta"], groups, L)
    return C.ratio(C.out16_error(C.gn32(base["x"], base["gamma"], base["beta"], groups, chain, **mut), want), bound)


def test_mutants_of_groupnorm_leave_the_bound():
    base = C.gn_family_case(3, 128, 8)                             # gsz 16, every family among its 24 (row, group)
    L = C.finish_gn_chain(16)
    assert _worst(_gn_mutant_ratio(base, 8, "finish", L)) <= 1
    assert _worst(_gn_mutant_ratio(base, 8, "finish", L, unbiased=True)) > 10
    assert _worst(_gn_mutant_ratio(base, 8, "finish", L, no_eps=True)) > 10
    assert _worst(_gn_mutant_ratio(base, 8, "finish", L, overflow_inf=True)) == float("inf")
    # one pass: on the +-1000 families
    r = _gn_mutant_ratio(base, 8, "finish", L, one_pass=True).reshape(3, 8, 16).amax(2)
    hit = [base["names"][row][g] for row in range(3) for g in range(8) if r[row, g] > 1]
    assert "mean_p1000" in hit and "mean_m1000" in hit, hit
    # a pair of 16-channel groups sharing their statistics: the fused kernel's (64, 0, 48, 3) shape, CT = 1
    k = C.fused_case(33, 64, 0, 48, 3, "rowbias")
    want, bound, _, _ = C.fused_statement(k["a"], k["w"], None, k["row_bias"], 0, 3, k["gamma"], k["beta"], exact_z=True)
    ok = C.fused32(k["a"], k["w"], None, k["row_bias"], 0, 3, k["gamma"], k["beta"])
    bad = C.fused32(k["a"], k["w"], None, k["row_bias"], 0, 3, k["gamma"], k["beta"], wide_stats=True)
    assert _worst(C.ratio(C.out16_error(ok, want), bound)) <= 1 < 10 < _worst(C.ratio(C.out16_error(bad, want), bound))
    # gamma of channel i >= 512 read from channel i - 512: (1024, 1)
    base = C.gn_family_case(3, 1024, 1)
    L = C.finish_gn_chain(1024)
    r = _gn_mutant_ratio(base, 1, "finish", L, gamma_wrap=True)
    assert _worst(r[:, :512]) <= 1 and _worst(r[:, 512:]) > 10
    assert _worst(_gn_mutant_ratio(C.gn_family_case(3, 4096, 8), 8, "finish", C.finish_gn_chain(512), gamma_wrap=True)) <= 1      # gsz 512: no such channel


def test_mutant_row_written_one_row_down():
    """Row m - 1 written to row m: the NaN pre-fill of the output shows the missing row, the guard region the stray one."""
    m, c = 33, 12
    val = torch.randn(m, c)
    buf = C.guarded(val, fill=C.NAN)
    buf[:m * c] = val.reshape(-1)
    assert C.guard_ok(buf, m * c) and not torch.isnan(buf[:m * c]).any()
    buf = C.guarded(val, fill=C.NAN)
    buf[:(m - 1) * c] = val[:m - 1].reshape(-1)
    buf[m * c:(m + 1) * c] = val[m - 1]
    assert not C.guard_ok(buf, m * c) and torch.isnan(buf[(m - 1) * c:m * c]).all()


def test_mutants_of_mode1_break_the_bitwise_equality():
    base, slabs, bias, rb = _finish_operands(12, 1, 3, True, "fam")
    slabs = slabs.clone()
    slabs[0, 0, 0] = 1e5                                           # the pre-activation passes 65504
    want = C.finish32(slabs, bias, rb, 1)
    assert float(want[0, 0]) == T.F16_MAX and torch.isfinite(want.float()).all() and bool((want == 0).any())
    assert not torch.equal(C.finish32(slabs, bias, rb, 1, no_relu=True), want)
    inf = C.finish32(slabs, bias, rb, 1, overflow_inf=True)
    assert torch.isinf(inf[0, 0]) and torch.equal(inf.flatten()[1:], want.flatten()[1:])


# ------------------------------------------------------------------------------------------------------------ 4. the whole network
@functools.lru_cache(maxsize=None)
def _net():
    from helpers import latent_sd
    from oracle import torch_oracle as O
    from shapegen_amd import packing
    sd = latent_sd()
    lin, gn, ex = packing.pack_latent_unet(sd, "model.")

    def trows(ts):
        temb = O.time_mlp(sd, "model.", O.timestep_embedding(ts.float(), 256)).double()
        return (temb @ torch.as_tensor(ex["e1w_t"]).t() + torch.as_tensor(ex["e1b"])).float()
    return C.pack_layers(lin, gn), trows, sd


def test_network_statement_is_the_oracles_function():
    """network() in fp64 on unrounded weights would be the oracle; with fp16 weights and activations it stays within 3e-3 of it (today's gate)."""
    from oracle import torch_oracle as O
    from helpers import rel_l2
    layers, trows, sd = _net()
    z = C.latent_input(8)
    t = torch.full((8,), 0.73)
    want = O.latent_unet(sd, "model.", z, t)
    got = C.network(layers, trows(t[:1])[0], z)
    assert rel_l2(got, want) < 2e-3


@pytest.mark.parametrize("nsteps", [0, 1, 4])
def test_network_orders_within_each_others_bounds_and_mutants_outside(nsteps):
    layers, trows, _ = _net()
    z = C.latent_input(64)
    if nsteps:
        ts, rates = C.ddim_tables(nsteps)
    else:
        ts, rates = torch.tensor([0.73]), None
    tb = trows(ts)
    want, figs = C.network_figures(layers, tb, rates, z, nsteps)
    for o in C.ORDERS:
        others = tuple(p for p in C.ORDERS if p != o)
        b = C.bounds_from(figs, others)
        for name in figs[o]:
            for f, v in figs[o][name].items():
                assert 0 < v <= b[name][f], (nsteps, o, name, f, v, b[name][f])
    e = C.bounds_from(figs, factor=1.0)
    print(f"nsteps {nsteps}: " + "; ".join(f"{n} " + " ".join(f"{f} {v:.2e}" for f, v in d.items()) for n, d in e.items()))
    if nsteps:
        return
    bounds = C.bounds_from(figs)["eps"]
    eps = C.network(layers, tb[0], z, torch.float32, "torch")
    outside = lambda got: [f for f, v in C.row_col_errors(got, want["eps"]).items() if v > bounds[f]]
    assert outside(eps) == []
    m = eps.clone(); m[17] *= 1.02
    assert "row_abs" in outside(m) and "row_l2" in outside(m)
    m = eps.clone(); m[:, 100] *= 1.05
    assert "col_abs" in outside(m) and "col_l2" in outside(m)
    assert outside(C.network(layers, tb[0], z, torch.float32, "torch", shift_z3_mutant=True)) != []
    # what the whole-tensor gate saw of the first two
    from helpers import rel_l2
    m = eps.clone(); m[17] *= 1.02
    assert rel_l2(m, want["eps"]) < 3e-3
