"""The latent denoiser's kernels (csrc/skinny.hip, csrc/latent.hip, csrc/latent_persist.hip) through their C entry points, every launch judged
against the fp64 statements of tests/latent_cases.py with the bounds derived there: the split-K GEMM slab by slab and element by element (bitwise on
the integer cases, which pin every k to its slab), pcd_skinny_finish bitwise against finish32 in modes 1 and 2 and per (row, group) in mode 0,
pcd_groupnorm_relu_f16 per (row, group), the fused layer per element; then the per-layer path stage by stage, each stage fed the device's own
previous activations, and the persistent kernel per row and per column against the fp64 network with bounds formed from three fp32 summation
orders when the test runs.  tests/test_latent_cases_cpu.py holds the statements, the bounds and the cases to account.

Every output and slab buffer is pre-filled with NaN and carries a NaN guard region past its end, checked after every launch.  A failure names the
entry point, the case and the first failing row, group and channel; each test prints the worst error / bound it saw per entry point."""
import pytest
import torch

import latent_cases as C
import train_cases as T

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ERR_ARG = -1


def _lib_st():
    from shapegen_amd import _lib
    return _lib, _lib.load(), _lib.stream_ptr()


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


class Out:
    """A NaN-filled device buffer of `shape` with a NaN guard region behind it."""

    def __init__(self, shape, dtype=torch.float32):
        self.shape, self.n = tuple(shape), int(torch.Size(shape).numel())
        self.buf = torch.full((self.n + C.GUARD,), C.NAN, dtype=dtype, device="cuda")

    def ptr(self):
        return self.buf.data_ptr()

    def get(self, what=""):
        """The contents on the host, after checking the guard."""
        host = self.buf.cpu()
        assert C.guard_ok(host, self.n), f"{what}: the guard region behind the buffer was written"
        return host[:self.n].reshape(self.shape)

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


class Judge:
    def __init__(self):
        self.worst = {}

    def within(self, entry, case, err, bound, groups=None, names=None):
        r = C.ratio(err, bound)
        self.worst[entry] = max(self.worst.get(entry, 0.0), float(r.max()))
        bad = C.first_bad(r, groups)
        if bad is not None:
            row, grp, ch = bad
            fam = names[row][grp] if names is not None and grp is not None else "-"
            idx = tuple((r > 1).nonzero()[0].tolist())
            raise AssertionError(f"{entry}, case {case}: {int((r > 1).sum())} elements outside their bound, first at row {row}, group {grp}, channel {ch} "
                                 f"({fam}; index {idx}): error {float(torch.as_tensor(err)[idx]):.4g} > bound {float(torch.as_tensor(bound).expand_as(r)[idx]):.4g}")

    def exact(self, entry, case, got, want):
        got, want = got.cpu(), want.cpu()
        assert got.shape == want.shape and got.dtype == want.dtype, (entry, case, got.shape, want.shape, got.dtype, want.dtype)
        same = (got == want) | (torch.isnan(got) & torch.isnan(want))
        if not bool(same.all()):
            idx = tuple((~same).nonzero()[0].tolist())
            raise AssertionError(f"{entry}, case {case}: {int((~same).sum())} elements differ bitwise, first at {idx}: got {got[idx].item()!r}, want {want[idx].item()!r}")
        self.worst.setdefault(entry + " (bitwise)", 0.0)

    def saturated(self, entry, case, got, want, bound):
        """Beyond 65504 + bound the output is 65504 exactly; never inf."""
        g = got.cpu().double()
        assert not bool(torch.isinf(g).any()), (entry, case, "inf in an fp16 output")
        over = want > T.F16_MAX + bound
        assert bool((g[over] == T.F16_MAX).all()), (entry, case, "not saturated to 65504 at", over.nonzero()[:4].tolist())
        return int(over.sum())

    def report(self):
        for entry, r in self.worst.items():
            print(f"worst error / bound  {entry}: {r:.4f}")


# ------------------------------------------------------------------------------------------------------------ the split-K GEMM
def _gemm(L, lib, st, a1, a2, w, ldw, m, c, dma, f32in=False):
    k1, k2 = a1.shape[1], (a2.shape[1] if a2 is not None else 0)
    out = Out((C.slab_count(k1 + k2, c), m, c))
    L.check(lib.pcd_skinny_config(dma))
    try:
        if f32in:
            L.check(lib.pcd_skinny_gemm_f32in(a1.data_ptr(), k1, w.data_ptr(), ldw, m, c, out.ptr(), st), "skinny_gemm_f32in")
        else:
            L.check(lib.pcd_skinny_gemm_f16(a1.data_ptr(), k1, _p(a2), k2, w.data_ptr(), ldw, m, c, out.ptr(), st), "skinny_gemm_f16")
    finally:
        L.check(lib.pcd_skinny_config(1))
    return out.get(f"gemm {(m, k1, k2, c, ldw, dma)}")


@pytest.mark.parametrize("k1,k2,c", C.GEMM_SHAPES)
def test_skinny_gemm_slab_by_slab(k1, k2, c):
    L, lib, st = _lib_st()
    J = Judge()
    k = k1 + k2
    assert lib.pcd_skinny_slabs(k, c) == C.slab_count(k, c)
    for m in C.gemm_ms(k1, k2, c):
        for kind in ("int", "fam"):
            cs = C.gemm_case(m, k1, k2, c, kind)
            want, bound = C.slab_statement(cs["a"], cs["w"], c)
            a1, a2 = _dev(cs["a1"]), _dev(cs["a2"])
            first = None
            for ldw in (k, k + 8):
                w = _dev(C.pad_ldw(cs["w"], ldw))
                for dma in (1, 0):
                    got = _gemm(L, lib, st, a1, a2, w, ldw, m, c, dma)
                    case = (m, k1, k2, c, kind, f"ldw {ldw}", f"dma {dma}")
                    if kind == "int":
                        J.exact("pcd_skinny_gemm_f16 integers", case, got.double(), want)
                    else:
                        J.within("pcd_skinny_gemm_f16", case, (got.double() - want).abs(), bound)
                    first = got if first is None else first
                    J.exact("pcd_skinny_gemm_f16 forms and strides", case, got, first)
            if k2 == 0 and m in C.GEMM_F32IN_MS and kind == "fam":
                a32 = cs["a"].float() * 1.0003
                a32[0, 0], a32[m - 1, k - 1] = 1e6, -1e6                    # saturate on load, like pcd_f32_to_f16
                a16 = T.sat16(a32)
                want32, bound32 = C.slab_statement(a16, cs["w"], c)
                got = _gemm(L, lib, st, _dev(a32), None, _dev(cs["w"]), k, m, c, 1, f32in=True)
                J.within("pcd_skinny_gemm_f32in", (m, k, c), (got.double() - want32).abs(), bound32)
                J.exact("pcd_skinny_gemm_f32in v. converted input", (m, k, c), got, _gemm(L, lib, st, _dev(a16), None, _dev(cs["w"]), k, m, c, 0))
        if m == 33:                                                         # an inf and a NaN in one row: every other row bitwise as without them
            cs = C.gemm_case(m, k1, k2, c, "fam")
            bad = cs["a1"].clone()
            bad[7, 3], bad[7, k1 - 1] = float("inf"), C.NAN
            w = _dev(cs["w"])
            clean = _gemm(L, lib, st, _dev(cs["a1"]), _dev(cs["a2"]), w, k, m, c, 1)
            got = _gemm(L, lib, st, _dev(bad), _dev(cs["a2"]), w, k, m, c, 1)
            rows = [r for r in range(m) if r != 7]
            J.exact("pcd_skinny_gemm_f16 non-finite row", (m, k1, k2, c), got[:, rows], clean[:, rows])
            assert not bool(torch.isfinite(got[0, 7]).any())
    J.report()


# ------------------------------------------------------------------------------------------------------------ pcd_skinny_finish
def _finish(L, lib, st, slabs, nslabs, m, c, bias, rb, mode, groups, gamma, beta):
    out = Out((m, c), torch.float32 if mode == 2 else torch.float16)
    L.check(lib.pcd_skinny_finish(slabs.data_ptr(), nslabs, m, c, _p(bias), _p(rb), mode, groups, _p(gamma), _p(beta),
                                  None if mode == 2 else out.ptr(), out.ptr() if mode == 2 else None, st), "skinny_finish")
    return out.get(f"finish {(m, c, mode, groups, nslabs)}")


def _finish_operands(c, groups, nslabs, with_bias, kind):
    rows = C.FINISH_ROWS
    base = C.gn_family_case(rows, c, groups, nslabs) if kind == "fam" else C.gn_plain_case(rows, c, groups)
    g = C._gen(c, groups, nslabs, with_bias, kind == "fam")
    bias = 0.5 * torch.randn(c, generator=g) if with_bias else None
    rb = 0.5 * torch.randn(rows, c, generator=g) if with_bias else None
    return base, C.split_into_slabs(base["x"], nslabs, bias, rb, g), bias, rb


@pytest.mark.parametrize("c,groups", C.FINISH_SHAPES)
def test_skinny_finish_by_row_and_group(c, groups):
    L, lib, st = _lib_st()
    J = Judge()
    m = C.FINISH_ROWS
    nsat = 0
    for nslabs in C.FINISH_NSLABS:
        for with_bias in (False, True):
            for kind in ("fam", "plain"):
                base, slabs, bias, rb = _finish_operands(c, groups, nslabs, with_bias, kind)
                gamma, beta = _dev(base["gamma"]), _dev(base["beta"])
                case = (c, groups, f"{nslabs} slabs", "bias" if with_bias else "no bias", kind)
                hot = slabs.clone()
                hot[0, 0, 0], hot[nslabs - 1, m - 1, c - 1] = 1e5, -1e5                  # past 65504 in mode 1
                hot, _, _ = C.nonfinite_rows(hot.reshape(nslabs * m, c), groups, row=1)   # and an inf and a NaN in slab 0, row 1
                hot = hot.reshape(nslabs, m, c)
                for sl in (slabs, hot):
                    dsl = Out(sl.shape)
                    dsl.buf[:sl.numel()] = sl.reshape(-1).cuda()
                    for mode in (2, 1):
                        got = _finish(L, lib, st, dsl.buf, nslabs, m, c, _dev(bias), _dev(rb), mode, groups, None, None)
                        J.exact(f"pcd_skinny_finish mode {mode} v. finish32", case, got, C.finish32(sl, bias, rb, mode))
                    dsl.get("finish's slabs")
                assert float(C.finish32(hot, bias, rb, 1)[0, 0]) == T.F16_MAX
                if (c, groups) == (12, 1):
                    continue
                dsl = _dev(slabs)
                got = _finish(L, lib, st, dsl, nslabs, m, c, _dev(bias), _dev(rb), 0, groups, gamma, beta)
                pre = C.finish32(slabs, bias, rb, 0, pre=True)
                want, bound = C.gn_relu_statement(pre, base["gamma"], base["beta"], groups, C.finish_gn_chain(c // groups))
                J.within("pcd_skinny_finish mode 0", case, C.out16_error(got, want), bound, groups, base.get("names"))
                nsat += J.saturated("pcd_skinny_finish mode 0", case, got, want, bound)
                if nslabs == 3 and kind == "fam":                                        # an inf and a NaN in one (row, group)
                    bad, row, grp = C.nonfinite_rows(slabs[1], groups)
                    sb = slabs.clone()
                    sb[1] = bad
                    gb = _finish(L, lib, st, _dev(sb), nslabs, m, c, _dev(bias), _dev(rb), 0, groups, gamma, beta)
                    keep = torch.ones(m, groups, dtype=torch.bool)
                    keep[row, grp] = False
                    keep = keep.repeat_interleave(c // groups, 1)
                    J.exact("pcd_skinny_finish mode 0 non-finite group", case, gb[keep], got[keep])
    assert nsat > 0 or (c, groups) == (12, 1)
    J.report()


# ------------------------------------------------------------------------------------------------------------ pcd_groupnorm_relu_f16
def test_groupnorm_relu_by_row_and_group():
    L, lib, st = _lib_st()
    J = Judge()
    nsat = 0
    for groups in C.GN_GROUPS:
        for gsz in C.GN_GSZ:
            c, rows = groups * gsz, C.GN_ROWS
            for base in (C.gn_family_case(rows, c, groups, groups), C.gn_plain_case(rows, c, groups)):
                gamma, beta = _dev(base["gamma"]), _dev(base["beta"])

                def run(x):
                    out = Out((rows, c), torch.float16)
                    L.check(lib.pcd_groupnorm_relu_f16(x.data_ptr(), rows, c, groups, gamma.data_ptr(), beta.data_ptr(), out.ptr(), st), "groupnorm_relu_f16")
                    return out.get(f"groupnorm_relu {(rows, c, groups)}")
                got = run(_dev(base["x"]))
                want, bound = C.gn_relu_statement(base["x"], base["gamma"], base["beta"], groups, C.gn_chain(gsz))
                case = (rows, c, groups, "fam" if "names" in base else "plain")
                J.within("pcd_groupnorm_relu_f16", case, C.out16_error(got, want), bound, groups, base.get("names"))
                nsat += J.saturated("pcd_groupnorm_relu_f16", case, got, want, bound)
                bad, row, grp = C.nonfinite_rows(base["x"], groups, row=1, group=groups // 2)
                gb = run(_dev(bad))
                keep = torch.ones(rows, groups, dtype=torch.bool)
                keep[row, grp] = False
                keep = keep.repeat_interleave(gsz, 1)
                J.exact("pcd_groupnorm_relu_f16 non-finite group", case, gb[keep], got[keep])
    assert nsat > 0
    J.report()


# ------------------------------------------------------------------------------------------------------------ the fused layer
def _fused(L, lib, st, cs, m, c, mode, groups, ldw=None, f32in=False, row_bias="case"):
    k1, k2 = cs["a1"].shape[1], (cs["a2"].shape[1] if cs["a2"] is not None else 0)
    ldw = ldw or k1 + k2
    w = _dev(C.pad_ldw(cs["w"], ldw))
    rb = _dev(cs["row_bias"] if isinstance(row_bias, str) else row_bias)
    out = Out((m, c), torch.float32 if mode == 2 else torch.float16)
    gamma, beta = (_dev(cs["gamma"]), _dev(cs["beta"])) if mode == 0 else (None, None)
    bias, a1, a2 = _dev(cs["bias"]), _dev(cs["a1"].float() if f32in else cs["a1"]), _dev(cs["a2"])      # held until the launch has been waited for
    tail = (w.data_ptr(), ldw, m, c, _p(bias), _p(rb), mode, groups, _p(gamma), _p(beta), None if mode == 2 else out.ptr(), out.ptr() if mode == 2 else None, st)
    if f32in:
        L.check(lib.pcd_skinny_fused_f32in(a1.data_ptr(), k1, *tail), "skinny_fused_f32in")
    else:
        L.check(lib.pcd_skinny_fused(a1.data_ptr(), k1, _p(a2), k2, *tail), "skinny_fused")
    return out.get(f"fused {(m, k1, k2, c, mode, groups, ldw)}")


@pytest.mark.parametrize("k1,k2,c,groups", C.FUSED_SHAPES)
def test_skinny_fused_element_by_element(k1, k2, c, groups):
    L, lib, st = _lib_st()
    J = Judge()
    assert lib.pcd_skinny_fused_supported(k1 + k2, c, 0, groups) == 1
    nsat = 0
    for m in C.FUSED_MS:
        for kind in ("int", "rowbias", "groupbias"):
            cs = C.fused_case(m, k1, k2, c, groups, kind)
            want, bound, _, _ = C.fused_statement(cs["a"], cs["w"], cs["bias"], cs["row_bias"], 0, groups, cs["gamma"], cs["beta"], exact_z=kind != "groupbias")
            case = (m, k1, k2, c, groups, kind)
            got = _fused(L, lib, st, cs, m, c, 0, groups)
            J.within(f"pcd_skinny_fused mode 0 {kind}", case, C.out16_error(got, want), bound, groups, cs["names"])
            nsat += J.saturated("pcd_skinny_fused mode 0", case, got, want, bound)
            J.exact("pcd_skinny_fused ldw = k + 8", case, _fused(L, lib, st, cs, m, c, 0, groups, ldw=k1 + k2 + 8), got)
            if k2 == 0:
                J.exact("pcd_skinny_fused_f32in", case, _fused(L, lib, st, cs, m, c, 0, groups, f32in=True), got)
            if kind == "rowbias" and m == 33:                               # an inf and a NaN in one (row, group) of the row bias
                bad, row, grp = C.nonfinite_rows(cs["row_bias"], groups, row=m - 1, group=groups - 1)
                gb = _fused(L, lib, st, cs, m, c, 0, groups, row_bias=bad)
                keep = torch.ones(m, groups, dtype=torch.bool)
                keep[row, grp] = False
                keep = keep.repeat_interleave(c // groups, 1)
                J.exact("pcd_skinny_fused non-finite group", case, gb[keep], got[keep])
    assert nsat > 0
    J.report()


def test_skinny_fused_plain_modes():
    L, lib, st = _lib_st()
    J = Judge()
    k1, k2, c = C.FUSED_PLAIN
    for m in C.FUSED_MS:
        for mode in (1, 2):
            cs = C.fused_case(m, k1, k2, c, 8, "int")
            want, _, _, _ = C.fused_statement(cs["a"], cs["w"], cs["bias"], cs["row_bias"], mode, 8, exact_z=True)
            got = _fused(L, lib, st, cs, m, c, mode, 8)
            J.exact(f"pcd_skinny_fused mode {mode} integers", (m, mode), got.double(), want.clamp(max=T.F16_MAX) if mode == 1 else want)
            cs = dict(C.fused_case(m, k1, k2, c, 8, "groupbias"))
            cs["bias"] = cs["bias"].clone()
            cs["bias"][5] = 1e5                                             # past 65504
            want, bound, _, _ = C.fused_statement(cs["a"], cs["w"], cs["bias"], cs["row_bias"], mode, 8)
            got = _fused(L, lib, st, cs, m, c, mode, 8)
            J.within(f"pcd_skinny_fused mode {mode}", (m, mode), C.out16_error(got, want) if mode == 1 else (got.double() - want).abs(), bound)
            if mode == 1:
                assert J.saturated("pcd_skinny_fused mode 1", (m, mode), got, want, bound) == m
            J.exact(f"pcd_skinny_fused_f32in mode {mode}", (m, mode), _fused(L, lib, st, cs, m, c, mode, 8, f32in=True), got)
    J.report()


# ------------------------------------------------------------------------------------------------------------ rejections
def test_rejections_return_err_arg_and_write_nothing():
    L, lib, st = _lib_st()
    a = torch.ones(257, 128, dtype=torch.float16, device="cuda")
    a32 = torch.ones(257, 128, device="cuda")
    w = torch.ones(128, 136, dtype=torch.float16, device="cuda")
    vec = torch.ones(128, device="cuda")
    slabs, o16, o32 = Out((2, 257, 128)), Out((257, 128), torch.float16), Out((257, 128))
    gemm = lambda k1, ldw, m: lib.pcd_skinny_gemm_f16(a.data_ptr(), k1, None, 0, w.data_ptr(), ldw, m, 128, slabs.ptr(), st)
    fused = lambda k1, ldw, m, c=128, mode=0, groups=8: lib.pcd_skinny_fused(a.data_ptr(), k1, None, 0, w.data_ptr(), ldw, m, c, vec.data_ptr(), None, mode, groups,
                                                                             vec.data_ptr(), vec.data_ptr(), o16.ptr(), o32.ptr(), st)
    finish = lambda mode, c, groups: lib.pcd_skinny_finish(a32.data_ptr(), 2, 4, c, vec.data_ptr(), None, mode, groups, vec.data_ptr(), vec.data_ptr(), o16.ptr(), o32.ptr(), st)
    calls = {"gemm m = 0": gemm(128, 128, 0), "gemm m = 257": gemm(128, 128, 257), "gemm k % 64": gemm(96, 128, 4), "gemm ldw % 8": gemm(128, 132, 4),
             "gemm ldw < k": gemm(128, 120, 4),
             "gemm_f32in m = 257": lib.pcd_skinny_gemm_f32in(a32.data_ptr(), 128, w.data_ptr(), 128, 257, 128, slabs.ptr(), st),
             "fused m = 0": fused(128, 128, 0), "fused m = 257": fused(128, 128, 257), "fused k % 64": fused(96, 128, 4), "fused ldw % 8": fused(128, 132, 4),
             "fused ldw < k": fused(128, 120, 4), "fused gsz 8": fused(128, 128, 4, 64, 0, 8), "fused mode 1, c % 32": fused(128, 128, 4, 48, 1, 8),
             "fused groups 3": fused(128, 128, 4, 128, 0, 3),
             "fused_f32in m = 257": lib.pcd_skinny_fused_f32in(a32.data_ptr(), 128, w.data_ptr(), 128, 257, 128, vec.data_ptr(), None, 0, 8, vec.data_ptr(), vec.data_ptr(),
                                                               o16.ptr(), None, st),
             "finish mode 3": finish(3, 128, 8), "finish c % groups": finish(0, 128, 3), "finish m = 0": lib.pcd_skinny_finish(a32.data_ptr(), 2, 0, 128, None, None, 2, 8,
                                                                                                                              None, None, None, o32.ptr(), st)}
    assert lib.pcd_skinny_fused_supported(128, 64, 0, 8) == 0 and lib.pcd_skinny_fused_supported(128, 48, 1, 8) == 0
    torch.cuda.synchronize()
    for name, rc in calls.items():
        assert rc == ERR_ARG, (name, rc)
    assert slabs.untouched() and o16.untouched() and o32.untouched()


# ------------------------------------------------------------------------------------------------------------ the per-layer path, stage by stage
@pytest.fixture(scope="module")
def net():
    from helpers import latent_sd
    from shapegen_amd import packing
    from shapegen_amd.networks import SimpleLatentUNetPointNet
    sd = {k[len("model."):]: v for k, v in latent_sd().items() if k.startswith("model.")}
    model = SimpleLatentUNetPointNet(256)
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda").eval()
    lin, gn, _ = packing.pack_latent_unet(sd, "")
    return model, C.pack_layers(lin, gn)


@pytest.mark.parametrize("batch", [1, 33, 256])
def test_per_layer_path_stage_by_stage(net, batch):
    """The entry points in csrc/latent.hip's order on this test's own buffers; every stage against the fp64 statement of that stage fed the device's
    own previous activations; then pcd_latent_forward through the handle is bitwise that composition."""
    model, layers = net
    L, lib, st = _lib_st()
    J = Judge()
    B = batch
    z = (torch.randn(256, 256, generator=torch.Generator().manual_seed(31)) * 1.2)[:B].contiguous()
    dz = _dev(z)
    trow = model.time_bias(torch.tensor([0.73]).cuda())[0].contiguous()
    trow_h = trow.cpu()
    dw = [dict((n, _dev(t)) for n, t in Lr.items()) for Lr in layers]
    acts_d, acts_h = {}, {-1: T.sat16(z)}
    for i, Lr in enumerate(layers):
        K, c, k2, mode = C.LAT_K[i], C.LAT_C[i], C.LAT_K2[i], C.LAT_MODE[i]
        a1h, a2h = C.layer_inputs(i, acts_h)
        a1d, a2d = (dz, None) if i == 0 else C.layer_inputs(i, acts_d)
        bias_h, bias_d = (trow_h, trow) if i == 0 else (Lr["b"], dw[i]["b"])
        gam_h, bet_h = Lr.get("gamma"), Lr.get("beta")
        gam_d, bet_d = dw[i].get("gamma"), dw[i].get("beta")
        out = Out((B, c), torch.float32 if mode == 2 else torch.float16)
        o16, o32 = (None, out.ptr()) if mode == 2 else (out.ptr(), None)
        ah = torch.cat([a1h, a2h], 1) if a2h is not None else a1h
        case = (B, f"layer {i}", K, c)
        if i == 0 or lib.pcd_skinny_fused_supported(K, c, mode, 8):
            assert C.fused_supported(K, c, mode, 8)
            if i == 0:
                L.check(lib.pcd_skinny_fused_f32in(dz.data_ptr(), K, dw[i]["w"].data_ptr(), K, B, c, bias_d.data_ptr(), None, 0, 8, gam_d.data_ptr(), bet_d.data_ptr(),
                                                   o16, None, st), "skinny_fused_f32in")
            else:
                L.check(lib.pcd_skinny_fused(a1d.data_ptr(), K - k2, _p(a2d), k2, dw[i]["w"].data_ptr(), K, B, c, bias_d.data_ptr(), None, mode, 8, _p(gam_d), _p(bet_d),
                                             o16, o32, st), "skinny_fused")
            got = out.get(str(case))
            want, bound, zpre, d = C.fused_statement(ah, Lr["w"], bias_h, None, mode, 8, gam_h, bet_h)
            if mode == 0:
                assert C.first_order_ok(zpre, 8, d) <= 0.05, case
            J.within(f"layer {i} (fused, mode {mode})", case, (got.double() - want).abs() if mode == 2 else C.out16_error(got, want), bound, 8 if mode == 0 else None)
        else:
            ns = C.slab_count(K, c)
            slabs = Out((ns, B, c))
            L.check(lib.pcd_skinny_gemm_f16(a1d.data_ptr(), K - k2, _p(a2d), k2, dw[i]["w"].data_ptr(), K, B, c, slabs.ptr(), st), "skinny_gemm_f16")
            L.check(lib.pcd_skinny_finish(slabs.ptr(), ns, B, c, bias_d.data_ptr(), None, mode, 8, _p(gam_d), _p(bet_d), o16, o32, st), "skinny_finish")
            sl = slabs.get(str(case))
            want, bound = C.slab_statement(ah, Lr["w"], c)
            J.within(f"layer {i} slabs", case, (sl.double() - want).abs(), bound)
            got = out.get(str(case))
            pre = C.finish32(sl, bias_h, None, 0, pre=True)
            want, bound = C.gn_relu_statement(pre, gam_h, bet_h, 8, C.finish_gn_chain(c // 8))
            J.within(f"layer {i} finish", case, C.out16_error(got, want), bound, 8)
        acts_d[i], acts_h[i] = out.buf[:out.n].reshape(B, c), got
    eps = model.forward_with_bias(dz, trow, 0)
    J.exact("pcd_latent_forward v. the composition", (B,), eps, acts_h[11])
    if B >= 31:                 # and the composition is the network: inside the bounds of the whole-network statement on these rows
        want, figs = C.network_figures(layers, trow_h.unsqueeze(0), None, z, 0)
        bounds = C.bounds_from(figs)["eps"]
        for f, v in C.row_col_errors(acts_h[11], want["eps"]).items():
            assert v <= bounds[f], (B, f, v, bounds[f])
    J.report()


# ------------------------------------------------------------------------------------------------------------ the persistent kernel
_ROW_BOUNDS = {}


def _row_bounds(layers, tb, rates, nsteps):
    """Row bounds from the 64-row sample (tests/test_latent_cases_cpu.py's part 4), for the time rows of this device."""
    key = (nsteps, tb.numpy().tobytes())
    if key not in _ROW_BOUNDS:
        _, figs = C.network_figures(layers, tb, rates, C.latent_input(64), nsteps)
        _ROW_BOUNDS[key] = C.bounds_from(figs)
    return _ROW_BOUNDS[key]


def _judge_rows_cols(layers, tb, rates, z, nsteps, got, what):
    """got {name: tensor} per row (bounds from the 64-row sample) and, from 31 rows up, per column (bounds from these rows)."""
    rowb = _row_bounds(layers, tb, rates, nsteps)
    want, figs = C.network_figures(layers, tb, rates, z, nsteps)
    colb = C.bounds_from(figs)
    worst = {}
    for name, g in got.items():
        assert bool(torch.isfinite(g).all()), (what, name)
        for f, v in C.row_col_errors(g.cpu(), want[name]).items():
            b = rowb[name][f] if f.startswith("row") else colb[name][f]
            if f.startswith("row") or z.shape[0] >= 31:
                worst[f"{name} {f}"] = v / b
                assert v <= b, (what, name, f, v, b)
    print(f"{what}: fraction of the bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_persistent_forward_by_row_and_column(net):
    model, layers = net
    if not model.persist_supported(64):
        pytest.skip("needs a 256-CU device")
    tb = model.time_bias(torch.tensor([0.73]).cuda()).contiguous()
    outs = {}
    for B in (1, 31, 32, 33, 64):
        z = C.latent_input(B)
        out = Out((B, 256))
        model.forward_persist(_dev(z), tb[0], out=out.buf[:out.n].reshape(B, 256))
        model.check_persist_status()
        outs[B] = out.get(f"forward_persist B = {B}")
        _judge_rows_cols(layers, tb.cpu(), None, z, 0, {"eps": outs[B]}, f"forward_persist B = {B}")
    assert torch.equal(outs[64][:32], outs[32])                       # a stream's rows do not depend on the other stream


@pytest.mark.parametrize("nsteps", [1, 4])
def test_persistent_ddim_by_row_and_column(net, nsteps):
    """4 steps: the first launch in which a step reads a buffer set that was re-poisoned inside the same launch."""
    model, layers = net
    if not model.persist_supported(64):
        pytest.skip("needs a 256-CU device")
    ts, rates = C.ddim_tables(nsteps)
    tb = model.time_bias(ts.cuda()).contiguous()
    drates = _dev(rates)
    for B in (32, 45):
        z = C.latent_input(B)
        zbuf, x0 = Out((B, 256)), Out((B, 256))
        zbuf.buf[:zbuf.n] = z.reshape(-1).cuda()
        counter = torch.zeros(2, dtype=torch.int32, device="cuda")
        model.ddim_steps_persist(zbuf.buf[:zbuf.n].reshape(B, 256), x0.buf[:x0.n].reshape(B, 256), tb, drates, counter, nsteps)
        model.check_persist_status()
        assert counter.tolist() == [nsteps, nsteps - 1]
        got = {"z": zbuf.get("ddim z"), "x0": x0.get("ddim x0")}
        _judge_rows_cols(layers, tb.cpu(), rates, z, nsteps, got, f"ddim_steps_persist {nsteps} steps, B = {B}")
