"""The kernels of csrc/train.hip through their C entry points, every launch judged against the fp64 statements of tests/train_cases.py: column
by column (element by element for the fp16 outputs) with the bounds derived there, never a whole-tensor figure, at the shapes where the
launch geometry changes (fewer rows than row lanes, a one-row last chunk, one 8-column group, ragged groups and blocks, widths that are
no multiple of 8) and on the column families a reduction or a normalisation can get wrong.  tests/test_train_cases_cpu.py holds the
statements, the margin construction (no element near a ReLU threshold: nothing is excluded from any comparison) and the bounds to account.

Each stage is fed its predecessor's own fp32 output, so a launch answers for its own arithmetic only.  Outputs a kernel must fill are
pre-filled with NaN.  A failure names the entry point, the shape, the element, its column family, the error and the bound; each test
prints the worst error / bound it saw per entry point."""
import pytest
import torch

import train_cases as T

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lib_st():
    from shapegen_amd import _lib
    return _lib, _lib.load(), _lib.stream_ptr()


def _dev(t):
    return t.cuda().contiguous()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


class Judge:
    """Collects the worst error / bound per entry point; `within` asserts one output of one launch."""

    def __init__(self):
        self.worst = {}

    def within(self, entry, shape, got, want, bound, names=None):
        got, want = got.detach().cpu().double(), torch.as_tensor(want, dtype=torch.float64)
        assert got.shape == want.shape, (entry, shape, got.shape, want.shape)
        bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(want)
        err = torch.nan_to_num((got - want).abs(), nan=float("inf"))
        ratio = torch.where(err <= bound, torch.where(bound > 0, err / bound, torch.zeros_like(err)), torch.where(bound > 0, err / bound, torch.full_like(err, float("inf"))))
        self.worst[entry] = max(self.worst.get(entry, 0.0), float(ratio.max()))
        bad = (err > bound).nonzero()
        if len(bad):
            lines = []
            for idx in bad[:8].tolist():
                col = idx[-1] if idx else 0
                fam = names[col] if names is not None else "-"
                i = tuple(idx)
                lines.append(f"element {i} (column {col}, {fam}): got {float(got[i])!r}, want {float(want[i])!r}, error {float(err[i]):.3g} > bound {float(bound[i]):.3g}")
            raise AssertionError(f"{entry}, shape {shape}: {len(bad)} elements outside their bound:\n  " + "\n  ".join(lines))

    def exact(self, entry, shape, got, want):
        got, want = got.detach().cpu(), want.cpu()
        assert got.dtype == want.dtype and got.shape == want.shape, (entry, shape, got.dtype, want.dtype, got.shape, want.shape)
        same = (got == want) | (torch.isnan(got) & torch.isnan(want)) if got.is_floating_point() else got == want
        if not bool(same.all()):
            idx = tuple((~same).nonzero()[0].tolist())
            raise AssertionError(f"{entry}, shape {shape}: {int((~same).sum())} elements differ, first {idx}: got {got[idx].item()!r}, want {want[idx].item()!r}")
        self.worst.setdefault(entry + " (exact)", 0.0)

    def report(self):
        for entry, r in self.worst.items():
            print(f"worst error / bound  {entry}: {r:.4f}")


def _saturated_exactly(entry, shape, got, want, bound, names):
    """Where the statement is beyond +-65504 by more than its bound the kernel must give +-65504 exactly, and never inf."""
    g = got.detach().cpu().float()
    assert bool(torch.isfinite(g).all()), (entry, shape, "non-finite output")
    over = want.abs() > T.F16_MAX + bound
    bad = over & (g.double() != torch.sign(want) * T.F16_MAX)
    assert not bool(bad.any()), (entry, shape, "not saturated to +-65504 at", bad.nonzero()[:4].tolist(), [names[j] for j in bad.nonzero()[:4, -1].tolist()])
    return int(over.sum())


# ------------------------------------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("c", T.BN_CS)
def test_bn_batch_stats_by_column(c):
    L, lib, st = _lib_st()
    J = Judge()
    for k in T.bn_cases(c):
        m, names = k["m"], k["names"]
        z = _dev(k["z"])
        scratch = _nan(2 * c)
        for running in (True, False):
            outs = []
            for rep in range(2):                      # workspace-reduced: two runs agree bitwise
                mean, var = _nan(c), _nan(c)
                rm, rv = _dev(k["running_mean"]), _dev(k["running_var"])
                L.check(lib.pcd_bn_batch_stats(z.data_ptr(), m, c, 0.1, mean.data_ptr(), var.data_ptr(), rm.data_ptr() if running else None,
                                               rv.data_ptr() if running else None, scratch.data_ptr(), st), "bn_batch_stats")
                outs.append((mean, var, rm, rv))
            torch.cuda.synchronize()
            for a, b in zip(*outs):
                J.exact("pcd_bn_batch_stats twice", (m, c), a, b)
            mean, var, rm, rv = outs[0]
            s = T.bn_stats_statement(k["z"], k["running_mean"], k["running_var"])
            shape = (m, c, "running" if running else "running NULL")
            J.within("pcd_bn_batch_stats mean", shape, mean, s["mean"], s["mean_bound"], names)
            J.within("pcd_bn_batch_stats var", shape, var, s["var"], s["var_bound"], names)
            if running:
                J.within("pcd_bn_batch_stats running_mean", shape, rm, s["running_mean"], s["running_mean_bound"], names)
                J.within("pcd_bn_batch_stats running_var", shape, rv, s["running_var"], s["running_var_bound"], names)
            else:
                J.exact("pcd_bn_batch_stats running NULL", shape, rm, k["running_mean"])
    J.report()


def test_bn_batch_stats_rejects_ragged_widths():
    L, lib, st = _lib_st()
    z, o = torch.zeros(4, 12, device="cuda"), _nan(24)
    assert lib.pcd_bn_batch_stats(z.data_ptr(), 4, 12, 0.1, o.data_ptr(), o.data_ptr(), None, None, o.data_ptr(), st) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all())


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("c", T.BN_CS + T.BN_CS_RAGGED)
def test_bn_apply_by_element(c, relu):
    L, lib, st = _lib_st()
    J = Judge()
    saturated = 0
    for k in T.bn_cases(c):
        m, names = k["m"], k["names"]
        z, mean, var, gamma, beta = (_dev(k[n]) for n in ("z", "mean", "var", "gamma", "beta"))
        out = _nan(m, c, dtype=torch.float16)
        L.check(lib.pcd_bn_apply_f16(z.data_ptr(), m, c, mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, relu,
                                     out.data_ptr(), st), "bn_apply")
        torch.cuda.synchronize()
        want, bound = T.bn_apply_statement(k["z"], k["mean"], k["var"], k["gamma"], k["beta"], relu)
        J.within("pcd_bn_apply_f16", (m, c, f"relu {relu}"), out, want.clamp(-T.F16_MAX, T.F16_MAX), bound, names)
        saturated += _saturated_exactly("pcd_bn_apply_f16", (m, c), out, want, bound, names)
    assert saturated > 0 or "saturate" not in sum((k["names"] for k in T.bn_cases(c)), [])
    J.report()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("c", T.BN_CS + T.BN_CS_RAGGED)
def test_bn_backward_by_column_and_element(c, relu):
    L, lib, st = _lib_st()
    J = Judge()
    for k in T.bn_cases(c):
        m, names = k["m"], k["names"]
        z, mean, var, gamma, beta, da = (_dev(k[n]) for n in ("z", "mean", "var", "gamma", "beta", "da"))
        outs = []
        for rep in range(2):
            dg, db, dz = _nan(c), _nan(c), _nan(m, c, dtype=torch.float16)
            L.check(lib.pcd_bn_backward_f16(da.data_ptr(), z.data_ptr(), m, c, mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                            1e-5, relu, dg.data_ptr(), db.data_ptr(), dz.data_ptr(), st), "bn_backward")
            outs.append((dg, db, dz))
        torch.cuda.synchronize()
        for a, b in zip(*outs):
            J.exact("pcd_bn_backward_f16 twice", (m, c), a, b)
        dg, db, dz = outs[0]
        shape = (m, c, f"relu {relu}")
        bw = T.bn_backward_statement(k["da"], k["z"], k["mean"], k["var"], k["gamma"], k["beta"], relu)
        J.within("pcd_bn_backward_f16 dbeta", shape, db, bw["dbeta"], bw["dbeta_bound"], names)
        J.within("pcd_bn_backward_f16 dgamma", shape, dg, bw["dgamma"], bw["dgamma_bound"], names)
        want, bound = T.bn_dz_statement(bw, k["gamma"], dg.cpu(), db.cpu(), m)          # from the entry point's own dgamma, dbeta
        J.within("pcd_bn_backward_f16 dz", shape, dz, want.clamp(-T.F16_MAX, T.F16_MAX), bound, names)
        _saturated_exactly("pcd_bn_backward_f16 dz", (m, c), dz, want, bound, names)
    J.report()


# ------------------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("c", T.BN_CS + T.BN_CS_RAGGED)
def test_colsum_by_column(c):
    L, lib, st = _lib_st()
    J = Judge()
    for groups in T.COLSUM_GROUPS:
        for rpg in T.COLSUM_ROWS:
            x, names = T.colsum_case(rpg, groups, c)
            xd = _dev(x)
            o1, o2 = _nan(groups, c), _nan(groups, c)
            L.check(lib.pcd_colsum_f16(xd.data_ptr(), rpg, groups, c, o1.data_ptr(), st), "colsum")
            L.check(lib.pcd_colsum_f16(xd.data_ptr(), rpg, groups, c, o2.data_ptr(), st), "colsum")
            torch.cuda.synchronize()
            want, bound = T.colsum_statement(x, rpg, groups)
            J.within("pcd_colsum_f16", (rpg, groups, c), o1, want, bound, names)
            J.exact("pcd_colsum_f16 twice", (rpg, groups, c), o1, o2)
    J.report()


@pytest.mark.parametrize("k", T.VEC3_KS + T.BN_CS_RAGGED)
def test_vec3_outer_by_column(k):
    L, lib, st = _lib_st()
    J = Judge()
    for m in T.BN_MS:
        mat, vec, names = T.vec3_case(m, k)
        md, vd = _dev(mat), _dev(vec)
        s = T.vec3_outer_statement(mat, vec)
        outs = []
        for with_vsum in (True, True, False):
            out, vsum = _nan(3, k), _nan(3)
            L.check(lib.pcd_vec3_outer(md.data_ptr(), vd.data_ptr(), m, k, out.data_ptr(), vsum.data_ptr() if with_vsum else None, st), "vec3_outer")
            outs.append((out, vsum))
        torch.cuda.synchronize()
        J.within("pcd_vec3_outer out", (m, k), outs[0][0], s["out"], s["out_bound"], names)
        J.within("pcd_vec3_outer vsum", (m, k), outs[0][1], s["vsum"], s["vsum_bound"])
        J.exact("pcd_vec3_outer twice", (m, k), outs[0][0], outs[1][0])
        J.exact("pcd_vec3_outer twice", (m, k), outs[0][1], outs[1][1])
        J.exact("pcd_vec3_outer vsum NULL", (m, k), outs[2][0], outs[0][0])
        assert bool(torch.isnan(outs[2][1]).all())
    J.report()


# ------------------------------------------------------------------------------------------------------------ exact kernels
@pytest.mark.parametrize("batch", T.COLMAX_BATCHES)
def test_colmax_argmax_and_scatter_exactly(batch):
    L, lib, st = _lib_st()
    J = Judge()
    for n in T.COLMAX_NS:
        for c in T.COLMAX_CS:
            a, dg = T.colmax_case(batch, n, c)
            ad, dgd = _dev(a), _dev(dg)
            mx, arg = _nan(batch, c), torch.full((batch, c), -7, dtype=torch.int32, device="cuda")
            L.check(lib.pcd_colmax_argmax_f16(ad.data_ptr(), batch, n, c, mx.data_ptr(), arg.data_ptr(), st), "colmax")
            want_mx, want_arg = T.colmax_statement(a, batch, n)
            argd = _dev(want_arg)                        # the scatter from the statement's indices: its own stage, and always in range
            da = _nan(batch * n, c, dtype=torch.float16)
            L.check(lib.pcd_maxpool_backward_f16(dgd.data_ptr(), argd.data_ptr(), batch, n, c, da.data_ptr(), st), "maxpool_backward")
            torch.cuda.synchronize()
            J.exact("pcd_colmax_argmax_f16 max", (batch, n, c), mx, want_mx)
            J.exact("pcd_colmax_argmax_f16 argmax", (batch, n, c), arg, want_arg)
            J.exact("pcd_maxpool_backward_f16", (batch, n, c), da, T.maxpool_backward_statement(dg, want_arg, batch, n))
    J.report()


def test_transpose_exactly():
    L, lib, st = _lib_st()
    J = Judge()
    g = torch.Generator().manual_seed(41)
    for rows in T.TRANSPOSE_SIZES:
        for cols in T.TRANSPOSE_SIZES:
            x = torch.randn(rows, cols, generator=g).half()
            xd, dst = _dev(x), _nan(cols, rows, dtype=torch.float16)
            L.check(lib.pcd_transpose_f16(xd.data_ptr(), rows, cols, dst.data_ptr(), st), "transpose")
            torch.cuda.synchronize()
            J.exact("pcd_transpose_f16", (rows, cols), dst, x.t().contiguous())
    J.report()


def test_relu_and_mask_scale_exactly():
    L, lib, st = _lib_st()
    J = Judge()
    g = torch.Generator().manual_seed(43)
    for n in (1, 255, 257):
        x, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
        x[::5] = 0.0
        mask = (torch.rand(n, generator=g) > 0.3).float()
        xd, dyd, md = _dev(x), _dev(dy), _dev(mask)
        y, dx, ms = _nan(n), _nan(n), _nan(n)
        L.check(lib.pcd_relu_f32(xd.data_ptr(), n, y.data_ptr(), st), "relu")
        L.check(lib.pcd_relu_backward_f32(xd.data_ptr(), dyd.data_ptr(), n, dx.data_ptr(), st), "relu_backward")
        L.check(lib.pcd_mask_scale_f32(xd.data_ptr(), md.data_ptr(), 1.25, n, ms.data_ptr(), st), "mask_scale")
        torch.cuda.synchronize()
        J.exact("pcd_relu_f32", n, y, x.clamp_min(0))
        J.exact("pcd_relu_backward_f32", n, dx, torch.where(x > 0, dy, torch.zeros(n)))
        J.exact("pcd_mask_scale_f32", n, ms, x * mask * torch.tensor(1.25))
    J.report()


# ------------------------------------------------------------------------------------------------------------ small fp32 products
def _padded(t, pad):
    """t in a buffer whose rows are `pad` floats longer; the padding holds NaN (a kernel that reads it spoils its result)."""
    buf = _nan(t.shape[0], t.shape[1] + pad)
    buf[:, :t.shape[1]] = t.cuda()
    return buf


@pytest.mark.parametrize("trans_a", [0, 1])
@pytest.mark.parametrize("m", T.MATMUL_MS)
def test_matmul_f32_by_element(m, trans_a):
    L, lib, st = _lib_st()
    J = Judge()
    for k in T.MATMUL_KS:
        for n in T.MATMUL_NS:
            case = T.matmul_case(m, k, n)
            a = case["a"].t().contiguous() if trans_a else case["a"]
            for trans_b in (0, 1):
                b = case["b"].t().contiguous() if trans_b else case["b"]
                route = T.matmul_route(m, trans_a, trans_b)
                for pad in (0, 3):
                    ad, bd = _padded(a, pad), _padded(b, pad)
                    for accumulate in (0, 1):
                        for bias in (None, case["bias"]):
                            c_old = case["c_old"] if accumulate else None
                            want, mag = T.matmul_statement(a, b, trans_a, trans_b, bias, c_old)
                            bound = T.sum_bound(T.matmul_chain(route, k), mag)
                            biasd = _dev(bias) if bias is not None else None
                            outs = []
                            for rep in range(2 if route == "nn" else 1):
                                cd = _padded(case["c_old"] if accumulate else torch.full((m, n), NAN), pad)
                                L.check(lib.pcd_matmul_f32(ad.data_ptr(), a.shape[1] + pad, trans_a, bd.data_ptr(), b.shape[1] + pad, trans_b, m, n, k,
                                                           biasd.data_ptr() if bias is not None else None, accumulate, cd.data_ptr(), n + pad, st), "matmul_f32")
                                outs.append(cd)
                            torch.cuda.synchronize()
                            shape = (m, k, n, f"trans_a {trans_a} trans_b {trans_b} pad {pad} accumulate {accumulate} bias {bias is not None}")
                            J.within(f"pcd_matmul_f32 {route}", shape, outs[0][:, :n], want, bound)
                            assert bool(torch.isnan(outs[0][:, n:]).all()), ("pcd_matmul_f32 wrote into the padding of C", shape)
                            if route == "nn":
                                J.exact("pcd_matmul_f32 nn twice", shape, outs[0][:, :n], outs[1][:, :n])
    J.report()


@pytest.mark.parametrize("n", T.L1_NS)
def test_l1_loss(n):
    L, lib, st = _lib_st()
    J = Judge()
    pred, target = T.l1_case(n)
    pd, td = _dev(pred), _dev(target)
    for scale in (8.0, 3.0):
        ls, dp = _nan(1), _nan(n)
        L.check(lib.pcd_l1_loss(pd.data_ptr(), td.data_ptr(), n, scale, ls.data_ptr(), dp.data_ptr(), st), "l1_loss")
        torch.cuda.synchronize()
        s, bound, dpred = T.l1_statement(pred, target, scale)
        J.within("pcd_l1_loss sum", (n, scale), ls, s.reshape(1), bound.reshape(1))
        J.exact("pcd_l1_loss dpred", (n, scale), dp, dpred)
        assert int((dpred == 0).sum()) == (n + 6) // 7
    J.report()


@pytest.mark.parametrize("m", [1, 257])
def test_enc1_linear_and_vec3_expand(m):
    L, lib, st = _lib_st()
    J = Judge()
    for n_points in (1, 128):
        for c1 in (64, 37):
            x, w, tb = T.enc1_case(m, n_points, c1)
            xd, wd, tbd = _dev(x), _dev(w), _dev(tb)
            out = _nan(m, c1)
            L.check(lib.pcd_enc1_linear(xd.data_ptr(), m, n_points, wd.data_ptr(), c1, tbd.data_ptr(), out.data_ptr(), st), "enc1_linear")
            torch.cuda.synchronize()
            want, bound = T.enc1_statement(x, n_points, w, tb)
            J.within("pcd_enc1_linear", (m, n_points, c1), out, want, bound)
    for k in (64, 37):
        vec, w = T.expand_case(m, k)
        vd, wd = _dev(vec), _dev(w)
        out = _nan(m, k, dtype=torch.float16)
        L.check(lib.pcd_vec3_expand_f16(vd.data_ptr(), wd.data_ptr(), m, k, out.data_ptr(), st), "vec3_expand")
        torch.cuda.synchronize()
        want, bound = T.vec3_expand_statement(vec, w)
        J.within("pcd_vec3_expand_f16", (m, k), out, want.clamp(-T.F16_MAX, T.F16_MAX), bound)
        _saturated_exactly("pcd_vec3_expand_f16", (m, k), out, want, bound, ["-"] * k)
    J.report()


# ------------------------------------------------------------------------------------------------------------ latent trainer kernels
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows,c,groups", T.GN_SHAPES)
def test_groupnorm_f32(rows, c, groups, relu):
    L, lib, st = _lib_st()
    J = Judge()
    k = T.gn_case(rows, c, groups)
    x, gamma, beta, dy = (_dev(k[n]) for n in ("x", "gamma", "beta", "dy"))
    y, mean, rstd = _nan(rows, c), _nan(rows, groups), _nan(rows, groups)
    L.check(lib.pcd_groupnorm_f32(x.data_ptr(), rows, c, groups, gamma.data_ptr(), beta.data_ptr(), 1e-5, relu, y.data_ptr(), mean.data_ptr(),
                                  rstd.data_ptr(), st), "groupnorm")
    dx, dgamma, dbeta = _nan(rows, c), _nan(c), _nan(c)
    L.check(lib.pcd_groupnorm_backward_f32(dy.data_ptr(), x.data_ptr(), rows, c, groups, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                           rstd.data_ptr(), relu, dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), st), "groupnorm_backward")
    torch.cuda.synchronize()
    shape = (rows, c, groups, f"relu {relu}")
    s = T.gn_stats_statement(k["x"], groups)
    J.within("pcd_groupnorm_f32 mean", shape, mean, s["mean"], s["mean_bound"])
    J.within("pcd_groupnorm_f32 rstd", shape, rstd, s["rstd"], s["rstd_bound"])
    mu, rs = mean.cpu(), rstd.cpu()                                    # the next stages from the kernel's own statistics
    want, bound = T.gn_y_statement(k["x"], mu, rs, k["gamma"], k["beta"], groups, relu)
    J.within("pcd_groupnorm_f32 y", shape, y, want, bound)
    bw = T.gn_backward_statement(k["dy"], k["x"], mu, rs, k["gamma"], k["beta"], groups, relu)
    for name, got in (("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
        J.within("pcd_groupnorm_backward_f32 " + name, shape, got, bw[name], bw[name + "_bound"])
    J.report()


def test_silu_across_the_exponent_range():
    L, lib, st = _lib_st()
    J = Judge()
    x, dy = T.silu_case()
    n = x.numel()
    xd, dyd = _dev(x), _dev(dy)
    y, dx = _nan(n), _nan(n)
    L.check(lib.pcd_silu_f32(xd.data_ptr(), n, y.data_ptr(), st), "silu")
    L.check(lib.pcd_silu_backward_f32(xd.data_ptr(), dyd.data_ptr(), n, dx.data_ptr(), st), "silu_backward")
    torch.cuda.synchronize()
    want, bound = T.silu_statement(x)
    J.within("pcd_silu_f32", n, y, want, bound)
    want, bound = T.silu_backward_statement(x, dy)
    J.within("pcd_silu_backward_f32", n, dx, want, bound)
    J.report()


@pytest.mark.parametrize("n", T.ADAMW_NS)
def test_adamw_vector_scalar_and_statement(n):
    """Aligned buffers take the 16-byte form, buffers offset by one float the one-element form; plain and EMA entry points: all four give
    the same bits, and those lie within the bounds of the fp64 statement."""
    L, lib, st = _lib_st()
    J = Judge()
    h = T.ADAMW_HYPER
    for step in T.ADAMW_STEPS:
        k = T.adamw_case(n, step)
        want_w, want_m1, want_m2, want_e, b = T.adamw_statement(k["w"], k["g"], k["m1"], k["m2"], k["ema"], step=step, **h)
        runs = {}
        for offset in (0, 1):
            for ema in (False, True):
                bufs = {}
                for name in ("w", "g", "m1", "m2", "ema"):
                    base = _nan(n + offset)
                    base[offset:] = k[name].cuda()
                    bufs[name] = base[offset:]
                    assert bufs[name].data_ptr() % 16 == (4 * offset)
                p = [bufs[name].data_ptr() for name in ("w", "g", "m1", "m2")]
                if ema:
                    L.check(lib.pcd_adamw_ema_step(*p, bufs["ema"].data_ptr(), n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], step, h["grad_scale"],
                                                   h["decay"], st), "adamw_ema_step")
                else:
                    L.check(lib.pcd_adamw_step(*p, n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], step, h["grad_scale"], st), "adamw_step")
                torch.cuda.synchronize()
                runs[(offset, ema)] = {name: bufs[name].cpu() for name in ("w", "g", "m1", "m2", "ema")}
        ref = runs[(0, True)]
        shape = (n, f"step {step}")
        for key, r in runs.items():
            for name in ("w", "m1", "m2") + (("ema",) if key[1] else ()):
                J.exact(f"pcd_adamw forms agree ({name})", shape + key, r[name], ref[name])
            J.exact("pcd_adamw leaves the gradient", shape + key, r["g"], k["g"])
            if not key[1]:
                J.exact("pcd_adamw_step leaves no average", shape + key, r["ema"], k["ema"])
        J.within("pcd_adamw_ema_step params", shape, ref["w"], want_w, b["w"])
        J.within("pcd_adamw_ema_step exp_avg", shape, ref["m1"], want_m1, b["m1"])
        J.within("pcd_adamw_ema_step exp_avg_sq", shape, ref["m2"], want_m2, b["m2"])
        J.within("pcd_adamw_ema_step ema", shape, ref["ema"], want_e, b["ema"])
    J.report()
