"""tests/train_cases.py held to account on the CPU, so that tests/test_gpu_train_kernels.py can judge the kernels of csrc/train.hip by it:
  1. every fp64 statement agrees with torch (autograd in float64, torch.max, torch.optim.AdamW) to 1e-12 relative;
  2. no element of any case the GPU module uses is within the ReLU margin (the cap on excluded elements is zero);
  3. an fp32 statement in the kernels' own order stays inside every bound on every case: correct fp32 code can meet the bounds;
  4. the bounds bite: each mutant of the fp32 statement leaves its bound by at least 10 x on a case this module names."""
import pytest
import torch
import torch.nn.functional as F

import train_cases as T

REL = 1e-12


def _close(got, want, what):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= REL * max(scale, 1e-300), (what, float((got - want).abs().max()), scale)


def _ratio(err, bound):
    """max err / bound, with 0 / 0 = 0 and x / 0 = inf; NaN counts as inf."""
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    r = torch.where(err <= bound, torch.where(bound > 0, err / bound, torch.zeros_like(err)), torch.where(bound > 0, err / bound, torch.full_like(err, float("inf"))))
    return float(torch.nan_to_num(r, nan=float("inf"), posinf=float("inf")).max()) if r.numel() else 0.0


def _err(got, want):
    return (got.double() - want.double()).abs()


# ------------------------------------------------------------------------------------------------------------ 1. statements v. torch
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("m,c", [(33, 12), (257, 72), (2, 8)])
def test_batchnorm_statements_agree_with_autograd(m, c, relu):
    g = torch.Generator().manual_seed(m + c)
    z = (torch.randn(m, c, generator=g) * torch.rand(c, generator=g) * 2 + torch.randn(c, generator=g) * 3).float()
    gamma, beta = (0.5 + torch.rand(c, generator=g)) * torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0), 0.3 * torch.randn(c, generator=g)
    da = (3 * torch.randn(m, c, generator=g)).half()
    rm, rv = torch.randn(c, generator=g).double(), (0.5 + torch.rand(c, generator=g)).double()
    with torch.enable_grad():
        zr, gr, br = z.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        rm_t, rv_t = rm.clone(), rv.clone()
        y = F.batch_norm(zr, rm_t, rv_t, gr, br, True, T.MOMENTUM, T.EPS)
        a = F.relu(y) if relu else y
        dz, dgamma, dbeta = torch.autograd.grad(a, (zr, gr, br), da.double())
    st = T.bn_stats_statement(z, rm, rv)
    _close(st["mean"], z.double().mean(0), "mean")
    _close(st["var"], z.double().var(0, unbiased=False), "var")
    _close(st["running_mean"], rm_t, "running_mean")
    _close(st["running_var"], rv_t, "running_var")
    want, _ = T.bn_apply_statement(z, st["mean"], st["var"], gamma, beta, relu)
    _close(want, a.detach(), "apply")
    bw = T.bn_backward_statement(da, z, st["mean"], st["var"], gamma, beta, relu)
    _close(bw["dbeta"], dbeta, "dbeta")
    _close(bw["dgamma"], dgamma, "dgamma")
    _close(T.bn_dz_statement(bw, gamma, bw["dgamma"], bw["dbeta"], m)[0], dz, "dz")


def test_batchnorm_statistics_at_one_row():
    """m = 1: variance 0 and the running variance takes the biased value (torch refuses m = 1 in training mode; the kernel documents this)."""
    z = torch.tensor([[1.5, -2.0, 0.0, 7.0, 1.0, 2.0, 3.0, 4.0]])
    rm, rv = torch.zeros(8), torch.ones(8)
    st = T.bn_stats_statement(z, rm, rv)
    assert torch.equal(st["mean"], z[0].double()) and torch.equal(st["var"], torch.zeros(8, dtype=torch.float64))
    _close(st["running_var"], (1 - T.MOMENTUM) * rv.double(), "running_var")
    assert float(st["var_bound"].max()) == 0.0


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows,c,groups", T.GN_SHAPES)
def test_groupnorm_statements_agree_with_autograd(rows, c, groups, relu):
    k = T.gn_case(rows, c, groups)
    with torch.enable_grad():
        xr, gr, br = (k[n].double().requires_grad_(True) for n in ("x", "gamma", "beta"))
        y = F.group_norm(xr, groups, gr, br, T.EPS)
        a = F.relu(y) if relu else y
        dx, dgamma, dbeta = torch.autograd.grad(a, (xr, gr, br), k["dy"].double())
    st = T.gn_stats_statement(k["x"], groups)
    want, _ = T.gn_y_statement(k["x"], st["mean"], st["rstd"], k["gamma"], k["beta"], groups, relu)
    _close(want, a.detach(), "y")
    bw = T.gn_backward_statement(k["dy"], k["x"], st["mean"], st["rstd"], k["gamma"], k["beta"], groups, relu)
    for name, ref in (("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
        _close(bw[name], ref, name)


def test_small_statements_agree_with_torch():
    pred, target = T.l1_case(257)
    with torch.enable_grad():
        pr = pred.double().requires_grad_(True)
        loss = F.l1_loss(pr, target.double())
        (dp,) = torch.autograd.grad(loss, pr)
    s, _, dpred = T.l1_statement(pred, target, 1.0)
    _close(s / 257, loss.detach(), "l1")
    assert torch.equal(torch.sign(dpred), torch.sign(dp).float()) and int((dpred == 0).sum()) == 37
    assert torch.equal(dpred.abs().max(), torch.tensor(1.0, dtype=torch.float32) / torch.tensor(257.0, dtype=torch.float32))
    x, dy = T.silu_case()
    with torch.enable_grad():
        xr = x.double().requires_grad_(True)
        y = F.silu(xr)
        (dx,) = torch.autograd.grad(y, xr, dy.double())
    _close(T.silu_statement(x)[0], y.detach(), "silu")
    _close(T.silu_backward_statement(x, dy)[0], dx, "silu backward")
    for batch, n, c in ((3, 257, 130), (1, 5, 65), (3, 2, 4), (1, 1, 1)):
        a, dg = T.colmax_case(batch, n, c)
        v, i = a.float().reshape(batch, n, c).max(1)                       # CPU torch.max: the first index on ties
        mx, arg = T.colmax_statement(a, batch, n)
        assert torch.equal(mx, v) and torch.equal(arg.long(), i)
        mx32, arg32 = T.colmax32(a, batch, n)
        assert torch.equal(mx32, v) and torch.equal(arg32.long(), i)
        da = T.maxpool_backward_statement(dg, arg, batch, n)
        want = torch.zeros(batch, n, c).scatter_(1, i.unsqueeze(1), dg.clamp(-T.F16_MAX, T.F16_MAX).unsqueeze(1)).reshape(batch * n, c).half()
        assert torch.equal(da, want) and float(da.float().abs().max()) == T.F16_MAX
    k = T.matmul_case(5, 70, 33)
    want, mag = T.matmul_statement(k["a"].t().contiguous(), k["b"].t().contiguous(), 1, 1, k["bias"], k["c_old"])
    _close(want, k["c_old"].double() + k["a"].double() @ k["b"].double() + k["bias"].double(), "matmul")
    assert bool((mag >= want.abs()).all())
    mat, vec, _ = T.vec3_case(129, 72)
    _close(T.vec3_outer_statement(mat, vec)["out"], torch.einsum("mj,mk->jk", vec.double(), mat.double()), "vec3_outer")
    x3, w3, tb = T.enc1_case(257, 128, 37)
    _close(T.enc1_statement(x3, 128, w3, tb)[0], F.linear(x3.double(), w3.double()) + tb.double().repeat_interleave(128, 0)[:257], "enc1")


def test_adamw_statement_agrees_with_torch_optim():
    h = T.ADAMW_HYPER
    f = {n: T.f32(h[n]) for n in ("lr", "b1", "b2", "eps", "wd")}
    k = T.adamw_case(1003, 1)
    w, m1, m2 = k["w"].double(), k["m1"].double(), k["m2"].double()
    p = torch.nn.Parameter(w.clone())
    opt = torch.optim.AdamW([p], lr=f["lr"], betas=(f["b1"], f["b2"]), eps=f["eps"], weight_decay=f["wd"])
    g = torch.Generator().manual_seed(3)
    for step in (1, 2, 3):
        grad = torch.randn(1003, generator=g, dtype=torch.float64)
        p.grad = grad.clone()
        opt.step()
        w, m1, m2, _, _ = T.adamw_statement(w, grad * 64.0, m1, m2, None, step=step, fp32_corrections=False,
                                            **{n: h[n] for n in ("lr", "b1", "b2", "eps", "wd", "grad_scale")})
        _close(w, p.detach(), f"adamw step {step}")
    _close(m1, opt.state[p]["exp_avg"], "exp_avg")
    _close(m2, opt.state[p]["exp_avg_sq"], "exp_avg_sq")


def test_sat16_and_geometry():
    t = torch.tensor([1e9, -1e9, 65519.0, 65520.0, -70000.0, 1.0], dtype=torch.float64)
    assert T.sat16(t).tolist() == [65504.0, -65504.0, 65504.0, 65504.0, -65504.0, 1.0]
    assert T.cr_grid(200, 2304) == (128, 18) and T.cr_grid(8, 1) == (128, 1) and T.cr_grid(72, 500, 6) == (128, 4)
    assert T.cr_grid(64, 1 << 20) == (512, 2048) and T.strip_chain(8, 129) == 4 + 32 + 2
    assert [T.matmul_route(m, ta, tb) for m, ta, tb in ((32, 0, 0), (33, 0, 0), (32, 0, 1), (32, 1, 0), (1, 1, 1))] == ["nn", "generic", "nt", "generic", "generic"]
    assert T.l1_blocks(262144) == 1024 and T.l1_chain(262144 + 257) == 2 + 8 + 1024


# ------------------------------------------------------------------------------------------------------------ 2. placement and margin
def test_families_stand_at_every_edge():
    every = set(T.FAMILIES)
    for c in T.BN_CS:
        first, last, boundary = set(), set(), set()
        for i in range(len(T.BN_MS)):
            names = T.column_names(c, 8 * i)
            first |= set(names[:8])
            last |= set(names[(c - 1) // 8 * 8:])
            if c > 64:
                boundary |= set(names[56:72])
                assert set(names[56:72]) == every                     # in every single case
        assert first == every and last == every and (c <= 64 or boundary == every), c


@pytest.mark.parametrize("c", T.BN_CS + T.BN_CS_RAGGED)
def test_no_element_near_the_relu_threshold(c):
    for k in T.bn_cases(c):
        assert int(T.in_band(k["z"], k["mean"], k["var"], k["gamma"], k["beta"], k["names"]).sum()) == 0, (k["m"], c)
        assert k["z"].dtype == torch.float32 and k["mean"].dtype == torch.float32 and k["da"].dtype == torch.float16
        t, y, _ = T.bn_pre64(k["z"], k["mean"], k["var"], k["gamma"], k["beta"])
        for j, name in enumerate(k["names"]):
            if name in T.CONSTANT or k["m"] == 1:                         # handed statistics of a constant column are exact
                assert float(k["mean"][j]) == float(k["z"][0, j]) and float(k["var"][j]) == 0.0, (k["m"], c, j, name)
            if name in T.EXEMPT:
                assert bool((y[:, j] == 0).all()) and float(k["beta"][j]) == 0.0
            if name == "saturate" and k["m"] >= 31:
                assert float(y[:, j].abs().max()) > T.F16_MAX, (k["m"], c, j)


def test_no_groupnorm_element_near_the_relu_threshold():
    for shape in T.GN_SHAPES:
        k = T.gn_case(*shape)
        assert int(T.gn_in_band(k).sum()) == 0, shape
        assert float(k["x"][shape[0] - 1, :shape[1] // shape[2]].std()) == 0.0 or shape[1] // shape[2] == 1


# ------------------------------------------------------------------------------------------------------------ 3. fp32 inside the bounds
def _bn_ratios(k, relu, **mut):
    """error / bound of the fp32 statement (or a mutant of it) on one case, per output."""
    z, m = k["z"], k["m"]
    a32 = T.bn_apply32(z, k["mean"], k["var"], k["gamma"], k["beta"], relu)
    want, bound = T.bn_apply_statement(z, k["mean"], k["var"], k["gamma"], k["beta"], relu)
    out = {"a": _ratio(_err(a32, want.clamp(-T.F16_MAX, T.F16_MAX)), bound)}
    dgamma, dbeta, dz = T.bn_backward32(k["da"], z, k["mean"], k["var"], k["gamma"], k["beta"], relu, **mut)
    bw = T.bn_backward_statement(k["da"], z, k["mean"], k["var"], k["gamma"], k["beta"], relu)
    out["dgamma"] = _ratio(_err(dgamma, bw["dgamma"]), bw["dgamma_bound"])
    out["dbeta"] = _ratio(_err(dbeta, bw["dbeta"]), bw["dbeta_bound"])
    want, bound = T.bn_dz_statement(bw, k["gamma"], dgamma, dbeta, m)
    out["dz"] = _ratio(_err(dz, want.clamp(-T.F16_MAX, T.F16_MAX)), bound)
    return out


def _stats_ratios(k, **mut):
    z, m = k["z"], k["m"]
    mean, var = T.bn_stats32(z, **mut)
    rm, rv = T.bn_running32(mean, var, m, k["running_mean"], k["running_var"])
    st = T.bn_stats_statement(z, k["running_mean"], k["running_var"])
    return {n: _ratio(_err(v, st[n]), st[n + "_bound"]) for n, v in (("mean", mean), ("var", var), ("running_mean", rm), ("running_var", rv))}


@pytest.mark.parametrize("c", T.BN_CS + T.BN_CS_RAGGED)
def test_fp32_batchnorm_stays_inside_the_bounds(c):
    worst = {}
    for k in T.bn_cases(c):
        rs = [_bn_ratios(k, relu) for relu in (0, 1)] + ([_stats_ratios(k)] if c % 8 == 0 else [])
        for r in rs:
            for n, v in r.items():
                assert v <= 1.0, (n, k["m"], c, v)
                worst[n] = max(worst.get(n, 0.0), v)
    print(f"fp32 statement, c = {c}: worst error / bound {({n: round(v, 4) for n, v in worst.items()})}")


def test_fp32_one_pass_variance_with_a_bad_shift():
    """The figures of the one-pass variance at m = 2304, std 0.7, mean 30 with row 0 an 8 sigma (and a 100 sigma) outlier: the formula is
    sound, and var_bound (which grows with the shift's distance) covers both."""
    g = torch.Generator().manual_seed(1)
    for sigmas in (8, 100):
        z = (30 + 0.7 * torch.randn(2304, 8, generator=g, dtype=torch.float64))
        z[0] = 30 + sigmas * 0.7
        z = z.float()
        _, var = T.bn_stats32(z)
        st = T.bn_stats_statement(z)
        rel = float((_err(var, st["var"]) / st["var"]).max())
        print(f"row 0 at {sigmas} sigma: relative error of the variance {rel:.2e}, error / bound {_ratio(_err(var, st['var']), st['var_bound']):.3f}")
        assert _ratio(_err(var, st["var"]), st["var_bound"]) <= 1.0


def test_fp32_sums_stay_inside_the_bounds():
    worst = {}

    def take(name, r, where):
        assert r <= 1.0, (name, where, r)
        worst[name] = max(worst.get(name, 0.0), r)
    for c in T.BN_CS + T.BN_CS_RAGGED:
        for groups in T.COLSUM_GROUPS:
            for rpg in T.COLSUM_ROWS:
                x, _ = T.colsum_case(rpg, groups, c)
                want, bound = T.colsum_statement(x, rpg, groups)
                take("colsum", _ratio(_err(T.colsum32(x, rpg, groups), want), bound), (rpg, groups, c))
    for k in T.VEC3_KS + T.BN_CS_RAGGED:
        for m in T.BN_MS:
            mat, vec, _ = T.vec3_case(m, k)
            st = T.vec3_outer_statement(mat, vec)
            out, vsum = T.vec3_outer32(mat, vec)
            take("vec3_outer", _ratio(_err(out, st["out"]), st["out_bound"]), (m, k))
            take("vec3_outer vsum", _ratio(_err(vsum, st["vsum"]), st["vsum_bound"]), (m, k))
    for n in T.L1_NS:
        pred, target = T.l1_case(n)
        s, bound, _ = T.l1_statement(pred, target, 8.0)
        take("l1", _ratio(_err(T.l1_32(pred, target), s), bound), n)
    print(f"fp32 statement: worst error / bound {({n: round(v, 4) for n, v in worst.items()})}")


@pytest.mark.parametrize("m", T.MATMUL_MS)
def test_fp32_matmul_stays_inside_the_bounds(m):
    worst = {}
    for k in T.MATMUL_KS:
        for n in T.MATMUL_NS:
            case = T.matmul_case(m, k, n)
            for ta in (0, 1):
                for tb in (0, 1):
                    for bias in (None, case["bias"]):
                        for c_old in (None, case["c_old"]):
                            a = case["a"].t().contiguous() if ta else case["a"]
                            b = case["b"].t().contiguous() if tb else case["b"]
                            route = T.matmul_route(m, ta, tb)
                            want, mag = T.matmul_statement(a, b, ta, tb, bias, c_old)
                            r = _ratio(_err(T.matmul32(a, b, ta, tb, bias, c_old), want), T.sum_bound(T.matmul_chain(route, k), mag))
                            assert r <= 1.0, (m, k, n, ta, tb, route, r)
                            worst[route] = max(worst.get(route, 0.0), r)
    print(f"fp32 matmul, m = {m}: worst error / bound {({n: round(v, 4) for n, v in worst.items()})}")


def test_generic_matmul_chain_counts_the_roundings_around_the_products():
    """Why matmul_chain("generic", k) is k + 3: with L = k, the additions of the products alone, correct fp32 code leaves the bound at k = 1,
    where the product's rounding, the bias and the accumulated C are the whole error (1.94 x on this case)."""
    case = T.matmul_case(33, 1, 257)
    want, mag = T.matmul_statement(case["a"], case["b"], 0, 0, case["bias"], case["c_old"])
    err = _err(T.matmul32(case["a"], case["b"], 0, 0, case["bias"], case["c_old"]), want)
    print(f"generic 33 x 1 x 257, bias and accumulate: error / bound {_ratio(err, T.sum_bound(1, mag)):.3f} with L = k, {_ratio(err, T.sum_bound(4, mag)):.3f} with L = k + 3")
    assert _ratio(err, T.sum_bound(1, mag)) > 1.0 and _ratio(err, T.sum_bound(T.matmul_chain("generic", 1), mag)) <= 1.0


def test_fp32_elementwise_stay_inside_the_bounds():
    worst = {}

    def take(name, r, where=None):
        assert r <= 1.0, (name, where, r)
        worst[name] = max(worst.get(name, 0.0), r)
    x, dy = T.silu_case()
    want, bound = T.silu_statement(x)
    take("silu", _ratio(_err(x / (1 + torch.exp(-x)), want), bound))
    s = 1 / (1 + torch.exp(-x))
    want, bound = T.silu_backward_statement(x, dy)
    take("silu backward", _ratio(_err(dy * s * (1 + x * (1 - s)), want), bound))
    for m in (1, 257):
        for n_points in (1, 128):
            for c1 in (64, 37):
                x3, w3, tb = T.enc1_case(m, n_points, c1)
                want, bound = T.enc1_statement(x3, n_points, w3, tb)
                rows = torch.arange(m) // n_points
                got = x3[:, 0:1] * w3[:, 0] + x3[:, 1:2] * w3[:, 1] + x3[:, 2:3] * w3[:, 2] + tb[rows]
                take("enc1", _ratio(_err(got, want), bound), (m, n_points, c1))
        for k in (64, 37):
            vec, w = T.expand_case(m, k)
            want, bound = T.vec3_expand_statement(vec, w)
            got = T.sat16(vec[:, 0:1] * w[0] + vec[:, 1:2] * w[1] + vec[:, 2:3] * w[2])
            take("vec3_expand", _ratio(_err(got, want.clamp(-T.F16_MAX, T.F16_MAX)), bound), (m, k))
            assert m == 1 or float(got.float().abs().max()) == T.F16_MAX
    for shape in T.GN_SHAPES:
        k = T.gn_case(*shape)
        groups = shape[2]
        for relu in (0, 1):
            y, mu, rs = T.gn32(k["x"], k["gamma"], k["beta"], groups, relu)
            st = T.gn_stats_statement(k["x"], groups)
            take("gn mean", _ratio(_err(mu, st["mean"]), st["mean_bound"]), shape)
            take("gn rstd", _ratio(_err(rs, st["rstd"]), st["rstd_bound"]), shape)
            want, bound = T.gn_y_statement(k["x"], mu, rs, k["gamma"], k["beta"], groups, relu)
            take("gn y", _ratio(_err(y, want), bound), shape)
            dx, dgamma, dbeta = T.gn_backward32(k["dy"], k["x"], mu, rs, k["gamma"], k["beta"], groups, relu)
            bw = T.gn_backward_statement(k["dy"], k["x"], mu, rs, k["gamma"], k["beta"], groups, relu)
            for name, got in (("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
                take("gn " + name, _ratio(_err(got, bw[name]), bw[name + "_bound"]), (shape, relu))
    h = T.ADAMW_HYPER
    for n in T.ADAMW_NS:
        for step in T.ADAMW_STEPS:
            k = T.adamw_case(n, step)
            w, m1, m2, e = T.adamw32(k["w"], k["g"], k["m1"], k["m2"], k["ema"], step=step, **h)
            ww, wm1, wm2, we, b = T.adamw_statement(k["w"], k["g"], k["m1"], k["m2"], k["ema"], step=step, **h)
            for name, got, want in (("w", w, ww), ("m1", m1, wm1), ("m2", m2, wm2), ("ema", e, we)):
                take("adamw " + name, _ratio(_err(got, want), b[name]), (n, step))
    print(f"fp32 statement: worst error / bound {({n: round(v, 4) for n, v in worst.items()})}")


# ------------------------------------------------------------------------------------------------------------ 4. the bounds bite
def test_mutants_leave_the_bounds():
    """Each mutant of the fp32 statement is outside its bound by >= 10 x on the case named here (error / bound printed)."""
    found = {}

    def take(mutant, r, where):
        if r > found.get(mutant, (0.0, None))[0]:
            found[mutant] = (r, where)
    # a. the last row of a ragged chunk dropped: colsum at 129 rows per group (a chunk of one row), BatchNorm backward at m = 129
    x, _ = T.colsum_case(129, 3, 72)
    want, bound = T.colsum_statement(x, 129, 3)
    take("last row of a ragged chunk dropped", _ratio(_err(T.colsum32(x, 129, 3, drop_last_ragged_row=True), want), bound), "colsum 3 x 129 x 72")
    k = T.bn_cases(72)[T.BN_MS.index(129)]
    take("last row of a ragged chunk dropped", _bn_ratios(k, 1, drop_last_ragged_row=True)["dbeta"], "bn_backward dbeta m = 129 c = 72")
    # b. the last column of a ragged 8-column group zeroed
    x, _ = T.colsum_case(500, 1, 37)
    want, bound = T.colsum_statement(x, 500, 1)
    take("last column of a ragged group zeroed", _ratio(_err(T.colsum32(x, 500, 1, zero_last_ragged_column=True), want), bound), "colsum 1 x 500 x 37")
    k = T.bn_cases(12)[T.BN_MS.index(257)]
    take("last column of a ragged group zeroed", _bn_ratios(k, 0, zero_last_ragged_column=True)["dgamma"], "bn_backward dgamma m = 257 c = 12")
    # c. unbiased for biased variance: the hardest case is the largest m (the two differ by 1 / (m - 1))
    for m in (33, 2305):
        k = T.bn_cases(200)[T.BN_MS.index(m)]
        take(f"unbiased variance for biased, m = {m}", _stats_ratios(k, unbiased_mutant=True)["var"], f"bn_batch_stats var m = {m} c = 200")
    # d. mask >= for >: the constant column with beta = 0, whose pre-activation is exactly 0
    k = T.bn_cases(64)[T.BN_MS.index(33)]
    r = _bn_ratios(k, 1, ge_mutant=True)
    take("mask >= for >", max(r["dbeta"], r["dz"]), "bn_backward dbeta / dz m = 33 c = 64 (const_beta0)")
    # e. dz without its dgamma / m term
    k = T.bn_cases(8)[T.BN_MS.index(32)]
    take("dgamma / m omitted from dz", _bn_ratios(k, 1, no_dgamma_mutant=True)["dz"], "bn_backward dz m = 32 c = 8")
    # f. the bias once per k block on the few-rows route
    case = T.matmul_case(32, 300, 70)
    want, mag = T.matmul_statement(case["a"], case["b"], 0, 0, case["bias"], None)
    got = T.matmul32(case["a"], case["b"], 0, 0, case["bias"], None, bias_per_block_mutant=True)
    take("bias added once per k block", _ratio(_err(got, want), T.sum_bound(T.matmul_chain("nn", 300), mag)), "matmul_f32 nn 32 x 300 x 70")
    for mutant, (r, where) in found.items():
        print(f"mutant '{mutant}': error / bound {r:.3g} on {where}")
        assert r >= 10.0, (mutant, r, where)
    assert len(found) == 7
    # g. argmax keeping the last index on ties: exact outputs, so the mutant simply has to differ
    a, _ = T.colmax_case(3, 5, 65)
    mx, arg = T.colmax_statement(a, 3, 5)
    mx_m, arg_m = T.colmax32(a, 3, 5, last_index_mutant=True)
    assert torch.equal(mx_m, mx) and not torch.equal(arg_m, arg)
    assert arg[:, 2].tolist() == [1, 1, 1] and arg_m[:, 2].tolist() == [4, 4, 4] and arg[:, 3].tolist() == [0, 0, 0] and arg_m[:, 3].tolist() == [4, 4, 4]
    print("mutant 'argmax takes the last index on ties': differs on colmax 3 x 5 x 65, columns 2 (rows 1 / 4) and 3 (rows 0 / 4)")
