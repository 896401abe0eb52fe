"""The evaluation kernels (csrc/metrics.hip, csrc/sinkhorn.hip, csrc/metrics_pairs.hip) stage by stage against the CPU statement
of tests/metrics_statement.py.  GPU only.

  * Stages compiled without contraction whose result does not depend on an order (normalised clouds, per-query min d^2, voxel bits,
    the BCE of two binary grids) must equal the fp32 statement bit for bit.
  * The Chamfer column is held to the fp64 statement at 2e-6 absolute (scale 1), the bound tests/test_gpu_kernels.py uses.
  * The Sinkhorn stages (contraction on, hardware exponential, online log-sum-exp) are held to the fp64 statement at
    FACTOR x the fp32 statement's own deviation from fp64 on the same input (tests/test_metrics_statement_cpu.py records them;
    the same helpers of tests/metrics_cases.py compute them here), the EMD never above 2e-5 relative.
The stages of `pcd_pair_metrics` are read from its workspace through `pcd_pair_metrics_workspace_layout`.

Measured on an MI355X: the kernel's deviation from fp64 as a multiple of the fp32 statement's deviation, worst over the cases
(and the worst absolute figure behind it):
    stage                                    worst ratio   kernel     fp32 statement   bound
    pcd_sinkhorn_dual_update                 1.53          1.43e-08   9.35e-09         8
    pcd_sinkhorn_cost, row costs             7.33          1.65e-06   2.25e-07         16 (see ROW_COST_FACTOR)
    pcd_sinkhorn_cost, cost (relative)       9.17          4.16e-07   4.54e-08         16
    pair entry, alpha                        2.84          2.46e-08   8.66e-09         8
    pair entry, beta                         2.34          2.37e-08   1.01e-08         8
    pair entry, row costs                    8.93          2.05e-08   2.30e-09         16
    pair entry, cmax                         1.65          1.87e-07   1.13e-07         8
    pair entry, EMD (relative)               4.69          1.83e-07   3.90e-08         8, at most 2e-5
    Chamfer column against fp64              worst 2.6e-07 (512 pairs of <= 8 points); 3.3e-09 at 1300 x 1100     2e-6
    pcd_binary_bce_mean against fp64         at most 1.0 x the fp32 torch call's deviation                          8"""
import pytest
import torch
import torch.nn.functional as F

import metrics_cases as K
import metrics_statement as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FACTOR = 8.0                 # bound of a Sinkhorn stage = FACTOR x (fp32 statement - fp64 statement) on that input
# The cost stage needs more than 8: measured up to 9.2 x (64 x 500, epsilon 1e-2, the batch cost) and 8.9 x (2048 x 2048 row costs).
# The statement divides every distance by cmax, each quotient rounded on its own, so its errors average out over a row; the kernel
# multiplies by ONE rounded 1 / cmax and feeds -lambda * c through the hardware exponential (argument scaled by a rounded log2 e):
# both add an error of ~|argument| 2^-24 with the same sign for every term of a row, which a sum over m terms does not average.
ROW_COST_FACTOR = 16.0
EMD_REL_MAX = 2e-5           # and the EMD never looser than this
CHAMFER_ABS = 2e-6           # Chamfer against the fp64 statement, scale 1
HALF_ULP = 2.0 ** -24        # a SCALAR stage's fp32 deviation is one draw of a rounding error and can be ~0 by luck: it counts as at
                             # least half an ulp of the value, the error of the correctly rounded fp32 result


@pytest.fixture(scope="module")
def lib():
    from shapegen_amd import _lib
    _lib.require_gpu()
    return _lib.load()


def same(x, y):
    """Bit-for-bit equality of two fp32 tensors, a NaN equal to a NaN."""
    return x.shape == y.shape and torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=5.0),
                                                                                                torch.nan_to_num(y, nan=5.0))


def run_pairs(lib, a, b, with_sinkhorn=False, epsilon=1e-2, thresh=1e-5, max_iter=100):
    """One `pcd_pair_metrics` call on ragged lists of (n_i, 3) clouds; -> rows and every stage buffer of the workspace, on the CPU.
    The workspace starts as all-ones bytes (NaN as fp32), so a stage the call did not write cannot pass for one it wrote."""
    from shapegen_amd import _lib
    pa, na = K.pack(a)
    pb, nb = K.pack(b)
    P, NA, NB = len(a), pa.shape[1], pb.shape[1]
    NQ = max(NA, NB)
    log_mu = torch.log(1.0 / na.clamp_min(1).float() + 1e-10)
    log_nu = torch.log(1.0 / nb.clamp_min(1).float() + 1e-10)
    lay = _lib.pair_metrics_workspace_layout(P, NA, NB)
    assert lay["total"] == lib.pcd_pair_metrics_workspace_bytes(P, NA, NB)
    ws = torch.full((lay["total"],), 255, dtype=torch.uint8, device="cuda")
    rows = torch.full((P, 3), float("nan"), device="cuda")
    dev = [t.cuda() for t in (pa, na, pb, nb, log_mu, log_nu)]
    _lib.check(lib.pcd_pair_metrics(dev[0].data_ptr(), dev[1].data_ptr(), NA, dev[2].data_ptr(), dev[3].data_ptr(), NB, P,
                                    1 if with_sinkhorn else 0, float(epsilon), float(thresh), int(max_iter), dev[4].data_ptr(),
                                    dev[5].data_ptr(), rows.data_ptr(), ws.data_ptr(), lay["total"], _lib.stream_ptr()), "pair_metrics")
    host = ws.cpu()

    def field(name, shape, dtype=torch.float32):
        count = 1
        for s in shape:
            count *= s
        return host[lay[name]:lay[name] + 4 * count].view(dtype).reshape(shape)

    return dict(rows=rows.cpu(), na=na, nb=nb, an=field("an", (P, NA, 3)), bn=field("bn", (P, NB, 3)), mins=field("mins", (P, 2, NQ)),
                alpha=field("alpha", (P, NA)), beta=field("beta", (P, NB)), rowc=field("rowc", (P, NA)), cmax=field("cmax", (P,)),
                err=field("err", (2, P, 2)), bits=field("bits", (P, 2, 1024), torch.int32))


def occupancy_bits(points):
    """The oracle's voxelize of one cloud as the kernel's bit sets: voxel v = (x*32 + y)*32 + z is bit (v & 31) of word v >> 5."""
    from oracle import torch_oracle as O
    occ = O.voxelize(points)[0].reshape(1024, 32).to(torch.int64)
    words = (occ << torch.arange(32)).sum(dim=1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


# ------------------------------------------------------------------ bit-exact stages
def _planted_clouds():
    """(n, where) clouds whose bounding box -- centre and scale -- is set by ONE point, at index 0, 256 (the second pass of the
    256-thread stride loop) or n - 1; n = 1 normalises to 0 / 0."""
    out = []
    for n in (1, 2, 255, 256, 257, 1000):
        for where in sorted({0, 256, n - 1}):
            if where >= n:
                continue
            g = torch.Generator().manual_seed(17 * n + where)
            c = torch.rand(n, 3, generator=g) - 0.5 + torch.tensor([0.3, -0.2, 0.1])
            c[where] = torch.tensor([3.25, -2.5, 0.1])                   # max x, min y of the cloud; the other extremes lie elsewhere
            out.append((n, where, c))
    return out


def test_normalised_clouds_are_bit_exact(lib):
    from shapegen_amd import metrics as M
    clouds = _planted_clouds()
    want = [S.normalize(c) for _, _, c in clouds]
    assert torch.isnan(want[0]).all() and all(torch.isfinite(w).all() for w in want[1:])
    for n in sorted({n for n, _, _ in clouds}):                             # pcd_normalize_to_cube: one batch per size
        sel = [i for i, (m, _, _) in enumerate(clouds) if m == n]
        got = M.normalize_to_cube(torch.stack([clouds[i][2] for i in sel]).cuda()).cpu()
        for j, i in enumerate(sel):
            assert same(got[j], want[i]), ("pcd_normalize_to_cube", clouds[i][:2])
    a = [c for _, _, c in clouds]                                           # the pair kernel: every cloud once as a, once as b
    b = a[1:] + a[:1]
    r = run_pairs(lib, a, b)
    for i in range(len(a)):
        assert same(r["an"][i, :a[i].shape[0]], want[i]), ("pair a", clouds[i][:2])
        assert same(r["bn"][i, :b[i].shape[0]], want[(i + 1) % len(a)]), ("pair b", clouds[(i + 1) % len(a)][:2])


@pytest.mark.parametrize("name", list(K.CHAMFER_CASES))
def test_chamfer_launch_shapes(lib, name):
    """Every launch shape of the Chamfer kernel (tests/metrics_cases.py says which case reaches which): min d^2 per query bit exact
    in both directions, the Chamfer column within 2e-6 of the fp64 statement, the BCE column and the voxel bits exact."""
    a, b, check = K.chamfer_case(name)
    r = run_pairs(lib, a, b)
    worst = 0.0
    for p in check:
        s32, s64 = S.pair(a[p], b[p], torch.float32, False), S.pair(a[p], b[p], torch.float64, False)
        n, m = a[p].shape[0], b[p].shape[0]
        assert same(r["an"][p, :n], s32["an"]) and same(r["bn"][p, :m], s32["bn"]), (name, p)
        assert torch.equal(r["mins"][p, 0, :n], s32["mins_a"]), (name, p, "a against b")
        assert torch.equal(r["mins"][p, 1, :m], s32["mins_b"]), (name, p, "b against a")
        worst = max(worst, abs(float(r["rows"][p, 0]) - float(s64["chamfer"])))
        assert abs(float(r["rows"][p, 0]) - float(s64["chamfer"])) < CHAMFER_ABS, (name, p)
        assert float(r["rows"][p, 2]) == float(s32["bce"]) and float(r["rows"][p, 1]) == 0.0, (name, p)
        assert torch.equal(r["bits"][p, 0], occupancy_bits(a[p])) and torch.equal(r["bits"][p, 1], occupancy_bits(b[p])), (name, p)
    print(f"chamfer {name}: worst |cd - fp64| {worst:.2e} (bound {CHAMFER_ABS:.0e})")
    for p in range(len(a)):
        if a[p].shape[0] == 0 or b[p].shape[0] == 0:
            assert torch.isnan(r["rows"][p]).all()
        else:
            assert torch.isfinite(r["rows"][p]).all()


def test_voxel_bits_and_bce_on_the_cube_edges(lib):
    """Coordinates outside the cube (+-1.5, +-100), exactly +-1, the voxel boundaries and NaN: `pcd_voxelize` and the bit sets of
    the pair kernel against the oracle's voxelize, the BCE of the two grids exactly 100 k / 32768."""
    from oracle import torch_oracle as O
    from shapegen_amd import utils as U
    g = torch.Generator().manual_seed(9)
    edge = torch.tensor([[-1.0, 1.0, 0.0], [1.5, -1.5, 100.0], [-100.0, float("nan"), 0.999999], [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0],
                         [-1.0000001, 0.9999999, 1.0000001], [float("nan"), float("nan"), float("nan")]])
    steps = (torch.arange(32).float() * 2 / 31 - 1)[:, None].expand(32, 3)          # the voxel boundaries themselves, and one ulp below
    a = torch.cat([edge, steps, torch.nextafter(steps, torch.full_like(steps, -2.0)), torch.rand(300, 3, generator=g) * 2.4 - 1.2])
    b = torch.cat([torch.rand(257, 3, generator=g) * 2 - 1, edge.flip(1)])
    assert torch.equal(U.voxelize(torch.stack([a, a.flip(0)]).cuda()).cpu(), O.voxelize(torch.stack([a, a.flip(0)])))
    assert torch.equal(U.voxelize(b.cuda()).cpu(), O.voxelize(b))
    r = run_pairs(lib, [a, b, a], [b, a, a])
    ba, bb = occupancy_bits(a), occupancy_bits(b)
    assert torch.equal(r["bits"][0, 0], ba) and torch.equal(r["bits"][0, 1], bb) and torch.equal(r["bits"][1, 0], bb)
    k = int((O.voxelize(a) != O.voxelize(b)).sum())
    want = float(F.binary_cross_entropy(O.voxelize(a), O.voxelize(b)))
    assert k > 100 and want == float(torch.tensor(100.0 * k / 32768, dtype=torch.float32))
    assert float(r["rows"][0, 2]) == want == float(r["rows"][1, 2]) and float(r["rows"][2, 2]) == 0.0


@pytest.mark.parametrize("n,kind", [(n, kind) for n in K.BCE_LENGTHS for kind in K.BCE_KINDS])
def test_binary_bce_mean(lib, n, kind):
    """Lengths that are no multiple of the block; binary grids exactly; probabilities and the -100 clamp against fp64
    `F.binary_cross_entropy` at 8 x the deviation of the fp32 torch call."""
    from shapegen_amd import metrics as M
    x, t, exact = K.bce_case(n, kind)
    got = float(M.voxel_bce(x.cuda(), t.cuda()))
    want = float(F.binary_cross_entropy(x.double(), t.double()))
    if exact is not None:
        assert got == float(torch.tensor(exact, dtype=torch.float32)), (n, kind)
        return
    bound = FACTOR * max(abs(float(F.binary_cross_entropy(x, t)) - want), HALF_ULP * want)
    print(f"bce {n} {kind}: |kernel - fp64| {abs(got - want):.2e}, bound {bound:.2e}")
    assert abs(got - want) <= bound, (n, kind, got, want)


# ------------------------------------------------------------------ pcd_chamfer_sums
@pytest.mark.parametrize("n,m", [(1025, 2049), (1024, 1024), (7, 200)])
def test_chamfer_sums(lib, n, m):
    """The one-block-per-cloud form: 1024 queries per pass and 1024 targets per LDS tile, so (1025, 2049) takes the second pass of
    the query loop and the third tile with one element each, (1024, 1024) fills both exactly, (7, 200) fills neither."""
    from shapegen_amd import _lib
    clouds = [K.matched(n, m, 50 + i) for i in range(3)]
    x = torch.stack([S.normalize(c[0]) for c in clouds])
    y = torch.stack([S.normalize(c[1]) for c in clouds])
    sums = torch.full((3, 2), float("nan"), device="cuda")
    xd, yd = x.cuda(), y.cuda()
    _lib.check(lib.pcd_chamfer_sums(xd.data_ptr(), yd.data_ptr(), 3, n, m, sums.data_ptr(), _lib.stream_ptr()), "chamfer_sums")
    sums = sums.cpu().double()
    for i in range(3):
        want = S.chamfer(x[i].double(), y[i].double())
        got = sums[i, 0] / n + sums[i, 1] / m
        print(f"chamfer_sums {n} x {m} [{i}]: |cd - fp64| {abs(float(got - want['chamfer'])):.2e}")
        assert abs(float(got - want["chamfer"])) < CHAMFER_ABS
        assert abs(float(sums[i, 0] - want["sums"][0])) / n < CHAMFER_ABS and abs(float(sums[i, 1] - want["sums"][1])) / m < CHAMFER_ABS


# ------------------------------------------------------------------ Sinkhorn stages, batch-joint entry points
def test_pairwise_max_dist_finds_a_planted_pair(lib):
    """The farthest pair sits at the last index of x and at index 512 of y (the first element of the second LDS tile), in one batch
    entry; its distance 2.5 = |(1.5, 2, 0)| is exact in fp32 at every step, so the kernel must return it exactly."""
    from shapegen_amd import _lib
    g = torch.Generator().manual_seed(3)
    for n, m, bx in ((300, 777, 2), (257, 513, 0)):
        x, y = torch.rand(3, n, 3, generator=g) - 0.5, torch.rand(3, m, 3, generator=g) - 0.5
        x[bx, n - 1] = torch.tensor([-0.75, -1.0, 0.25])
        y[bx, 512] = torch.tensor([0.75, 1.0, 0.25])
        assert float(S.sq_dists(x, y).sqrt().max()) == 2.5
        out = torch.full((1,), float("nan"), device="cuda")
        xd, yd = x.cuda(), y.cuda()
        _lib.check(lib.pcd_pairwise_max_dist(xd.data_ptr(), yd.data_ptr(), 3, n, m, out.data_ptr(), _lib.stream_ptr()), "pair_max")
        assert float(out[0]) == 2.5
        _lib.check(lib.pcd_pairwise_max_dist(yd.data_ptr(), xd.data_ptr(), 3, m, n, out.data_ptr(), _lib.stream_ptr()), "pair_max")
        assert float(out[0]) == 2.5


@pytest.mark.parametrize("epsilon", K.JOINT_EPSILONS)
@pytest.mark.parametrize("n,m", K.JOINT_SIZES)
def test_sinkhorn_dual_update_and_cost(lib, n, m, epsilon):
    """One half-iteration from a NON-ZERO dual of the other cloud (so the fourth float of an LDS entry matters) and the cost stage,
    batch 3, sizes that end inside a tile and inside a block.  err_max is exactly max |new - old| of the arrays the call returns."""
    from shapegen_amd import _lib
    st = _lib.stream_ptr()
    x, y, dual_q, dual_p = K.joint_case(n, m)
    stage, dev = K.joint_stages(n, m, epsilon), K.joint_stage_deviations(n, m, epsilon)
    want = stage[torch.float64]
    xd, yd, cmax = x.cuda(), y.cuda(), stage["cmax"].reshape(1).cuda()
    dq, dp = dual_q.cuda(), dual_p.clone().cuda()
    err = torch.full((1,), float("nan"), device="cuda")
    _lib.check(lib.pcd_sinkhorn_dual_update(xd.data_ptr(), yd.data_ptr(), 3, n, m, cmax.data_ptr(), epsilon, float(stage["log_mu"]),
                                            dq.data_ptr(), dp.data_ptr(), err.data_ptr(), st), "dual_update")
    new = dp.cpu()
    got = float((new.double() - want["dual"]).abs().max())
    print(f"dual_update {n} x {m} eps {epsilon}: kernel {got:.2e}, fp32 statement {dev['dual']:.2e}, ratio {got / dev['dual']:.2f}")
    assert got <= FACTOR * dev["dual"]
    assert float(err[0]) == float((new - dual_p).abs().max())
    assert torch.equal(dq.cpu(), dual_q)
    # cost stage on the duals of a converged run
    alpha, beta = stage["alpha"].cuda(), stage["beta"].cuda()
    rowc = torch.full((3, n), float("nan"), device="cuda")
    cost = torch.full((3,), float("nan"), device="cuda")
    _lib.check(lib.pcd_sinkhorn_cost(xd.data_ptr(), yd.data_ptr(), 3, n, m, cmax.data_ptr(), epsilon, alpha.data_ptr(), beta.data_ptr(),
                                     rowc.data_ptr(), cost.data_ptr(), st), "sinkhorn_cost")
    got_r = float((rowc.cpu().double() - want["row_cost"]).abs().max())
    got_c = float(((cost.cpu().double() - want["cost"]).abs() / want["cost"]).max())
    print(f"sinkhorn_cost {n} x {m} eps {epsilon}: rows kernel {got_r:.2e}, fp32 statement {dev['row_cost']:.2e}, ratio "
          f"{got_r / dev['row_cost']:.2f}; cost kernel {got_c:.2e}, fp32 statement {dev['cost']:.2e}, ratio {got_c / dev['cost']:.2f}")
    assert got_r <= ROW_COST_FACTOR * dev["row_cost"]
    assert got_c <= min(ROW_COST_FACTOR * max(dev["cost"], HALF_ULP), EMD_REL_MAX)
    assert torch.equal(cost.cpu(), rowc.cpu().double().sum(dim=1).float())          # the row sum adds in double: order cannot show


# ------------------------------------------------------------------ Sinkhorn stages, pair entry
def _check_pair_sinkhorn(name, r, tag=""):
    """alpha, beta, row costs per pair and element, cmax and the EMD per case, against each pair's OWN fp64 statement run."""
    runs = K.pair_sinkhorn_statements(name)
    d_cmax = max(max(K.deviation(r32, r64, "cmax"), HALF_ULP * float(r64["cmax"])) for r64, r32 in runs)
    d_emd = max(max(K.deviation(r32, r64, "emd", True), HALF_ULP) for r64, r32 in runs)
    failed = []
    for p, (r64, r32) in enumerate(runs):
        n, m = r64["alpha"].shape[0], r64["beta"].shape[0]
        got = dict(alpha=r["alpha"][p, :n], beta=r["beta"][p, :m], row_cost=r["rowc"][p, :n])
        line = [f"pair_sinkhorn {name}{tag} [{p}] {n} x {m} stop {r64['stop']}:"]
        for key in ("alpha", "beta", "row_cost"):
            k, d = float((got[key].double() - r64[key]).abs().max()), K.deviation(r32, r64, key)
            line.append(f"{key} kernel {k:.2e} fp32 {d:.2e} ratio {k / d:.2f};")
            if not k <= (ROW_COST_FACTOR if key == "row_cost" else FACTOR) * d:
                failed.append((p, key, k, d))
        k = abs(float(r["cmax"][p]) - float(r64["cmax"]))
        line.append(f"cmax kernel {k:.2e} case fp32 {d_cmax:.2e} ratio {k / d_cmax:.2f};")
        if not k <= FACTOR * d_cmax:
            failed.append((p, "cmax", k, d_cmax))
        k = abs(float(r["rows"][p, 1]) - float(r64["emd"])) / float(r64["emd"])
        line.append(f"emd rel kernel {k:.2e} case fp32 {d_emd:.2e} ratio {k / d_emd:.2f}")
        if not k <= min(FACTOR * d_emd, EMD_REL_MAX):
            failed.append((p, "emd", k, d_emd))
        print(" ".join(line))
        assert float(r["rows"][p, 1]) == float(r["rowc"][p, :n].double().sum().float()), (name, p)
        assert abs(float(r["rows"][p, 0]) - float(r64["chamfer"])) < CHAMFER_ABS and float(r["rows"][p, 2]) == float(r64["bce"])
    assert not failed, failed


@pytest.mark.parametrize("name", list(K.PAIR_SINKHORN_CASES))
def test_pair_sinkhorn_stages(lib, name):
    """One call per case; every pair against its own statement run, which stopped at its own iteration: pairs that stop at
    different iterations in one call, a pair that only beta's error keeps running, max_iter before the stop, and thresh = 0 (all
    100 iterations)."""
    a, b, epsilon, thresh, max_iter = K.pair_sinkhorn_case(name)
    _check_pair_sinkhorn(name, run_pairs(lib, a, b, True, epsilon, thresh, max_iter))


def test_the_device_side_stop_iteration_by_iteration(lib):
    """The error slots of the workspace show which iteration a pair ran last.  `stops_differ` has a pair that stops after 3
    iterations and three that stop after 4: with max_iter = 3 every pair's third-iteration errors are the statement's; with
    max_iter = 4 the fourth iteration leaves zeros for the pair that had stopped and the statement's errors for the others; with
    max_iter = 5 the fifth leaves zeros for all, and the duals are those of max_iter = 100."""
    name = "stops_differ"
    a, b, epsilon, thresh, _ = K.pair_sinkhorn_case(name)
    runs = K.pair_sinkhorn_statements(name)
    assert [r64["stop"] for r64, _ in runs] == [3, 4, 4, 4]
    for max_iter in (3, 4, 5):
        r = run_pairs(lib, a, b, True, epsilon, thresh, max_iter)
        slots = r["err"][(max_iter - 1) & 1]                                   # what the last enqueued iteration left: (P, 2)
        for p, (r64, r32) in enumerate(runs):
            if max_iter > r64["stop"]:
                assert slots[p].tolist() == [0.0, 0.0], (max_iter, p)
                continue
            it = r64["iters"][max_iter - 1]
            for j, (key, dual) in enumerate((("err_alpha", "alpha"), ("err_beta", "beta"))):
                tol = 2 * FACTOR * K.deviation(r32, r64, dual)                 # a difference of two duals, each within its bound
                assert abs(float(slots[p, j]) - float(it[key])) <= tol, (max_iter, p, key)
            assert slots[p, 0] > 0, (max_iter, p)                                  # it ran: some alpha moved by at least an ulp
        if max_iter == 5:
            _check_pair_sinkhorn(name, r, " max_iter 5")
