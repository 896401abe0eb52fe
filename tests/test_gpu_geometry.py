"""The cloud-geometry kernels (csrc/cloud_geometry.hip) against the CPU statement of tests/geometry_statement.py.  GPU only.

  * Stage (a), the k nearest neighbours, must equal the fp32 statement bit for bit, d2 and index, in every case of tests/geometry_cases.py
    (which states the launch shape) and for k on both sides of every template instance: same formula without contraction, same key.
  * Stage (b), the normals, is fed with the statement's own neighbour lists.  Directions are compared with the fp64 statement through the
    sine of the angle, |n x n64|; the error of an eigenvector scales with 1 / gap, gap = (l1 - l0) / l2, so the quantity bounded is
    sine x gap in units of 2^-24, over the points with gap >= 0.1 (at most 3 % of a case's points have less: the CPU test asserts it).  The
    curvature is bounded as |c - c64| in units of 2^-24, both lying in [0, 1/3].  The kernel works in double and rounds once, so both
    figures are those of one fp32 rounding of the result, not a multiple of k.
  * Stage (c), the masks, is fed with the statement's d2: mean_distance within 1 fp32 ulp of the rounded fp64 statement, the statistical
    mask equal to the statement's (the cases keep every point 1e-9 relative away from its limit), the radius mask bit for bit.
  * Stage (d), the compaction, bit for bit.

Measured on an MI355X, the worst value per surface case, in units of 2^-24.  The bounds are 4 x the worst of each table rounded up to a power
of two: 4 x 0.641 -> 4 for sine x gap, 4 x 0.130 -> 1 for the curvature.  The kernel is deterministic; the margin is for another compiler.
    sine x gap          sphere 257   sphere 1024   sphere 1300   torus 257   torus 1024   torus 1300
      k =  8            0.385        0.527         0.641         0.319       0.514        0.525
      k = 16            0.531        0.585         0.562         0.488       0.532        0.489
      k = 32            0.480        0.628         0.636         0.477       0.560        0.559
    |c - c64|
      k =  8            0.012        0.004         0.002         0.057       0.023        0.015
      k = 16            0.015        0.004         0.004         0.110       0.031        0.028
      k = 32            0.029        0.008         0.006         0.130       0.060        0.031"""
import numpy as np
import pytest
import torch

import geometry_cases as K
import geometry_statement as G
import surface_statement as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

U = 2.0 ** -24
SINE_GAP_BOUND = 4.0        # units of 2^-24
CURVATURE_BOUND = 1.0       # units of 2^-24
NORM_BOUND = 4 * U


@pytest.fixture(scope="module")
def lib():
    from shapegen_amd import _lib
    _lib.require_gpu()
    return _lib.load()


def same(x, y):
    """Bit-for-bit equality of two tensors, a NaN equal to a NaN."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if not x.dtype.is_floating_point:
        return torch.equal(x, y)
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=5.0), torch.nan_to_num(y, nan=5.0))


def run_knn(lib, queries, targets, k, exclude_self):
    """One `pcd_knn` call on ragged lists (`targets=None`: every cloud against itself, ONE array passed twice); -> d2, index (P, NQ, k) on the
    CPU.  Padding rows hold copies of the cloud's live points and the outputs start as 77 / -7, so nothing unwritten passes."""
    from shapegen_amd import _lib
    pq, nq = K.pack(queries)
    dq, cq = pq.cuda(), nq.cuda()
    if targets is None:
        dt, ct = dq, cq
    else:
        pt, nt = K.pack(targets)
        dt, ct = pt.cuda(), nt.cuda()
    P, NQ, NT = dq.shape[0], dq.shape[1], dt.shape[1]
    d2 = torch.full((P, NQ, k), 77.0, device="cuda")
    index = torch.full((P, NQ, k), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.pcd_knn(dq.data_ptr(), cq.data_ptr(), NQ, dt.data_ptr(), ct.data_ptr(), NT, P, k, int(exclude_self), d2.data_ptr(),
                           index.data_ptr(), _lib.stream_ptr()), "knn")
    return d2.cpu(), index.cpu()


def check_knn(got_d2, got_index, statements, sizes, k, where):
    for i, ((d2, index), n) in enumerate(zip(statements, sizes)):
        assert same(got_d2[i, :n], d2[:, :k].contiguous()), (where, i, k, "d2")
        assert torch.equal(got_index[i, :n], index[:, :k].contiguous()), (where, i, k, "index")
        assert torch.isnan(got_d2[i, n:]).all() and (got_index[i, n:] == -1).all(), (where, i, k, "padding")


@pytest.fixture(scope="module")
def self_runs(lib):
    """`pcd_knn` of a case against itself at one k, made when first asked for and shared."""
    done = {}

    def get(name, k):
        if (name, k) not in done:
            done[name, k] = run_knn(lib, K.self_case(name), None, k, True)
        return done[name, k]
    return get


# ------------------------------------------------------------------ 1. stage (a), bit for bit
@pytest.mark.parametrize("name", list(K.SELF_CASES))
def test_k_nearest_are_bit_exact_within_a_cloud(self_runs, name):
    sizes = [x.shape[0] for x in K.self_case(name)]
    for k in K.KS:
        d2, index = self_runs(name, k)
        check_knn(d2, index, K.self_statements(name), sizes, k, name)


def test_k_nearest_are_bit_exact_between_two_clouds(lib):
    q, t = K.pair_case("pairs")
    for k in K.KS:
        d2, index = run_knn(lib, q, t, k, False)
        check_knn(d2, index, K.pair_statements("pairs"), [x.shape[0] for x in q], k, "pairs")


def test_k_1_without_exclusion_is_the_single_nearest_neighbour(lib):
    """`pcd_knn` at k = 1 equals `pcd_nearest_neighbors` bit for bit: between two clouds, and of a cloud with itself (every point finds
    itself, or the lower index of a duplicate, at distance 0)."""
    from shapegen_amd import metrics as M
    q, t = K.pair_case("pairs")
    for a, b in ((q, t), (K.self_case("doubled"), K.self_case("doubled")), (K.self_case("edges")[:4], K.self_case("edges")[:4])):
        d2, index = run_knn(lib, a, b, 1, False)
        pa, na = K.pack(a)
        pb, nb = K.pack(b)
        want_d2, want_index = (v.cpu() for v in M.nearest_neighbors(pa.cuda(), pb.cuda(), na.cuda(), nb.cuda()))
        assert same(d2[:, :, 0], want_d2) and torch.equal(index[:, :, 0], want_index)


@pytest.mark.parametrize("name", ["edges", "lattice", "tiny"])
def test_a_slot_does_not_depend_on_k(self_runs, name):
    big_d2, big_index = self_runs(name, 32)
    for k in (8, 9, 16, 17):
        d2, index = self_runs(name, k)
        assert same(d2, big_d2[:, :, :k].contiguous()) and torch.equal(index, big_index[:, :, :k].contiguous()), (name, k)


def test_python_k_nearest_neighbors(lib, self_runs):
    """`geometry.k_nearest_neighbors` on ragged lists (zero padding) and on a padded tensor with counts gives the bits of the poisoned call."""
    from shapegen_amd import geometry
    clouds = K.self_case("tiny")
    want_d2, want_index = self_runs("tiny", 9)
    d2, index = (v.cpu() for v in geometry.k_nearest_neighbors([x.cuda() for x in clouds], k=9))
    assert same(d2, want_d2) and torch.equal(index, want_index)
    packed, counts = K.pack(clouds)
    d2, index = (v.cpu() for v in geometry.k_nearest_neighbors(packed.cuda(), k=9, query_counts=counts.cuda()))
    assert same(d2, want_d2) and torch.equal(index, want_index)
    q, t = K.pair_case("pairs")
    d2, index = (v.cpu() for v in geometry.k_nearest_neighbors([x.cuda() for x in q], [y.cuda() for y in t], k=17))
    check_knn(d2, index, K.pair_statements("pairs"), [x.shape[0] for x in q], 17, "python pairs")
    default = geometry.k_nearest_neighbors(packed.cuda(), query_counts=counts.cuda())
    assert default[0].shape == (len(clouds), packed.shape[1], 16)


def test_repeatable_and_independent_of_the_batch(lib, self_runs):
    clouds = K.self_case("edges")
    d2, index = self_runs("edges", 16)
    again = run_knn(lib, clouds, None, 16, True)
    assert same(d2, again[0]) and torch.equal(index, again[1])
    for i in (0, 5, 9):
        alone = run_knn(lib, [clouds[i]], None, 16, True)                       # P = 1 and another padded size
        n = clouds[i].shape[0]
        assert same(alone[0][0, :n], d2[i, :n]) and torch.equal(alone[1][0, :n], index[i, :n]), i


# ------------------------------------------------------------------ 2. stage (b), the normals
def run_normals(lib, clouds, tables, k, mode=0, view=None, curvature=True, index_fill=0):
    """One `pcd_cloud_normals` call on ragged clouds and their (n_i, k) neighbour lists; -> normals (P, N, 3), curvature (P, N) on the CPU.
    The index rows past a count point at row `index_fill`, the workspace starts as 0x55 bytes and the outputs as 77."""
    from shapegen_amd import _lib
    points, counts = K.pack(clouds)
    index = K.pack_rows(tables, k, index_fill, torch.int32)
    dp, dc, di = points.cuda(), counts.cuda(), index.cuda()
    P, N = dp.shape[0], dp.shape[1]
    need = lib.pcd_cloud_normals_workspace_bytes(P)
    ws = torch.full((need,), 0x55, dtype=torch.uint8, device="cuda")
    normals = torch.full((P, N, 3), 77.0, device="cuda")
    curv = torch.full((P, N), 77.0, device="cuda") if curvature else None
    dv = view.cuda() if view is not None else None
    _lib.check(lib.pcd_cloud_normals(dp.data_ptr(), dc.data_ptr(), N, P, di.data_ptr(), k, mode, _lib.ptr(dv), normals.data_ptr(), _lib.ptr(curv),
                                     ws.data_ptr(), need, _lib.stream_ptr()), "cloud_normals")
    return normals.cpu(), (curv.cpu() if curvature else None)


@pytest.fixture(scope="module")
def surface_runs(lib):
    done = {}

    def get(k, mode=0):
        if (k, mode) not in done:
            view = VIEW[None, :].expand(len(K.SURFACES), 3).contiguous() if mode == 2 else None
            done[k, mode] = run_normals(lib, [x for x, _ in K.surfaces()], [s["index"] for s in K.surface_statements(k)], k, mode, view)
        return done[k, mode]
    return get


VIEW = torch.tensor([0.3, -2.0, 1.5])


@pytest.mark.parametrize("k", K.SURFACE_KS)
def test_normals_and_curvature_against_the_fp64_statement(surface_runs, k, capsys):
    normals, curv = surface_runs(k)
    sine_row, curv_row = [], []
    for i, ((kind, n), s) in enumerate(zip(K.SURFACES, K.surface_statements(k))):
        r = s["normals"]
        got = normals[i, :n].double()
        length = got.norm(dim=1)
        assert bool(((length - 1).abs() <= NORM_BOUND).all()), (kind, n, k, float((length - 1).abs().max()) / U)
        use = r["gap"] >= K.GAP_MIN
        assert float((~use).double().mean()) <= K.GAP_SHARE
        sine = torch.linalg.cross(got / length[:, None], r["normal"]).norm(dim=1)
        sine_row.append(float((sine * r["gap"])[use].max()) / U)
        curv_row.append(float((curv[i, :n].double() - r["curvature"]).abs().max()) / U)
        assert bool((normals[i, n:] == 0).all()) and torch.isnan(curv[i, n:]).all(), (kind, n, k, "padding")
    with capsys.disabled():
        print(f"\n[normals] k = {k:2d}: sine x gap " + "  ".join(f"{v:7.3f}" for v in sine_row)
              + "   |c - c64| " + "  ".join(f"{v:7.3f}" for v in curv_row) + "   (units of 2^-24)")
    assert max(sine_row) <= SINE_GAP_BOUND, sine_row
    assert max(curv_row) <= CURVATURE_BOUND, curv_row


def test_short_neighbourhoods_and_padding_follow_the_statement(lib):
    """Fewer than 3 members: a zero normal and a NaN curvature, exactly; every other row a unit vector (also where the two smallest
    eigenvalues meet, as in the doubled clouds and on the lattice); rows past a count zero / NaN."""
    for name in ("tiny", "non_finite", "doubled", "lattice"):
        clouds = K.self_case(name)
        tables = [index[:, :16].contiguous() for _, index in K.self_statements(name)]
        normals, curv = run_normals(lib, clouds, tables, 16, mode=1)
        for i, (x, table) in enumerate(zip(clouds, tables)):
            n = x.shape[0]
            r = G.normals(x, table)
            none = (r["normal"] == 0).all(dim=1)
            assert bool((r["members"][none] < 3).all())
            assert bool((normals[i, :n][none] == 0).all()) and torch.isnan(curv[i, :n][none]).all(), (name, i)
            length = normals[i, :n][~none].double().norm(dim=1)
            assert bool(((length - 1).abs() <= NORM_BOUND).all()), (name, i)
            assert same(torch.isnan(curv[i, :n]), torch.isnan(r["curvature"])), (name, i)
            ok = ~torch.isnan(r["curvature"])
            assert bool(((curv[i, :n][ok].double() - r["curvature"][ok]).abs() <= CURVATURE_BOUND * U).all()), (name, i)
            assert bool((normals[i, n:] == 0).all()) and torch.isnan(curv[i, n:]).all(), (name, i, "padding")


@pytest.mark.parametrize("k", [16])
def test_orientation(surface_runs, k):
    plain, _ = surface_runs(k, 0)
    outward, _ = surface_runs(k, 1)
    toward, _ = surface_runs(k, 2)
    for i, ((kind, n), (x, ref)) in enumerate(zip(K.SURFACES, K.surfaces())):
        n0, n1, n2 = plain[i, :n], outward[i, :n], toward[i, :n]
        # mode 0 against the oriented ones: the same bits up to the sign of the whole vector
        flips = []
        for other in (n1, n2):
            flips.append((other != n0).any(dim=1))
            assert torch.equal(torch.where(flips[-1][:, None], -other, other), n0), (kind, n)
        _, dot1 = G.oriented(n1.double(), x, 1)
        _, dot2 = G.oriented(n2.double(), x, 2, VIEW)
        for dot in (dot1, dot2):
            decided = dot.abs() > 1e-4
            assert int(decided.sum()) > n // 2 and bool((dot[decided] > 0).all()), (kind, n)
        if kind == "sphere":
            assert bool(((n1.double() * ref).sum(dim=1) > 0.9).all())          # outward on a sphere: along the radius
            assert bool(flips[0].any())                                         # the unoriented signs were not all outward already


# ------------------------------------------------------------------ 3. stage (c), the masks
def run_mask(lib, tables, k, method, ratio=2.0, radius=0.0, min_neighbors=1):
    """One `pcd_cloud_outlier_mask` call on ragged (n_i, k) fp32 tables; the d2 rows past a count are 0 (a neighbour at distance 0), the
    outputs start as 77."""
    from shapegen_amd import _lib
    d2 = K.pack_rows(tables, k, 0.0, torch.float32).cuda()
    counts = torch.tensor([t.shape[0] for t in tables], dtype=torch.int32).cuda()
    P, N = d2.shape[0], d2.shape[1]
    mask = torch.full((P, N), 77, dtype=torch.uint8, device="cuda")
    dbar = torch.full((P, N), 77.0, device="cuda")
    _lib.check(lib.pcd_cloud_outlier_mask(d2.data_ptr(), counts.data_ptr(), N, P, k, method, ratio, radius, min_neighbors, mask.data_ptr(),
                                          dbar.data_ptr(), _lib.stream_ptr()), "cloud_outlier_mask")
    return mask.cpu(), dbar.cpu()


def ulps(x, y):
    """|x - y| in units of the fp32 spacing at y"""
    spacing = (torch.nextafter(y.abs(), torch.full_like(y, float("inf"))) - y.abs()).double()
    return (x.double() - y.double()).abs() / spacing


@pytest.mark.parametrize("name", ["surfaces_k8", "surfaces_k16", "surfaces_k32", "sphere_outliers", "small", "non_finite", "doubled"])
def test_statistical_mask_and_mean_distance(lib, name):
    k, clouds, tables = K.outlier_batches()[name]
    for ratio in K.OUTLIER_RATIOS:
        mask, dbar = run_mask(lib, tables, k, 0, ratio=ratio)
        for i, d2 in enumerate(tables):
            n = d2.shape[0]
            s = G.outlier_statistical(d2, ratio)
            want = s["dbar"].float()
            have = ~torch.isnan(want)
            assert same(torch.isnan(dbar[i, :n]), ~have), (name, i)
            assert bool((ulps(dbar[i, :n][have], want[have]) <= 1).all()), (name, i)
            if bool(have.any()):
                outside = ~have | ((s["dbar"] - s["limit"]).abs() > K.BAND * s["limit"])
                assert bool(outside.all()), (name, i, "the band is not empty")
            assert torch.equal(mask[i, :n], s["mask"]), (name, i, ratio)
            assert bool((mask[i, n:] == 0).all()) and torch.isnan(dbar[i, n:]).all(), (name, i, "padding")


@pytest.mark.parametrize("name", ["surfaces_k16", "sphere_outliers", "small", "non_finite", "doubled"])
def test_radius_mask_is_bit_exact(lib, name):
    k, clouds, tables = K.outlier_batches()[name]
    kept = 0
    for radius, need in K.RADII:
        mask, _ = run_mask(lib, tables, k, 1, radius=radius, min_neighbors=need)
        for i, d2 in enumerate(tables):
            n = d2.shape[0]
            want = G.outlier_radius(d2, radius, need)
            assert torch.equal(mask[i, :n], want) and bool((mask[i, n:] == 0).all()), (name, i, radius, need)
            kept += int(want.sum())
    assert kept > 0 or name == "small"


# ------------------------------------------------------------------ 4. stage (d), the compaction
def run_compact(lib, clouds, masks, attrs=None):
    from shapegen_amd import _lib
    points, counts = K.pack(clouds)
    N = points.shape[1]
    mask = torch.ones(len(clouds), N, dtype=torch.uint8)                      # the mask bytes past a count are set: they must not count
    for i, m in enumerate(masks):
        mask[i, :m.shape[0]] = m
    attr = K.pack(attrs)[0] if attrs is not None else None
    dp, dm, dc = points.cuda(), mask.cuda(), counts.cuda()
    da = attr.cuda() if attr is not None else None
    out = torch.full_like(dp, 77.0)
    aout = torch.full_like(dp, 77.0) if attr is not None else None
    kept = torch.full((len(clouds),), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.pcd_cloud_compact(dp.data_ptr(), _lib.ptr(da), dm.data_ptr(), dc.data_ptr(), N, len(clouds), out.data_ptr(), _lib.ptr(aout),
                                     kept.data_ptr(), _lib.stream_ptr()), "cloud_compact")
    return out.cpu(), (aout.cpu() if aout is not None else None), kept.cpu()


@pytest.mark.parametrize("with_attr", [False, True])
def test_compaction_is_bit_exact(lib, with_attr):
    clouds = K.self_case("edges") + K.self_case("tiny")
    g = torch.Generator().manual_seed(12)
    masks = [(torch.rand(x.shape[0], generator=g) < 0.7).to(torch.uint8) * 3 for x in clouds]      # any byte != 0 keeps
    masks[2] = torch.ones_like(masks[2])                                       # 257 rows, all kept
    masks[4] = torch.zeros_like(masks[4])                                      # 512 rows, all dropped
    attrs = [torch.randn(x.shape[0], 3, generator=g) for x in clouds] if with_attr else None
    out, aout, kept = run_compact(lib, clouds, masks, attrs)
    N = out.shape[1]
    for i, (x, m) in enumerate(zip(clouds, masks)):
        want, want_attr, count = G.compact(x, m, attrs[i] if with_attr else None, rows=N)
        assert int(kept[i]) == count and same(out[i], want), i
        if with_attr:
            assert same(aout[i], want_attr), i
    assert int(kept[2]) == 257 and int(kept[4]) == 0 and bool((out[4] == 0).all())


# ------------------------------------------------------------------ 5. end to end
def test_remove_outliers_returns_the_sphere(lib):
    from shapegen_amd import geometry
    x, flag = K.sphere_with_outliers()
    nrm = torch.randn(x.shape[0], 3, generator=torch.Generator().manual_seed(2))
    out, counts, out_n, mask = geometry.remove_outliers(x[None].cuda(), k=16, std_ratio=2.0, normals=nrm[None].cuda(), return_mask=True)
    assert counts.dtype == torch.int32 and counts.tolist() == [1024]
    assert torch.equal(out[0, :1024].cpu(), x[~flag]) and bool((out[0, 1024:] == 0).all())
    assert torch.equal(out_n[0, :1024].cpu(), nrm[~flag]) and torch.equal(mask[0].cpu().bool(), ~flag)
    # ragged lists, the radius rule: an outlier is 0.7 or more from the sphere, and a disc of radius 0.4 holds ~ 70 (~ 19) of the sphere's points
    other, _ = K.sphere(300, 77)
    out, counts = geometry.remove_outliers([x.cuda(), other.cuda()], k=16, radius=0.4, min_neighbors=4)
    assert counts.tolist() == [1024, 300] and torch.equal(out[0, :1024].cpu(), x[~flag]) and torch.equal(out[1, :300].cpu(), other)
    assert bool((out[1, 300:] == 0).all())


def uv_sphere(radius=0.8, rings=16, segments=24):
    """A closed latitude / longitude sphere about the origin as a device `Mesh`."""
    from shapegen_amd.utils import Mesh
    v = [(0.0, 0.0, 1.0)]
    for r in range(1, rings):
        th = np.pi * r / rings
        v += [(np.sin(th) * np.cos(2 * np.pi * s / segments), np.sin(th) * np.sin(2 * np.pi * s / segments), np.cos(th)) for s in range(segments)]
    v.append((0.0, 0.0, -1.0))
    ring = lambda r, s: 1 + (r - 1) * segments + s % segments                  # noqa: E731
    f = []
    for s in range(segments):
        f.append((0, ring(1, s), ring(1, s + 1)))
        f.append((len(v) - 1, ring(rings - 1, s + 1), ring(rings - 1, s)))
        for r in range(1, rings - 1):
            f.append((ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)))
            f.append((ring(r, s), ring(r + 1, s + 1), ring(r, s + 1)))
    return Mesh(torch.from_numpy((np.asarray(v) * radius).astype(np.float32)).cuda(), torch.from_numpy(np.asarray(f, np.int32)).cuda())


def test_estimated_normals_give_a_normal_consistency(lib):
    """`surface_metrics` of samples of a sphere mesh with `estimate_normals` on side a and the face normals on side b: NC is finite (it is NaN
    without normals) and is the statement's for the same inputs -- every term |n . n'| moves by at most the sine between the kernel's and
    the statement's normal, bounded at stage (b) by SINE_GAP_BOUND 2^-24 / gap with gap >= 0.1 for every point here, plus the roundings of
    an fp32 dot product of unit vectors."""
    from shapegen_amd import geometry, metrics as M
    from shapegen_amd.utils import sample_mesh_points
    mesh = uv_sphere()
    pa = sample_mesh_points([mesh], 1024, seed=5)
    pb, nb = sample_mesh_points([mesh], 1024, seed=6, return_normals=True)
    na, curv = geometry.estimate_normals(pa, k=16, orient="outward", return_curvature=True)
    assert na.shape == pa.shape and curv.shape == pa.shape[:2]
    rows = M.surface_metrics(pa, pb, na, nb, thresholds=()).cpu()
    bare = M.surface_metrics(pa, pb, thresholds=()).cpu()
    nc = [S.NC_A, S.NC_B, S.NC]
    assert torch.isnan(bare[0, nc]).all() and torch.isfinite(rows[0, nc]).all()
    a, b = pa[0].cpu(), pb[0].cpu()
    r = G.normals(a, G.knn(a, a, 16, True)[1])
    assert bool((r["gap"] >= K.GAP_MIN).all())
    want = S.row(a, b, r["normal"], nb[0].cpu(), (), torch.float64)["row"]
    tol = (SINE_GAP_BOUND / K.GAP_MIN + 8) * U
    for col in nc:
        assert abs(float(rows[0, col]) - float(want[col])) <= tol, (S.ROW[col], float(rows[0, col]), float(want[col]))
    assert float(rows[0, S.NC]) > 0.95                                          # PCA normals of a sphere against its facets
    assert bool(((na[0].cpu().double() * a.double()).sum(dim=1) > 0).all())     # outward


def test_remove_outliers_replays_from_a_graph(lib):
    """A capture of `remove_outliers` (no hidden synchronisation, nothing read back) replays to the bits of the eager call, also after the
    input buffer has been refilled."""
    from shapegen_amd import geometry
    x, flag = K.sphere_with_outliers()
    y, _ = K.sphere_with_outliers(seed=47)
    static = x[None].cuda().clone()
    eager_x = [v.clone() for v in geometry.remove_outliers(static, return_mask=True)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        geometry.remove_outliers(static, return_mask=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = geometry.remove_outliers(static, return_mask=True)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(out, eager_x):
        assert same(got.cpu(), want.cpu())
    static.copy_(y[None].cuda())
    graph.replay()
    torch.cuda.synchronize()
    eager_y = geometry.remove_outliers(y[None].cuda(), return_mask=True)
    for got, want in zip(out, eager_y):
        assert same(got.cpu(), want.cpu())
    assert out[1].tolist() == [1024]
