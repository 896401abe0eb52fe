"""The surface-metric kernels (csrc/surface_metrics.hip) against the CPU statement of tests/surface_statement.py.  GPU only.

  * Stage (a), the nearest neighbour with its index, must equal the fp32 statement bit for bit in both directions, at every edge of the
    launch shape (tests/surface_cases.py states it), with the lowest index on ties.
  * HAUSDORFF, PRECISION / RECALL / FSCORE, the IoU, and CHAMFER_L1 / CHAMFER_L2 / NC given their two halves must equal the fp32 statement
    bit for bit.  HAUSDORFF relies on a correctly rounded sqrtf: the build's default, and the disassembly of surf_rows_kernel shows the
    v_sqrt_f32 with its fma correction sequence.
  * The six means (ACC, COMP, ACC2, COMP2, NC_A, NC_B) are held to the fp64 statement at 4 x 2^-24 relative: one rounding of each fp32
    term, an effectively exact double sum, one division, one final rounding; both statements start from the same stage-(a) values.

Measured on an MI355X: the worst |kernel - fp64 statement| / |fp64 statement| of each mean per case, in units of 2^-24 (bound 4):
    case               ACC    COMP   ACC2   COMP2  NC_A   NC_B
    edges_split        0.66   0.40   0.42   0.73   0.94   0.95
    edges_one_split    1.16   1.32   0.99   0.97   2.44   1.83
    one_pair_split     0.34   0.06   0.50   0.72   0.50   0.35
    ragged             0.63   0.29   0.95   0.59   0.71   0.56
    many_tiny          1.26   1.35   0.99   0.99   2.85   3.55
The two cases above 1 are the ones with pairs of 2 to 8 points, where the roundings of so few terms do not cancel.  The NC terms are fp32
dot products of unit normals, up to five roundings a term."""
import numpy as np
import pytest
import torch

import mesh_in_statement as MS
import surface_cases as K
import surface_statement as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MEAN_REL = 4 * 2.0 ** -24
NC_COLS = [S.NC_A, S.NC_B, S.NC]


@pytest.fixture(scope="module")
def lib():
    from shapegen_amd import _lib
    _lib.require_gpu()
    return _lib.load()


def cube(lo, hi):
    """`mesh_in_statement.cube` as a device `Mesh`."""
    from shapegen_amd.utils import Mesh
    v, f = MS.cube(lo, hi)
    return Mesh(torch.from_numpy(np.asarray(v, np.float32)).cuda(), torch.from_numpy(np.asarray(f, np.int32)).cuda())


def same(x, y):
    """Bit-for-bit equality of two tensors, a NaN equal to a NaN."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if not x.dtype.is_floating_point:
        return torch.equal(x, y)
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=5.0), torch.nan_to_num(y, nan=5.0))


def run_surface(lib, a, b, ka=None, kb=None, thresholds=K.THRESHOLDS):
    """One `pcd_surface_metrics` call on ragged lists; -> rows and the stage-(a) outputs of both directions, on the CPU.  Padding rows hold
    copies of the pair's other cloud, the workspace starts as 0x55 bytes and the outputs as 77 / -7, so nothing unwritten passes."""
    import ctypes as C
    from shapegen_amd import _lib
    pa, na = K.pack(a, b)
    pb, nb = K.pack(b, a)
    P, NA, NB = len(a), pa.shape[1], pb.shape[1]
    na_dev, nb_dev = na.cuda(), nb.cuda()
    da, db = pa.cuda(), pb.cuda()
    normals = [K.pack(k)[0].cuda() if k is not None else None for k in (ka, kb)]
    need = lib.pcd_surface_metrics_workspace_bytes(P, NA, NB)
    ws = torch.full((need,), 0x55, dtype=torch.uint8, device="cuda")
    rows = torch.full((P, S.BASE + 3 * len(thresholds)), 77.0, device="cuda")
    d2_a, d2_b = torch.full((P, NA), 77.0, device="cuda"), torch.full((P, NB), 77.0, device="cuda")
    index_a = torch.full((P, NA), -7, dtype=torch.int32, device="cuda")
    index_b = torch.full((P, NB), -7, dtype=torch.int32, device="cuda")
    taus = (C.c_float * max(1, len(thresholds)))(*thresholds)
    _lib.check(lib.pcd_surface_metrics(da.data_ptr(), _lib.ptr(normals[0]), na_dev.data_ptr(), NA, db.data_ptr(), _lib.ptr(normals[1]),
                                       nb_dev.data_ptr(), NB, P, taus, len(thresholds), rows.data_ptr(), d2_a.data_ptr(), index_a.data_ptr(),
                                       d2_b.data_ptr(), index_b.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), "surface_metrics")
    return dict(rows=rows.cpu(), d2_a=d2_a.cpu(), index_a=index_a.cpu(), d2_b=d2_b.cpu(), index_b=index_b.cpu(), na=na, nb=nb)


@pytest.fixture(scope="module")
def runs(lib):
    """One call per case of surface_cases.CASES, made when first asked for and shared by the stage-(a) and the row tests."""
    done = {}

    def get(name):
        if name not in done:
            a, b, ka, kb = K.case(name)
            done[name] = run_surface(lib, a, b, ka, kb)
        return done[name]
    return get


def check_stage_a(got, want, n, m, where):
    """d2 / index of both directions equal the fp32 statement; the rows past a count hold (NaN, -1)."""
    for side, count in (("a", n), ("b", m)):
        d2, index = got["d2_" + side], got["index_" + side]
        assert same(d2[:count], want["d2_" + side]), (where, side, "d2")
        assert torch.equal(index[:count], want["index_" + side]), (where, side, "index")
        assert torch.isnan(d2[count:]).all() and (index[count:] == -1).all(), (where, side, "padding")


# ------------------------------------------------------------------ 1. stage (a), bit for bit
@pytest.mark.parametrize("name", list(K.CASES))
def test_nearest_neighbours_are_bit_exact_in_both_directions(runs, name):
    a, b, _, _ = K.case(name)
    r = runs(name)
    for i, (s32, _) in enumerate(K.statements(name)):
        got = {k: r[k][i] for k in ("d2_a", "index_a", "d2_b", "index_b")}
        check_stage_a(got, s32, a[i].shape[0], b[i].shape[0], (name, i))
        if a[i].shape[0] and b[i].shape[0]:
            assert (s32["index_a"] >= 0).all() and (s32["index_b"] >= 0).all()


@pytest.mark.parametrize("name", ["edges_split", "ragged", "many_tiny", "single"])
def test_nearest_neighbors_entry_equals_the_statement(lib, name):
    """`metrics.nearest_neighbors` (jobs = P, its own split count) on padded tensors with counts, and on ragged lists."""
    from shapegen_amd import metrics as M
    a, b, _, _ = K.case(name)
    pa, na = K.pack(a, b)
    pb, nb = K.pack(b, a)
    d2, index = (t.cpu() for t in M.nearest_neighbors(pa.cuda(), pb.cuda(), na.cuda(), nb.cuda()))
    l2, lindex = (t.cpu() for t in M.nearest_neighbors([x.cuda() for x in a], [y.cuda() for y in b]))
    assert same(d2, l2) and torch.equal(index, lindex)
    for i, (s32, _) in enumerate(K.statements(name)):
        n = a[i].shape[0]
        assert same(d2[i, :n], s32["d2_a"]) and torch.equal(index[i, :n], s32["index_a"]), (name, i)
        assert torch.isnan(d2[i, n:]).all() and (index[i, n:] == -1).all(), (name, i)


# ------------------------------------------------------------------ 2. ties and the threshold boundary
def test_ties_go_to_the_lowest_index_and_the_boundary_counts(lib):
    a, b, ka, kb = K.lattice_case()
    taus = (0.25, 0.125, 0.36)
    s32 = S.row(a, b, ka, kb, taus)
    d2 = S.sq_dists(a, b)
    tied = (d2 == s32["d2_a"][:, None]).sum(dim=1)
    assert int((tied > 1).sum()) >= 1, "the case holds no tie"
    on = int((s32["d2_a"] == 0.0625).sum()) + int((s32["d2_b"] == 0.0625).sum())
    assert on >= 1 and 0.25 * 0.25 == 0.0625, "the case holds no query exactly on the threshold 0.25"
    r = run_surface(lib, [a], [b], [ka], [kb], taus)
    check_stage_a({k: r[k][0] for k in ("d2_a", "index_a", "d2_b", "index_b")}, s32, a.shape[0], b.shape[0], "lattice")
    row = r["rows"][0]
    for k, (ca, cb) in enumerate(s32["within"]):
        assert round(float(row[S.BASE + 3 * k]) * a.shape[0]) == ca and round(float(row[S.BASE + 3 * k + 1]) * b.shape[0]) == cb, (k, ca, cb)
    assert 0 < s32["within"][1][0] < s32["within"][0][0] < s32["within"][2][0]       # 0.125: coincident only; 0.25: + axis neighbours; 0.36: + diagonals
    assert same(row[S.BASE:], s32["row"][S.BASE:])


# ------------------------------------------------------------------ 3. rows
def check_row(got, s32, s64, where, worst=None):
    want32, want64 = s32["row"], s64["row"]
    if torch.isnan(want32).all():
        assert torch.isnan(got).all(), (where, "NaN row")
        return
    for col in S.MEANS:
        rel = abs(float(got[col]) - float(want64[col])) / abs(float(want64[col])) if float(want64[col]) != 0 else abs(float(got[col]))
        if worst is not None:
            worst[col] = max(worst.get(col, 0.0), rel / 2.0 ** -24)
        assert rel <= MEAN_REL, (where, S.ROW[col], float(got[col]), float(want64[col]), rel / 2.0 ** -24)
    # the derived columns from the KERNEL's halves, and the order-free ones, bit for bit
    far2 = torch.maximum(s32["d2_a"].max(), s32["d2_b"].max())
    want = S.derived(got, far2, s32["within"], s32["d2_a"].shape[0], s32["d2_b"].shape[0])
    for col in [S.CHAMFER_L1, S.CHAMFER_L2, S.NC, S.HAUSDORFF] + list(range(S.BASE, got.shape[0])):
        assert same(got[col], want[col]), (where, col, float(got[col]), float(want[col]))
    assert same(got[S.HAUSDORFF], want32[S.HAUSDORFF]) and same(got[S.BASE:], want32[S.BASE:]), where


@pytest.mark.parametrize("name", list(K.CASES))
def test_rows(runs, name, capsys):
    r = runs(name)
    worst = {}
    for i, (s32, s64) in enumerate(K.statements(name)):
        check_row(r["rows"][i], s32, s64, (name, i), worst)
    with capsys.disabled():
        print(f"\n[surface rows] {name}: worst |kernel - fp64| / |fp64| in units of 2^-24: "
              + "  ".join(f"{S.ROW[c]} {v:.2f}" for c, v in sorted(worst.items())))


def test_python_surface_metrics_equals_the_entry_point(lib, runs):
    """`metrics.surface_metrics` on ragged lists (zero padding) and on a dense tensor gives the rows of the poisoned-padding call."""
    from shapegen_amd import metrics as M
    a, b, ka, kb = K.case("ragged")
    cuda = lambda xs: [x.cuda() for x in xs]
    rows = M.surface_metrics(cuda(a), cuda(b), cuda(ka), cuda(kb), K.THRESHOLDS).cpu()
    assert same(rows, runs("ragged")["rows"])
    bare = M.surface_metrics(cuda(a), cuda(b), thresholds=K.THRESHOLDS).cpu()
    keep = [c for c in range(rows.shape[1]) if c not in NC_COLS]
    assert torch.isnan(bare[:, NC_COLS]).all() and same(bare[:, keep], rows[:, keep])
    dense = M.surface_metrics(a[4][None].cuda(), b[4][None].cuda(), ka[4][None].cuda(), kb[4][None].cuda(), K.THRESHOLDS).cpu()
    assert same(dense[0], rows[4])
    none = M.surface_metrics(a[4][None].cuda(), b[4][None].cuda(), thresholds=()).cpu()
    assert none.shape == (1, S.BASE) and same(none[0, keep[:7]], rows[4, keep[:7]])


# ------------------------------------------------------------------ 4. planes
def square(z=0.0, axis=2):
    """The unit square [0, 1]^2 as two triangles, in the plane `axis` = z."""
    flat = torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    v = torch.full((4, 3), float(z))
    v[:, [k for k in range(3) if k != axis]] = flat
    from shapegen_amd.utils import Mesh
    return Mesh(v.cuda(), torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32).cuda())


def test_parallel_and_perpendicular_planes(lib):
    from shapegen_amd import metrics as M
    delta, taus = 0.125, (0.1, 0.5)
    cols = M.mesh_columns(taus)
    rows, smp = M.mesh_metrics([square(0.0), square(0.0)], [square(delta), square(0.5, axis=0)], num_points=2000, thresholds=taus,
                               iou_resolution=None, return_samples=True)
    rows = rows.cpu()
    par = dict(zip(cols, rows[0].tolist()))
    assert par["NC"] == 1.0 and par["NC_A"] == 1.0 and par["NC_B"] == 1.0
    assert par["ACC"] >= delta and par["COMP"] >= delta and par["HAUSDORFF"] >= delta and par["CHAMFER_L1"] >= delta
    assert par["PRECISION@0.1"] == 0.0 and par["RECALL@0.1"] == 0.0 and par["FSCORE@0.1"] == 0.0
    assert par["PRECISION@0.5"] == 1.0 and par["RECALL@0.5"] == 1.0 and par["FSCORE@0.5"] == 1.0
    perp = dict(zip(cols, rows[1].tolist()))
    assert perp["NC"] == 0.0 and perp["NC_A"] == 0.0 and perp["NC_B"] == 0.0
    assert torch.isnan(rows[:, -1]).all()                                   # iou_resolution=None
    # the same samples without normals: NC columns NaN, the rest the same bits
    bare = M.surface_metrics(smp["points_a"], smp["points_b"], thresholds=taus).cpu()
    keep = [c for c in range(bare.shape[1]) if c not in NC_COLS]
    assert torch.isnan(bare[:, NC_COLS]).all() and same(bare[:, keep], rows[:, :-1][:, keep])


# ------------------------------------------------------------------ 5. non-finite and empty
def test_non_finite_and_empty_pairs(lib):
    from shapegen_amd import metrics as M
    from shapegen_amd.utils import Mesh
    a, b, ka, kb = (list(t[:3]) for t in K.case("many_tiny"))
    a[0], b[1] = a[0].clone(), b[1].clone()
    a[0][1, 2] = float("nan")
    b[1][0, 1] = float("inf")
    r = run_surface(lib, a, b, ka, kb)
    alone = run_surface(lib, a[2:], b[2:], ka[2:], kb[2:])
    assert torch.isnan(r["rows"][:2]).all() and torch.isfinite(r["rows"][2]).all()
    assert same(r["rows"][2], alone["rows"][0])
    d2, index = (t.cpu() for t in M.nearest_neighbors([x.cuda() for x in a], [y.cuda() for y in b]))
    assert torch.isnan(d2[0, 1]) and index[0, 1] == -1                       # the NaN query
    others = [i for i in range(a[0].shape[0]) if i != 1]
    assert torch.isfinite(d2[0, others]).all() and (index[0, others] >= 0).all()
    assert (index[1, :a[1].shape[0]] != 0).all() and (index[1, :a[1].shape[0]] >= 0).all()    # never the infinite target
    for i in range(3):
        s_d2, s_index = S.nearest(a[i], b[i])
        n = a[i].shape[0]
        assert same(d2[i, :n], s_d2) and torch.equal(index[i, :n], s_index), i
    back, back_index = (t.cpu() for t in M.nearest_neighbors([b[1].cuda()], [a[1].cuda()]))
    assert torch.isnan(back[0, 0]) and back_index[0, 0] == -1               # the infinite point as a query
    all_bad = torch.full((4, 3), float("inf"))
    d2, index = (t.cpu() for t in M.nearest_neighbors([a[2].cuda()], [all_bad.cuda()]))
    assert torch.isnan(d2).all() and (index == -1).all()
    # a faceless mesh in mesh_metrics: a NaN row, its neighbours' rows those of the call without it
    cubes = [cube((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), cube((-0.25, -0.5, 0.0), (0.5, 0.25, 0.75))]
    empty = Mesh(torch.zeros(0, 3).cuda(), torch.zeros(0, 3, dtype=torch.int32).cuda())
    kw = dict(num_points=500, iou_resolution=16)
    with_empty = M.mesh_metrics([cubes[0], empty, cubes[1], cubes[0]], [cubes[1], cubes[0], cubes[0], empty], **kw).cpu()
    without = M.mesh_metrics([cubes[0], cubes[1]], [cubes[1], cubes[0]], **kw).cpu()
    assert torch.isnan(with_empty[[1, 3]]).all() and torch.isfinite(without).all()
    assert same(with_empty[[0, 2]], without)


# ------------------------------------------------------------------ 6. repeatability and batch independence
def test_repeatable_and_independent_of_the_batch(lib):
    a, b, ka, kb = K.case("ragged")
    pick = [4, 0, 3, 2, 1, 4, 3]
    batch = [[t[i] for i in pick] for t in (a, b, ka, kb)]
    first, second = run_surface(lib, *batch), run_surface(lib, *batch)
    for k in ("rows", "d2_a", "index_a", "d2_b", "index_b"):
        assert same(first[k], second[k]), k
    for slot, i in enumerate(pick):
        alone = run_surface(lib, [a[i]], [b[i]], [ka[i]], [kb[i]])           # P = 1: another split count than in the batch of 7
        assert same(first["rows"][slot], alone["rows"][0]), (slot, i)
        n, m = a[i].shape[0], b[i].shape[0]
        assert same(first["d2_a"][slot, :n], alone["d2_a"][0, :n]) and torch.equal(first["index_b"][slot, :m], alone["index_b"][0, :m])


# ------------------------------------------------------------------ 7. IoU
def test_voxel_iou(lib):
    from shapegen_amd import metrics as M
    from shapegen_amd.utils import meshes_to_voxel_tensor
    g = torch.Generator().manual_seed(5)
    for side in (8, 33):
        x, y = torch.rand(5, 1, side, side, side, generator=g), torch.rand(5, 1, side, side, side, generator=g)
        x[3], y[3] = 0.0, 0.25                                                # an empty union
        x[4] = y[4]
        for thr in (0.5, 0.9):
            got = M.voxel_iou(x.cuda(), y.cuda(), thr).cpu()
            want = torch.stack([S.iou(x[i], y[i], thr) for i in range(5)])
            assert same(got, want), (side, thr)
            assert torch.isnan(got[3]) and got[4] == 1.0
    big, small = cube((-0.75, -0.75, -0.75), (0.75, 0.75, 0.75)), cube((-0.25, -0.25, -0.25), (0.25, 0.5, 0.25))
    left, right = cube((-0.75, -0.5, -0.5), (-0.25, 0.5, 0.5)), cube((0.25, -0.5, -0.5), (0.75, 0.5, 0.5))
    ma, mb = [big, left, big], [small, right, big]                            # nested, disjoint, identical
    for res, fill in ((32, "solid"), (16, "surface")):
        rows = M.mesh_metrics(ma, mb, num_points=500, iou_resolution=res, iou_fill=fill).cpu()
        ga, gb = meshes_to_voxel_tensor(ma, res, fill).cpu(), meshes_to_voxel_tensor(mb, res, fill).cpu()
        want = torch.stack([S.iou(ga[i], gb[i]) for i in range(3)])
        assert same(rows[:, -1], want), (res, fill)
        assert rows[1, -1] == 0.0 and rows[2, -1] == 1.0
        assert 0.0 < rows[0, -1] < 1.0 if fill == "solid" else rows[0, -1] == 0.0      # nested surfaces do not touch


# ------------------------------------------------------------------ 8. mesh_metrics(return_samples=True)
def test_mesh_metrics_returns_its_samples(lib):
    from shapegen_amd import metrics as M
    from shapegen_amd.utils import sample_mesh_points
    ma = [cube((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), cube((-0.75, -0.25, -0.5), (0.25, 0.5, 0.5))]
    mb = [cube((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), cube((-0.5, -0.5, -0.25), (0.5, 0.5, 0.75))]
    taus = (0.05, 0.2)
    rows, smp = M.mesh_metrics(ma, mb, num_points=1500, thresholds=taus, seed=11, iou_resolution=16, return_samples=True)
    assert smp["keep"] == [0, 1] and rows.shape == (2, S.BASE + 6 + 1)
    pa, na = sample_mesh_points(ma, 1500, seed=11, return_normals=True)
    pb, nb = sample_mesh_points(mb, 1500, seed=12, return_normals=True)
    for key, want in (("points_a", pa), ("normals_a", na), ("points_b", pb), ("normals_b", nb)):
        assert same(smp[key].cpu(), want.cpu()), key
    again = M.surface_metrics(smp["points_a"], smp["points_b"], smp["normals_a"], smp["normals_b"], taus)
    assert same(rows[:, :-1].cpu(), again.cpu())
    assert not same(pa[0].cpu(), pb[0].cpu())                                 # a mesh against itself: other draws
    row = dict(zip(M.mesh_columns(taus), rows[0].tolist()))
    assert row["IOU"] == 1.0 and row["FSCORE@0.2"] == 1.0 and 0.0 < row["ACC"] < 0.05
