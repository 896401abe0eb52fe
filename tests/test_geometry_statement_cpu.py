"""tests/geometry_statement.py against itself, against geometry and against cases worked out by hand; the conditions the GPU tests rely on
(tests/geometry_cases.py); the PLY cloud files; and the argument checks of shapegen_amd.geometry.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

import geometry_cases as K
import geometry_statement as G

NAN = float("nan")


def angles_deg(n, ref):
    """The angle between two direction fields up to sign, in degrees, through the sine (the cosine has no digits left near 0)."""
    sine = torch.linalg.cross(n, ref).norm(dim=1).clamp(max=1.0)
    return torch.rad2deg(torch.asin(sine))


# ------------------------------------------------------------------ (a) k nearest
def test_knn_by_hand():
    """Five points on a line at 0, 1, 3, 3, 7: ties by index, the own row excluded but not the duplicate, NaN padding past the candidates."""
    x = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    for dt in (torch.float32, torch.float64):
        d2, index = G.knn(x, x, 3, True, dt)
        assert d2.dtype == dt and index.dtype == torch.int32
        assert index.tolist() == [[1, 2, 3], [0, 2, 3], [3, 1, 0], [2, 1, 0], [2, 3, 1]]
        assert d2.tolist() == [[1, 9, 9], [1, 4, 4], [0, 4, 9], [0, 4, 9], [16, 16, 36]]
        d2, index = G.knn(x, x, 6, True, dt)
        assert index[0].tolist() == [1, 2, 3, 4, -1, -1] and torch.isnan(d2[0, 4:]).all() and d2[0, 3] == 49
        d2, index = G.knn(x, x, 2, False, dt)                                  # no exclusion: every point finds itself first ...
        assert index[:, 0].tolist() == [0, 1, 2, 2, 4] and index[3].tolist() == [2, 3]      # ... but the duplicate's lower index wins the tie
    d2, index = G.knn(x[:0], x, 2)
    assert d2.shape == (0, 2)
    d2, index = G.knn(x, x[:0], 2)
    assert torch.isnan(d2).all() and (index == -1).all()


def test_knn_non_finite():
    x = torch.tensor([[0.0, 0, 0], [NAN, 0, 0], [1.0, 0, 0], [float("inf"), 0, 0], [2.0, 0, 0]])
    d2, index = G.knn(x, x, 4, True)
    assert index[0].tolist() == [2, 4, -1, -1] and index[2].tolist() == [0, 4, -1, -1]      # rows 1 and 3 are nobody's neighbours
    assert (index[1] == -1).all() and torch.isnan(d2[1]).all() and (index[3] == -1).all() and torch.isnan(d2[3]).all()


@pytest.mark.parametrize("name", ["edges", "lattice", "doubled"])
def test_fp32_order_is_the_fp64_order_where_the_distances_are_apart(name):
    """Where a slot's fp64 distance differs from both neighbours' by more than the rounding of the fp32 formula (4 x 2^-24 relative on each
    side), the fp32 key order names the same target."""
    checked = 0
    for x, (d32, i32), (d64, i64) in zip(K.self_case(name), K.self_statements(name), K.self_statements(name, torch.float64)):
        if x.shape[0] < 3:
            continue
        full = torch.cat([torch.full((x.shape[0], 1), -1.0, dtype=torch.float64), d64, torch.full((x.shape[0], 1), float("inf"), dtype=torch.float64)], 1)
        tol = 8 * 2.0 ** -24 * full[:, 1:-1]
        apart = (full[:, 1:-1] - full[:, :-2] > tol) & (full[:, 2:] - full[:, 1:-1] > tol) & (i64 >= 0)
        apart[:, -1] = False                                                    # the last slot's upper neighbour is not in the list
        assert torch.equal(i32[apart], i64[apart]), name
        assert ((d32.double() - d64).abs()[apart] <= 4 * 2.0 ** -24 * d64[apart]).all()
        checked += int(apart.sum())
    assert checked > 1000 or name != "edges"


def test_case_conditions_of_stage_a():
    """What the GPU cases are there for: ties in the lattice, a zero-distance neighbour at another index in the doubled clouds, fewer
    candidates than slots in the tiny clouds, the non-finite rows."""
    for x, (d2, index) in zip(K.self_case("lattice"), K.self_statements("lattice")):
        ties = (d2[:, 1:] == d2[:, :-1]) & (index[:, 1:] >= 0)
        assert int(ties.sum()) > x.shape[0] and bool((index[:, 1:][ties] > index[:, :-1][ties]).all())
    for x, (d2, index) in zip(K.self_case("doubled"), K.self_statements("doubled")):
        assert bool((d2[:, 0] == 0).all()) and bool((index[:, 0] != torch.arange(x.shape[0])).all())
        assert torch.equal(x[index[:, 0].long()], x)
    for x, (d2, index) in zip(K.self_case("tiny"), K.self_statements("tiny")):
        n = x.shape[0]
        assert bool(((index >= 0).sum(dim=1) == min(n - 1, K.K_MAX)).all()) if n else index.shape == (0, K.K_MAX)
    x, (d2, index) = K.self_case("non_finite")[0], K.self_statements("non_finite")[0]
    assert (index[[3, 10]] == -1).all() and not bool(((index == 3) | (index == 10)).any()) and bool((index[0] >= 0).sum() == 32)
    sizes = [x.shape[0] for x in K.self_case("edges")]
    assert all(n in sizes for n in (255, 256, 257, 511, 512, 513)) and len(K.self_case("many_tiny")) == 512


# ------------------------------------------------------------------ (b) normals
def test_normals_by_hand():
    """A flat 3 x 3 grid in the plane z = 2: normal +-z, curvature 0; a collinear row: a unit vector across it; two members: nothing."""
    grid = torch.tensor([[float(i), float(j), 2.0] for i in range(3) for j in range(3)])
    index = G.knn(grid, grid, 8, True)[1]
    r = G.normals(grid, index)
    assert torch.allclose(r["normal"].abs(), torch.tensor([0.0, 0, 1], dtype=torch.float64).expand(9, 3), atol=1e-12)
    assert bool((r["curvature"].abs() < 1e-15).all()) and bool((r["members"] == 9).all())
    line = torch.tensor([[float(i), 0.0, 0.0] for i in range(5)])
    r = G.normals(line, G.knn(line, line, 4, True)[1])
    assert torch.allclose(r["normal"].norm(dim=1), torch.ones(5, dtype=torch.float64)) and bool((r["normal"][:, 0].abs() < 1e-12).all())
    assert bool((r["gap"].abs() < 1e-12).all())
    two = torch.tensor([[0.0, 0, 0], [1.0, 0, 0]])
    r = G.normals(two, G.knn(two, two, 4, True)[1])
    assert bool((r["normal"] == 0).all()) and torch.isnan(r["curvature"]).all()
    same = torch.ones(6, 3)
    r = G.normals(same, G.knn(same, same, 4, True)[1])
    assert torch.isnan(r["curvature"]).all() and torch.allclose(r["normal"].norm(dim=1), torch.ones(6, dtype=torch.float64))


@pytest.mark.parametrize("n, mean_deg, worst_deg", [(2048, 1.1, 4.5), (1024, 1.7, 7.0)])
def test_sphere_normals_lie_close_to_the_analytic_ones(n, mean_deg, worst_deg):
    """PCA on k = 16 samples of a sphere of radius 0.8: the angles to the analytic normal, asserted at twice the figures one seed gave."""
    x, ref = K.sphere(n, 4242 + n)
    r = G.normals(x, G.knn(x, x, 16, True)[1])
    ang = angles_deg(r["normal"], ref)
    print(f"\n[sphere normals] N = {n}, k = 16: mean {float(ang.mean()):.2f} deg, worst {float(ang.max()):.2f} deg")
    assert float(ang.mean()) <= 2 * mean_deg and float(ang.max()) <= 2 * worst_deg
    flipped, dot = G.oriented(r["normal"], x, 1)
    assert bool(((flipped * ref).sum(dim=1) > 0.9).all())                       # outward on a sphere: along the radius
    assert float(r["curvature"].max()) < 0.05


def test_case_conditions_of_stage_b():
    """The direction comparison leaves out at most 3 % of any case's points (gap < 0.1); every case has points whose orientation is decided
    by more than 1e-4; every surface point has its full neighbourhood."""
    view = torch.tensor([0.3, -2.0, 1.5])
    for k in K.SURFACE_KS:
        for (kind, n), (x, ref), s in zip(K.SURFACES, K.surfaces(), K.surface_statements(k)):
            r = s["normals"]
            share = float((r["gap"] < K.GAP_MIN).double().mean())
            print(f"\n[gap] {kind} N = {n} k = {k}: {100 * share:.2f} % of the points below {K.GAP_MIN}")
            assert share <= K.GAP_SHARE, (kind, n, k, share)
            assert bool((r["members"] == k + 1).all()) and torch.allclose(r["normal"].norm(dim=1), torch.ones(n, dtype=torch.float64))
            for mode in (1, 2):
                _, dot = G.oriented(r["normal"], x, mode, view)
                assert int((dot.abs() > 1e-4).sum()) > n // 2
            if k == 16 and kind == "sphere":                                    # the torus tube (radius 0.25) bends inside a neighbourhood
                assert float(angles_deg(r["normal"], ref).mean()) < (8.0 if n == 257 else 4.0)


# ------------------------------------------------------------------ (c) outliers
def test_outlier_rules_by_hand():
    d2 = torch.tensor([[1.0, 4.0], [1.0, NAN], [NAN, NAN], [9.0, 9.0], [4.0, 4.0]])
    s = G.outlier_statistical(d2, 1.0)
    assert s["dbar"][:2].tolist() == [1.5, 1.0] and math.isnan(float(s["dbar"][2])) and s["dbar"][3:].tolist() == [3.0, 2.0]
    assert s["mu"] == 1.875 and abs(s["sigma"] - math.sqrt((0.375 ** 2 + 0.875 ** 2 + 1.125 ** 2 + 0.125 ** 2) / 4)) < 1e-15
    assert s["mask"].tolist() == [1, 1, 0, 0, 1]                                # limit 2.62: the point without a slot and the far one go
    assert G.outlier_statistical(d2, 2.0)["mask"].tolist() == [1, 1, 0, 1, 1]
    assert G.outlier_radius(d2, 2.0, 2).tolist() == [1, 0, 0, 0, 1] and G.outlier_radius(d2, 2.0, 1).tolist() == [1, 1, 0, 0, 1]
    none = G.outlier_statistical(d2[2:3], 2.0)
    assert none["mask"].tolist() == [0]
    # the radius is compared as the fp32 product r * r
    r = 0.1
    r2 = torch.tensor(r) * torch.tensor(r)
    on = torch.stack([r2, torch.nextafter(r2, torch.tensor(1.0))])[:, None]
    assert G.outlier_radius(on, r, 1).tolist() == [1, 0]


def test_far_outliers_go_and_the_sphere_stays():
    x, flag = K.sphere_with_outliers()
    d2 = G.knn(x, x, 16, True)[0]
    s = G.outlier_statistical(d2, 2.0)
    assert torch.equal(s["mask"].bool(), ~flag)
    out, _, count = G.compact(x, s["mask"])
    assert count == 1024 and torch.equal(out[:count], x[~flag]) and bool((out[count:] == 0).all())


def test_case_conditions_of_stage_c():
    """No point of any case lies within 1e-9 relative of its cloud's limit, so the masks can be compared everywhere; the roots of the statement
    are the correctly rounded ones; the cases hold points without a valid slot, kept and dropped points."""
    nearest = float("inf")
    kept = dropped = slotless = 0
    for name, (k, clouds, tables) in K.outlier_batches().items():
        for d2 in tables:
            for ratio in K.OUTLIER_RATIOS:
                s = G.outlier_statistical(d2, ratio)
                have = ~torch.isnan(s["dbar"])
                if bool(have.any()):
                    rel = ((s["dbar"][have] - s["limit"]).abs() / s["limit"]).min() if s["limit"] > 0 else torch.tensor(float("inf"))
                    nearest = min(nearest, float(rel))
                    assert float(rel) > K.BAND, (name, ratio, float(rel))
                kept += int(s["mask"].sum())
                dropped += int((have & ~s["mask"].bool()).sum())
                slotless += int((~have).sum())
    print(f"\n[outliers] the nearest dbar lies {nearest:.2e} relative from its limit")
    assert kept > 1000 and dropped > 100 and slotless >= 4
    v = torch.tensor([2.0, 3.0, 0.1, 1e-30, 7.0])
    assert torch.equal(G.sqrt(v, torch.float32), torch.from_numpy(np.sqrt(v.double().numpy())).float())


def test_compact_by_hand():
    x = torch.arange(15.0).reshape(5, 3)
    a = -x
    out, attr, count = G.compact(x, torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8), a, rows=7)
    assert count == 3 and out.shape == (7, 3) and out[:3].tolist() == x[[1, 2, 4]].tolist() and bool((out[3:] == 0).all())
    assert torch.equal(attr[:3], a[[1, 2, 4]]) and bool((attr[3:] == 0).all())
    assert G.compact(x, torch.zeros(5, dtype=torch.uint8))[2] == 0 and G.compact(x, torch.ones(5, dtype=torch.uint8))[2] == 5


# ------------------------------------------------------------------ PLY cloud files
def test_ply_cloud_round_trip(tmp_path):
    from shapegen_amd.utils import Mesh, load_mesh, load_point_cloud, save_mesh, save_point_cloud
    g = torch.Generator().manual_seed(3)
    pts = torch.randn(37, 3, generator=g) * 1e-3 + 0.3
    nrm = torch.nn.functional.normalize(torch.randn(37, 3, generator=g), dim=1)
    for ascii_ in (False, True):
        for normals in (None, nrm):
            path = str(tmp_path / f"cloud_{int(ascii_)}_{normals is not None}.ply")
            save_point_cloud(path, pts, normals, ascii=ascii_)
            head = open(path, "rb").read(64)
            assert head.startswith(b"ply\nformat ascii 1.0\n" if ascii_ else b"ply\nformat binary_little_endian 1.0\n")
            got, got_n = load_point_cloud(path)
            assert got.dtype == torch.float32 and torch.equal(got, pts)          # 9 significant digits round-trip float32
            assert (got_n is None) if normals is None else torch.equal(got_n, nrm)
            mesh = load_mesh(path)                                               # a cloud file is a mesh file without faces
            assert torch.equal(mesh.vertices, pts) and mesh.faces.shape == (0, 3)
    # a mesh file is a cloud file: the faces are ignored
    tri = Mesh(pts[:4], torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32))
    path = str(tmp_path / "mesh.ply")
    save_mesh(path, tri)
    got, got_n = load_point_cloud(path)
    assert torch.equal(got, pts[:4]) and got_n is None
    # an empty cloud
    path = str(tmp_path / "empty.ply")
    save_point_cloud(path, torch.zeros(0, 3))
    got, got_n = load_point_cloud(path)
    assert got.shape == (0, 3) and got_n is None
    # double coordinates and a skipped property, written by hand
    path = str(tmp_path / "hand.ply")
    with open(path, "w") as out:
        out.write("ply\nformat ascii 1.0\ncomment by hand\nelement vertex 2\nproperty double x\nproperty double y\nproperty uchar red\n"
                  "property double z\nend_header\n0.5 1.5 255 2.5\n-1 -2 0 -3\n")
    got, got_n = load_point_cloud(path)
    assert got.tolist() == [[0.5, 1.5, 2.5], [-1.0, -2.0, -3.0]] and got_n is None


def test_ply_cloud_errors(tmp_path):
    from shapegen_amd.utils import load_point_cloud, save_point_cloud
    pts = torch.rand(20, 3)
    nrm = torch.rand(20, 3)
    for ascii_ in (False, True):
        path = str(tmp_path / f"cut_{int(ascii_)}.ply")
        save_point_cloud(path, pts, nrm, ascii=ascii_)
        raw = open(path, "rb").read()
        open(path, "wb").write(raw[:len(raw) - 100])
        with pytest.raises(ValueError, match="ends inside the vertex element"):
            load_point_cloud(path)
    with pytest.raises(ValueError, match="writes .ply"):
        save_point_cloud(str(tmp_path / "cloud.obj"), pts)
    with pytest.raises(ValueError, match="shaped like"):
        save_point_cloud(str(tmp_path / "bad.ply"), pts, nrm[:5])
    path = str(tmp_path / "not.ply")
    open(path, "w").write("plain text\n")
    with pytest.raises(ValueError, match="not a PLY file"):
        load_point_cloud(path)
    path = str(tmp_path / "half.ply")
    open(path, "w").write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
                          "end_header\n0 0 0 1\n")
    with pytest.raises(ValueError, match="all three or not at all"):
        load_point_cloud(path)
    assert not os.path.exists(str(tmp_path / "cloud.obj"))


# ------------------------------------------------------------------ argument checks of shapegen_amd.geometry
def test_geometry_refuses_bad_arguments_before_the_library_is_loaded():
    from shapegen_amd import _lib, geometry
    x = torch.zeros(2, 8, 3)
    loaded = _lib.load
    _lib.load = lambda: pytest.fail("the library was loaded before the arguments were checked")
    try:
        for k in (0, 33, -1, 2.5, True, None):
            with pytest.raises(ValueError, match="k must be"):
                geometry.k_nearest_neighbors(x, k=k)
            with pytest.raises(ValueError, match="k must be"):
                geometry.estimate_normals(x, k=k)
            with pytest.raises(ValueError, match="k must be"):
                geometry.remove_outliers(x, k=k)
        with pytest.raises(ValueError, match="orient"):
            geometry.estimate_normals(x, orient="inward")
        with pytest.raises(ValueError, match="orient"):
            geometry.estimate_normals(x, orient=torch.zeros(2, 4))
        with pytest.raises(ValueError, match="std_ratio"):
            geometry.remove_outliers(x, std_ratio=float("nan"))
        with pytest.raises(ValueError, match="radius"):
            geometry.remove_outliers(x, radius=-1.0)
        with pytest.raises(ValueError, match="min_neighbors"):
            geometry.remove_outliers(x, k=8, radius=0.1, min_neighbors=9)
        with pytest.raises(ValueError, match="min_neighbors"):
            geometry.remove_outliers(x, min_neighbors=3)
        with pytest.raises(ValueError, match="target_counts"):
            geometry.k_nearest_neighbors(x, target_counts=torch.tensor([1, 1]))
        with pytest.raises(ValueError, match=r"\(P, N, 3\)"):
            geometry.k_nearest_neighbors(torch.zeros(8, 3))
        # a CPU tensor: the project's usual RuntimeError, still before the library is loaded
        for call in (lambda: geometry.k_nearest_neighbors(x), lambda: geometry.estimate_normals([x[0]]), lambda: geometry.remove_outliers(x)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()
    finally:
        _lib.load = loaded


def test_entry_points_refuse_bad_arguments_on_the_host():
    """The C entry points report argument errors before any device work: every pointer below is a dummy, and every call is refused."""
    from shapegen_amd import _lib
    lib = _lib.load()
    p = 64
    for k in (0, 33):
        assert lib.pcd_knn(p, p, 8, p, p, 8, 1, k, 1, p, p, None) == -1 and b"bad argument" in lib.pcd_last_error()
    assert lib.pcd_knn(None, p, 8, p, p, 8, 1, 4, 1, p, p, None) == -1
    assert lib.pcd_knn(p, p, 0, p, p, 8, 1, 4, 1, p, p, None) == -1 and lib.pcd_knn(p, p, 8, p, p, 8, 65536, 4, 1, p, p, None) == -1
    assert lib.pcd_cloud_normals_workspace_bytes(0) == 0 and lib.pcd_cloud_normals_workspace_bytes(64) >= 64 * 24
    assert lib.pcd_cloud_normals(p, p, 8, 1, p, 4, 3, None, p, None, None, 0, None) == -1                 # unknown mode
    assert lib.pcd_cloud_normals(p, p, 8, 1, p, 4, 2, None, p, None, None, 0, None) == -1                 # no viewpoints
    assert lib.pcd_cloud_normals(p, p, 8, 1, p, 4, 1, None, p, None, None, 0, None) == -1                 # outward without a workspace
    assert lib.pcd_cloud_normals(p, p, 8, 1, p, 4, 1, None, p, None, p, 8, None) == -1                    # ... or too small a one
    assert lib.pcd_cloud_outlier_mask(p, p, 8, 1, 4, 2, 2.0, 0.0, 1, p, None, None) == -1                 # unknown method
    assert lib.pcd_cloud_outlier_mask(p, p, 8, 1, 4, 0, float("inf"), 0.0, 1, p, None, None) == -1
    assert lib.pcd_cloud_outlier_mask(p, p, 8, 1, 4, 1, 2.0, -1.0, 1, p, None, None) == -1
    assert lib.pcd_cloud_outlier_mask(p, p, 8, 1, 4, 1, 2.0, 0.1, 5, p, None, None) == -1                 # min_neighbors > k
    assert lib.pcd_cloud_compact(p, p, p, p, 8, 1, 128, None, p, None) == -1                              # attr without attr_out
    assert lib.pcd_cloud_compact(p, None, p, p, 8, 1, p, None, p, None) == -1                             # in place
    assert lib.pcd_cloud_compact(p, None, p, p, 0, 1, 128, None, p, None) == -1
