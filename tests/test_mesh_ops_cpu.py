"""Mesh processing without a device: the numpy statement (tests/mesh_ops_statement.py) against brute force on the cases of
tests/mesh_ops_cases.py, the fp32 form of the statement against the fp64 form, `save_mesh(normals=)`, and the argument errors of
`shapegen_amd.mesh_ops`, raised before the library is touched."""
import numpy as np
import pytest
import torch

import mesh_ops_cases as C
import mesh_ops_statement as S

ALL = tuple(C.BUILDERS)


@pytest.mark.parametrize("name", ALL)
def test_adjacency_statement_equals_an_edge_dictionary(name):
    v, f = C.case(name)
    nv = v.shape[0]
    adj = S.adjacency(nv, f)
    edges, incident = {}, {a: [] for a in range(nv)}
    for t, (a, b, c) in enumerate(f.tolist()):
        if not (0 <= a < nv and 0 <= b < nv and 0 <= c < nv) or a == b or b == c or a == c:
            continue
        for p, q in ((a, b), (b, c), (c, a)):
            edges.setdefault((p, q), [0, 0])[0] += 1
            edges.setdefault((q, p), [0, 0])[1] += 1
        for p in (a, b, c):
            incident[p].append(t)
    ring = {a: [] for a in range(nv)}
    for (p, u), (o, i) in edges.items():
        ring[p].append((u, o, i))
    for a in range(nv):
        want = sorted(ring[a])
        r0, r1 = adj["nbr_start"][a], adj["nbr_start"][a + 1]
        got = [(int(u), int(o), int(i)) for u, (o, i) in zip(adj["nbr_index"][r0:r1], adj["nbr_counts"][r0:r1])]
        assert got == want, (name, a)
        assert adj["inc_faces"][adj["inc_start"][a]:adj["inc_start"][a + 1]].tolist() == incident[a], (name, a)
        flags = (S.REFERENCED if incident[a] else 0) | (S.BOUNDARY if any(o + i == 1 for _, o, i in want) else 0) | \
                (S.IRREGULAR if any(o != 1 or i != 1 for _, o, i in want) else 0)
        assert adj["flags"][a] == flags, (name, a)
    if name == "pole_fan":
        assert adj["nbr_start"][1] - adj["nbr_start"][0] == 70               # a row longer than a wave


@pytest.mark.parametrize("name", ALL)
def test_closed_statement_equals_mesh_is_closed(name):
    """`bad_indices` is an open patch, so the invalid faces, which `mesh_is_closed` counts and the statement skips, do not decide it."""
    from shapegen_amd.utils import mesh_is_closed
    v, f = C.case(name)
    m = S.measures(v, f)
    assert bool(m["closed"]) == mesh_is_closed((torch.from_numpy(v.copy()), torch.from_numpy(f.copy()))), name
    assert m["closed"] == (0 if name in ("grid_patch", "cube_flipped", "non_manifold", "pole_fan", "bad_indices") else 1)
    if name in C.CLOSED_GENUS_0:
        assert m["euler"] == 2 and m["boundary_edges"] == 0 and m["irregular_edges"] == 0 and m["components"] == 1 and m["volume"] > 0
    if name == "cube":
        assert m["volume"] == 8.0 and m["area"] == 24.0 and np.array_equal(m["centroid"], np.zeros(3))
    if name == "cube_flipped":
        assert m["irregular_edges"] == 3 and m["boundary_edges"] == 0
    if name == "non_manifold":
        assert m["irregular_edges"] == 7 and m["boundary_edges"] == 6


@pytest.mark.parametrize("name", ALL)
def test_component_statement_equals_union_find(name):
    v, f = C.case(name)
    nv = v.shape[0]
    parent = list(range(nv))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    valid = S.valid_faces(nv, f)
    used = set()
    for (a, b, c), ok in zip(f.tolist(), valid):
        if ok:
            used.update((a, b, c))
            for p, q in ((a, b), (b, c)):
                rp, rq = find(p), find(q)
                parent[max(rp, rq)] = min(rp, rq)
    want = np.array([find(a) if a in used else -1 for a in range(nv)], np.int32).reshape(-1)
    labels, count, sizes = S.components(nv, f)
    assert np.array_equal(labels, want), name
    assert count == len({int(x) for x in want if x >= 0})
    for root in np.unique(want[want >= 0]):
        assert sizes[root] == sum(1 for (a, _, _), ok in zip(f.tolist(), valid) if ok and want[a] == root)
    assert sizes.sum() == valid.sum()
    if name == "mixed":
        assert count == 3 and labels[0] == -1 and sizes[1] == 12 and sizes[9] == sizes[13] == 4
        assert np.array_equal(np.nonzero(S.keep_flags(nv, f, keep_largest=True))[0], np.arange(1, 9))
        assert np.array_equal(np.nonzero(S.keep_flags(nv, f, min_faces=4))[0], np.arange(1, 17))
        assert np.array_equal(np.nonzero(S.keep_flags(nv, f, min_faces=5))[0], np.arange(1, 9))
        cv, cf = S.compact(v, f, S.keep_flags(nv, f, keep_largest=True))
        assert np.array_equal(cv, C.case("cube")[0]) and np.array_equal(cf, C.case("cube")[1])
    if name == "two_tetrahedra":
        assert np.array_equal(np.nonzero(S.keep_flags(nv, f, keep_largest=True))[0], np.arange(4))   # the tie: the smaller label


SMOOTH_ARGS = ((1, 0.5, 0.0), (3, 0.5, -0.53), (10, 0.33, -0.34))


def test_fp32_statement_is_the_fp64_statement_up_to_rounding():
    """The fp32-mirrored smoothing and normals against the same formulas in double, over every case and the three parameter sets of the
    device tests.  Measured here: smoothing 4.96e-7 (largest absolute difference of a coordinate; the coordinates are of order 1, a step
    adds a handful of 6e-8 roundings and ten rounds keep them), normals 2.44e-7 (unit vectors).  The bounds are four times those: the margin
    only has to catch a wrong order of operations, which shows as orders of magnitude."""
    worst_s = worst_n = 0.0
    for name in C.BUILDERS:
        v, f = C.case(name)
        if v.shape[0] == 0:
            continue
        for it, lam, mu in SMOOTH_ARGS:
            a, b = S.smooth(v, f, it, lam, mu, dtype=np.float32), S.smooth(v, f, it, lam, mu, dtype=np.float64)
            worst_s = max(worst_s, float(np.abs(a.astype(np.float64) - b).max()))
        a, b = S.vertex_normals(v, f, np.float32), S.vertex_normals(v, f, np.float64)
        assert np.array_equal(np.abs(a).sum(axis=1) == 0, np.abs(b).sum(axis=1) == 0), name
        worst_n = max(worst_n, float(np.abs(a.astype(np.float64) - b).max()))
    print(f"fp32 against fp64: smoothing {worst_s:.3e}, normals {worst_n:.3e}")
    assert worst_s <= 4 * 4.96e-7 and worst_n <= 4 * 2.44e-7


def test_smoothing_statement_pins_and_moves_what_it_should():
    v, f = C.case("grid_patch")
    boundary = (S.adjacency(v.shape[0], f)["flags"] & S.BOUNDARY) != 0
    assert boundary.sum() == 16
    out = S.smooth(v, f, 3, 0.5, -0.53, pin_boundary=True)
    assert np.array_equal(out[boundary].view(np.uint32), v[boundary].view(np.uint32)) and not np.array_equal(out[~boundary], v[~boundary])
    assert np.array_equal(S.smooth(v, f, 0, 0.5, -0.53).view(np.uint32), v.view(np.uint32))
    mv, mf = C.case("mixed")
    assert np.array_equal(S.smooth(mv, mf, 2, 0.5, 0.0)[0], mv[0])           # the unreferenced vertex
    n = S.vertex_normals(mv, mf)
    assert np.array_equal(n[0], np.zeros(3, np.float32)) and np.allclose(np.linalg.norm(n[1:], axis=1), 1.0, atol=1e-6)
    sphere = C.case("icosphere_642")
    assert (S.vertex_normals(*sphere) * sphere[0]).sum(axis=1).min() > 0.5   # outward (the jitter tilts them)


@pytest.mark.parametrize("ext", [".obj", ".ply"])
def test_save_mesh_with_normals_round_trips_and_without_writes_the_same_bytes(tmp_path, ext):
    from shapegen_amd import utils
    v, f = C.case("icosphere_642")
    n = S.vertex_normals(v, f)
    mesh = (torch.from_numpy(v.copy()), torch.from_numpy(f.copy()))
    plain, none, with_n = (str(tmp_path / (k + ext)) for k in ("plain", "none", "normals"))
    utils.save_mesh(plain, mesh)
    utils.save_mesh(none, mesh, normals=None)
    utils.save_mesh(with_n, mesh, normals=torch.from_numpy(n.copy()))
    assert open(plain, "rb").read() == open(none, "rb").read()
    assert open(plain, "rb").read() != open(with_n, "rb").read()
    if ext == ".ply":
        header = open(plain, "rb").read().split(b"end_header\n")[0]
        assert b"nx" not in header and header.count(b"property") == 4
        pts, nrm = utils.load_point_cloud(with_n)
        assert np.array_equal(pts.numpy(), v) and np.array_equal(nrm.numpy().view(np.uint32), n.view(np.uint32))
        assert utils.load_point_cloud(plain)[1] is None
    else:
        text = open(with_n).read().splitlines()
        assert sum(line.startswith("vn ") for line in text) == v.shape[0]
        assert text[-1] == "f {0}//{0} {1}//{1} {2}//{2}".format(*(f[-1] + 1))
        got = np.array([[float(x) for x in line.split()[1:]] for line in text if line.startswith("vn ")], np.float32)
        assert np.array_equal(got.view(np.uint32), n.view(np.uint32))        # nine significant digits: fp32 round-trips
        assert not any(line.startswith("vn") or "//" in line for line in open(plain).read().splitlines())
    back = utils.load_mesh(with_n)
    assert np.array_equal(back.vertices.numpy(), v) and np.array_equal(back.faces.numpy(), f)
    with pytest.raises(ValueError, match="one row per vertex"):
        utils.save_mesh(with_n, mesh, normals=torch.zeros(3, 3))


def test_argument_errors_come_before_the_library_and_cpu_tensors_are_refused():
    from shapegen_amd import _lib, mesh_ops
    v, f = C.case("cube")
    cpu = [(torch.from_numpy(v.copy()), torch.from_numpy(f.copy()))]
    loaded = _lib.load
    _lib.load = lambda: pytest.fail("the library was loaded before the arguments were checked")
    try:
        for kw, match in ((dict(iterations=-1), "iterations"), (dict(iterations=1.5), "iterations"), (dict(lam=float("nan")), "finite"),
                          (dict(mu=float("inf")), "finite"), (dict(lam=0.0), r"lam must lie in \(0, 1\]"), (dict(lam=1.01), "lam must lie"),
                          (dict(mu=-1.0), r"mu must lie in \(-1, 0\]"), (dict(mu=0.1), "mu must lie"), (dict(lam=0.5, mu=-0.4), "nonzero mu")):
            with pytest.raises(ValueError, match=match):
                mesh_ops.smooth_meshes(cpu, **kw)
        with pytest.raises(ValueError, match="exactly one"):
            mesh_ops.remove_small_components(cpu)
        with pytest.raises(ValueError, match="exactly one"):
            mesh_ops.remove_small_components(cpu, min_faces=3, keep_largest=True)
        with pytest.raises(ValueError, match="min_faces"):
            mesh_ops.remove_small_components(cpu, min_faces=-1)
        with pytest.raises(ValueError, match="2 keep tensors"):
            mesh_ops.compact_meshes(cpu, [torch.ones(8, dtype=torch.bool)] * 2)
        with pytest.raises(ValueError, match="bool or integer"):
            mesh_ops.compact_meshes(cpu, [torch.ones(7, dtype=torch.bool)])
        with pytest.raises(ValueError, match="bool or integer"):
            mesh_ops.compact_meshes(cpu, [torch.ones(8)])
        with pytest.raises(ValueError, match="no meshes"):
            mesh_ops.mesh_adjacency([])
        for call in (mesh_ops.mesh_adjacency, mesh_ops.smooth_meshes, mesh_ops.vertex_normals, mesh_ops.connected_components,
                     mesh_ops.mesh_measures, lambda m: mesh_ops.remove_small_components(m, keep_largest=True),
                     lambda m: mesh_ops.compact_meshes(m, [torch.ones(8, dtype=torch.bool)])):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call(cpu)
    finally:
        _lib.load = loaded


def test_library_refuses_bad_arguments_before_any_device_work():
    """The C entry points: null pointers, sizes out of range, factors out of range, unknown codes -- PCD_ERR_ARG with no device."""
    from shapegen_amd import _lib
    lib = _lib.load()
    p = 64                                                                   # never dereferenced on the host
    assert lib.pcd_mesh_adjacency_workspace_bytes(1, 10, 20) > 0 and lib.pcd_mesh_adjacency_workspace_bytes(0, 10, 20) == 0
    assert lib.pcd_mesh_adjacency_workspace_bytes(1, 10, (1 << 31) // 6) == 0
    assert lib.pcd_mesh_adjacency(p, p, 1, 10, 20, None, p, p, p, p, p, p, 0) == -1 and b"bad argument" in lib.pcd_last_error()
    assert lib.pcd_mesh_adjacency(p, p, 0, 10, 20, p, p, p, p, p, p, p, 0) == -1
    assert lib.pcd_mesh_adjacency(p, p, 1, -1, 20, p, p, p, p, p, p, p, 0) == -1
    smooth = lambda **kw: lib.pcd_mesh_smooth(p, p, 1, kw.get("tv", 10), p, p, p, kw.get("it", 1), kw.get("lam", 0.5), kw.get("mu", -0.53), 0,
                                              p, kw.get("out", 128), 0)
    for kw in (dict(it=-1), dict(it=(1 << 20) + 1), dict(lam=0.0), dict(lam=1.5), dict(lam=float("nan")), dict(mu=-1.0), dict(mu=0.25),
               dict(mu=float("inf")), dict(tv=-1), dict(out=p)):
        assert smooth(**kw) == -1, kw
    assert lib.pcd_mesh_smooth_workspace_bytes(10) >= 120 and lib.pcd_mesh_smooth_workspace_bytes(-1) == 0
    assert lib.pcd_mesh_vertex_normals(p, p, p, 1, 10, p, p, None, 0) == -1
    assert lib.pcd_mesh_components(p, p, 1, 10, 11, p, p, p, p, p, p, p, 0) == -1
    assert lib.pcd_mesh_components_workspace_bytes(10) >= 40 and lib.pcd_mesh_compact_workspace_bytes(10) >= 40
    assert lib.pcd_mesh_component_keep(p, 1, p, p, 2, 0, p, 0) == -1 and lib.pcd_mesh_component_keep(p, 1, p, p, 1, -1, p, 0) == -1
    assert lib.pcd_mesh_compact_count(p, p, 1, None, p, p, 0) == -1 and lib.pcd_mesh_compact_emit(p, p, p, 1, p, p, p, None, 0) == -1
    assert lib.pcd_mesh_measures(p, p, p, 0, p, p, p, p, p, p, 0) == -1
    try:
        for code in (0, 1):
            assert lib.pcd_mesh_ops_config(code) == 0, code
        for code in (-1, 2, 4):
            assert lib.pcd_mesh_ops_config(code) == -1, code
    finally:
        assert lib.pcd_mesh_ops_config(0) == 0
