"""`shapegen_amd.mesh_ops` on the device against the numpy statement (tests/mesh_ops_statement.py) on the cases of
tests/mesh_ops_cases.py: integer results exactly, smoothed positions and normals to the bit against the fp32-mirrored statement, area,
volume and centroid against the fp64 statement, and what must hold whatever the numbers are -- repeatability, independence of the rest
of the batch, junk past the packed rows, and both label paths of the components kernel."""
import functools

import numpy as np
import pytest
import torch

import mesh_ops_cases as C
import mesh_ops_statement as S

pytestmark = pytest.mark.gpu

SMOOTH_ARGS = ((1, 0.5, 0.0), (3, 0.5, -0.53), (10, 0.33, -0.34))
LABELS_WORKSPACE = 1                                                         # pcd_mesh_ops_config code


def dev(names):
    return [tuple(torch.from_numpy(a.copy()).cuda() for a in C.case(n)) for n in names]


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


class forced:
    """pcd_mesh_ops_config(code) for a block, the default restored on the way out."""
    def __init__(self, code):
        self.code = code

    def __enter__(self):
        from shapegen_amd import _lib
        assert _lib.load().pcd_mesh_ops_config(self.code) == 0

    def __exit__(self, *exc):
        from shapegen_amd import _lib
        assert _lib.load().pcd_mesh_ops_config(0) == 0


@functools.lru_cache(maxsize=None)
def want_smooth(name, it, lam, mu, pin=False):
    return S.smooth(*C.case(name), it, lam, mu, pin_boundary=pin, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def want_adjacency(name):
    return S.adjacency(C.case(name)[0].shape[0], C.case(name)[1])


@functools.lru_cache(maxsize=None)
def want_components(name):
    return S.components(C.case(name)[0].shape[0], C.case(name)[1])


def check_smooth(names, got, it, lam, mu, pin=False):
    for name, (v, f), src in zip(names, got, dev(names)):
        assert np.array_equal(bits(v), want_smooth(name, it, lam, mu, pin).view(np.uint32)), (name, it, lam, mu)
        assert torch.equal(f, src[1])


@pytest.mark.parametrize("names", [C.SMALL, C.MIXED_BATCH], ids=["small", "mixed"])
def test_adjacency_is_the_statement_exactly(names):
    from shapegen_amd import mesh_ops
    adj = mesh_ops.mesh_adjacency(dev(names))
    for i, name in enumerate(names):
        want = want_adjacency(name)
        (start, index, counts), (istart, ifaces) = adj.rows(i)
        for got, key in ((start, "nbr_start"), (index, "nbr_index"), (counts, "nbr_counts"), (istart, "inc_start"), (ifaces, "inc_faces"),
                         (adj.flags(i), "flags")):
            assert np.array_equal(got.cpu().numpy(), want[key]), (name, key)
        assert np.array_equal(adj.boundary(i).cpu().numpy(), (want["flags"] & S.BOUNDARY) != 0)
    if "pole_fan" in names:
        i = names.index("pole_fan")
        assert int(adj.rows(i)[0][0][1]) == 70                               # a row longer than a wave


@pytest.mark.parametrize("it,lam,mu", SMOOTH_ARGS)
@pytest.mark.parametrize("names", [C.SMALL, C.MIXED_BATCH], ids=["small", "mixed"])
def test_smoothing_is_the_fp32_statement_to_the_bit(names, it, lam, mu):
    from shapegen_amd import mesh_ops
    check_smooth(names, mesh_ops.smooth_meshes(dev(names), it, lam, mu), it, lam, mu)


def test_pinned_boundaries_and_zero_iterations_keep_the_input_bits():
    from shapegen_amd import mesh_ops
    names = ("grid_patch", "empty", "bad_indices", "cube", "icosphere_10242")
    meshes = dev(names)
    got = mesh_ops.smooth_meshes(meshes, 3, 0.5, -0.53, pin_boundary=True)
    same = mesh_ops.smooth_meshes(meshes, 0)
    check_smooth(names, got, 3, 0.5, -0.53, pin=True)
    for name, (v, _), (v0, _), (vz, _) in zip(names, got, meshes, same):
        b = (want_adjacency(name)["flags"] & S.BOUNDARY) != 0
        assert np.array_equal(bits(v)[b], bits(v0)[b]) and np.array_equal(bits(vz), bits(v0)), name
        assert vz.data_ptr() != v0.data_ptr() or v0.numel() == 0             # new vertices
    assert (want_adjacency("grid_patch")["flags"] & S.BOUNDARY != 0).sum() == 16


def test_vertex_normals_are_the_fp32_statement_to_the_bit():
    from shapegen_amd import mesh_ops
    got = mesh_ops.vertex_normals(dev(C.MIXED_BATCH))
    for name, n in zip(C.MIXED_BATCH, got):
        want = S.vertex_normals(*C.case(name), dtype=np.float32)
        assert np.array_equal(bits(n), want.view(np.uint32)), name
    mixed = got[C.MIXED_BATCH.index("mixed")]
    assert np.array_equal(bits(mixed[0]), np.zeros(3, np.uint32))            # the unreferenced vertex


@pytest.mark.parametrize("code", [0, LABELS_WORKSPACE], ids=["lds", "workspace"])
def test_components_are_the_statement_exactly_on_both_label_paths(code):
    from shapegen_amd import mesh_ops
    with forced(code):
        labels, counts, sizes = mesh_ops.connected_components(dev(C.MIXED_BATCH), return_sizes=True)
    counts = counts.cpu().tolist()
    for i, name in enumerate(C.MIXED_BATCH):
        wl, wc, ws = want_components(name)
        assert np.array_equal(labels[i].cpu().numpy(), wl) and counts[i] == wc and np.array_equal(sizes[i].cpu().numpy(), ws), name
    assert counts[C.MIXED_BATCH.index("mixed")] == 3


def test_component_removal_and_compaction():
    from shapegen_amd import mesh_ops
    names = ("mixed", "empty", "two_tetrahedra", "bad_indices", "icosphere_642")
    meshes = dev(names)
    largest = mesh_ops.remove_small_components(meshes, keep_largest=True)
    atleast4 = mesh_ops.remove_small_components(meshes, min_faces=4)
    atleast5 = mesh_ops.remove_small_components(meshes, min_faces=5)
    for i, name in enumerate(names):
        v, f = C.case(name)
        for got, kw in ((largest, dict(keep_largest=True)), (atleast4, dict(min_faces=4)), (atleast5, dict(min_faces=5))):
            wv, wf = S.compact(v, f, S.keep_flags(v.shape[0], f, **kw))
            assert np.array_equal(bits(got[i].vertices), wv.view(np.uint32)) and np.array_equal(got[i].faces.cpu().numpy(), wf), (name, kw)
            assert got[i].faces.dtype == torch.int32 and tuple(got[i].faces.shape[1:]) == (3,)
    cube_v, cube_f = C.case("cube")
    assert np.array_equal(largest[0].vertices.cpu().numpy(), cube_v) and np.array_equal(largest[0].faces.cpu().numpy(), cube_f)
    assert atleast4[0].vertices.shape[0] == 16 and atleast4[0].faces.shape[0] == 20 and atleast5[0].faces.shape[0] == 12
    tv, tf = C.case("two_tetrahedra")                                        # the tie: the tetrahedron with the smaller label
    assert np.array_equal(largest[2].vertices.cpu().numpy(), tv[:4]) and np.array_equal(largest[2].faces.cpu().numpy(), tf[:4])
    rng = np.random.default_rng(5)
    keep = [rng.uniform(size=C.case(n)[0].shape[0]) < 0.7 for n in names]
    for dtype in (torch.bool, torch.int32, torch.int64):
        got = mesh_ops.compact_meshes(meshes, [torch.from_numpy(k).cuda().to(dtype) for k in keep])
        for name, g, k in zip(names, got, keep):
            wv, wf = S.compact(*C.case(name), k)
            assert np.array_equal(bits(g.vertices), wv.view(np.uint32)) and np.array_equal(g.faces.cpu().numpy(), wf), name


def test_measures():
    """Integer measures exactly; area, volume and centroid against the fp64 statement at 1e-10 of sum |term| (double rounding times a
    generous count of operations for F <= 1e5)."""
    from shapegen_amd import mesh_ops
    names = C.MIXED_BATCH + ("tetrahedron", "octahedron", "cube_flipped", "non_manifold", "grid_patch", "two_tetrahedra")
    got = {k: t.cpu().numpy() for k, t in mesh_ops.mesh_measures(dev(names)).items()}
    assert got["area"].dtype == np.float64 and got["centroid"].shape == (len(names), 3) and got["closed"].dtype == np.int32
    for i, name in enumerate(names):
        want = S.measures(*C.case(name))
        for k in ("vertices", "edges", "faces", "boundary_edges", "irregular_edges", "components", "euler", "closed"):
            assert got[k][i] == want[k], (name, k)
        print(name, got["area"][i] - want["area"], got["volume"][i] - want["volume"], got["centroid"][i] - want["centroid"])
        assert abs(got["area"][i] - want["area"]) <= 1e-10 * want["abs_area"], name
        assert abs(got["volume"][i] - want["volume"]) <= 1e-10 * want["abs_volume"], name
        if want["area"] > 0:
            assert np.all(np.abs(got["centroid"][i] - want["centroid"]) * want["area"] <= 1e-10 * want["abs_moment"]), name
        else:
            assert np.array_equal(got["centroid"][i], np.zeros(3))
        if name in C.CLOSED_GENUS_0:
            assert got["euler"][i] == 2 and got["closed"][i] == 1
    cube = names.index("cube")
    assert got["volume"][cube] == 8.0 and got["area"][cube] == 24.0


def _everything(meshes, adjacency=None):
    from shapegen_amd import mesh_ops
    adj = mesh_ops.mesh_adjacency(meshes) if adjacency is None else adjacency
    out = [[v for v, _ in mesh_ops.smooth_meshes(meshes, 3, 0.5, -0.53, adjacency=adj)], mesh_ops.vertex_normals(meshes, adjacency=adj)]
    labels, counts, sizes = mesh_ops.connected_components(meshes, adjacency=adj, return_sizes=True)
    out += [labels, sizes, [c for c in counts]]
    kept = mesh_ops.remove_small_components(meshes, keep_largest=True)
    out += [[m.vertices for m in kept], [m.faces for m in kept]]
    measures = mesh_ops.mesh_measures(meshes, adjacency=adj)
    out += [[row for row in measures[k]] for k in sorted(measures)]
    out += [[adj.flags(i) for i in range(len(meshes))]]
    out += [[torch.cat([t.reshape(-1) for part in adj.rows(i) for t in part]) for i in range(len(meshes))]]
    return out


def _same(a, b):
    raw = lambda t: t.detach().cpu().contiguous().reshape(-1).numpy().view(np.uint8)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def test_repeatable_and_independent_of_the_rest_of_the_batch():
    meshes = dev(C.MIXED_BATCH)
    first, second = _everything(meshes), _everything(meshes)
    for a, b in zip(first, second):
        assert all(_same(x, y) for x, y in zip(a, b))
    for i in (1, 2, 3, 5, 7, 9):                                             # alone: also the empty mesh by itself
        alone = _everything([meshes[i]])
        for a, b in zip(first, alone):
            assert _same(a[i], b[0]), C.MIXED_BATCH[i]


def test_an_adjacency_of_other_meshes_is_refused():
    from shapegen_amd import mesh_ops
    adj = mesh_ops.mesh_adjacency(dev(("cube",)))
    with pytest.raises(ValueError, match="other meshes"):
        mesh_ops.smooth_meshes(dev(("octahedron",)), adjacency=adj)


def test_junk_rows_past_the_packed_totals_change_nothing(monkeypatch):
    """The packed tensors get junk vertex rows (NaN) and junk face rows (valid-looking and out of range) appended after the totals of
    `offsets`: nothing reads them."""
    from shapegen_amd import mesh_ops
    names = ("cube", "empty", "pole_fan", "mixed", "icosphere_642")
    meshes = dev(names)
    clean = _everything(meshes)
    pack = mesh_ops._pack_meshes

    def with_junk(ms, what):
        verts, faces, offsets, rows = pack(ms, what)
        tv, tf = rows[-1]
        jv = torch.full((37, 3), float("nan"), device=verts.device)
        jf = torch.tensor([[0, 1, 2], [5, 4, 3], [1 << 30, 2, 3], [-7, 0, 1]] * 9, dtype=torch.int32, device=verts.device)
        return torch.cat([verts[:tv], jv]), torch.cat([faces[:tf], jf]), offsets, rows
    monkeypatch.setattr(mesh_ops, "_pack_meshes", with_junk)
    junk = _everything(meshes)
    for a, b in zip(clean, junk):
        assert all(_same(x, y) for x, y in zip(a, b))
