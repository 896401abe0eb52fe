"""`data.DeviceMeshDataModule` and the C ABI of csrc/mesh_data.hip without a device: the symbols, the argument refusals (decided on the
host before any device work), the directory walk with its categories, labels and split, the refusals of `setup()`, and the numpy
statement (tests/mesh_data_statement.py) against float64."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_data_statement as S
from shapegen_amd import _lib as L
from shapegen_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcd_mesh_area_sums", "pcd_mesh_batch_clouds", "pcd_mesh_data_config")


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pcd_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in L._SIGS and getattr(lib, name).argtypes == L._SIGS[name][1]
    assert len(L._SIGS["pcd_mesh_batch_clouds"][1]) == 17 and len(L._SIGS["pcd_mesh_area_sums"][1]) == 6
    assert lib.pcd_abi_version() == L.ABI_VERSION == 2
    const = dict(re.findall(r"#define PCD_MESH_(CTR_\w+|MAX_POINTS) (.+)", header))
    value = lambda t: eval(t.split("/*")[0].replace("ull", ""))           # noqa: E731
    assert {k: value(v) for k, v in const.items()} == {"CTR_POINT": S.CTR_POINT, "CTR_ANGLE": S.CTR_ANGLE, "CTR_JITTER": S.CTR_JITTER,
                                                       "CTR_SPAN": S.CTR_SPAN, "MAX_POINTS": S.MAX_POINTS}
    assert D.MESH_CTR_SPAN == S.CTR_SPAN and D.MESH_MAX_POINTS == S.MAX_POINTS
    for n in (1, 2048, S.MAX_POINTS):                       # the ranges of a slot cannot meet, nor can two slots
        a, b = S.span_ranges(n, 0, 5 * S.CTR_SPAN), S.span_ranges(n, 1, 5 * S.CTR_SPAN)
        parts = [a[k] for k in ("point", "angle", "jitter")]
        for i, (lo, hi) in enumerate(parts):
            assert a["span"][0] <= lo < hi <= a["span"][1]
            assert all(hi <= lo2 or hi2 <= lo for lo2, hi2 in parts[i + 1:])
        assert a["span"][1] <= b["span"][0]


def test_bad_arguments_are_refused_before_any_device_work():
    """No device here: a call that got past its argument checks would fail with a HIP error (-2), not -1."""
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    good = [p, p, p, 3, p, None]
    for pos, bad in ((0, None), (1, None), (2, None), (4, None), (3, 0), (3, -2)):
        args = list(good)
        args[pos] = bad
        assert lib.pcd_mesh_area_sums(*args) == -1 and b"bad argument" in lib.pcd_last_error(), pos
    nan, inf = float("nan"), float("inf")
    #       vertices faces offsets n_meshes sums index batch points seed offset flags sigma clip out normals faces stream
    good = [p, p, p, 3, p, p, 4, 64, 1, 0, 1, 0.01, 0.05, p, None, None, None]
    for pos, bad in ((0, None), (1, None), (2, None), (4, None), (5, None), (13, None), (3, 0), (3, -1), (6, 0), (6, -4), (7, 0), (7, -1),
                     (7, (1 << 24) + 1), (10, 8), (10, -1), (11, nan), (11, inf), (12, nan), (12, -inf)):
        args = list(good)
        args[pos] = bad
        assert lib.pcd_mesh_batch_clouds(*args) == -1 and b"bad argument" in lib.pcd_last_error(), pos
    assert lib.pcd_mesh_data_config(2) == -1 and lib.pcd_mesh_data_config(-1) == -1
    assert lib.pcd_mesh_data_config(0) == 0 and lib.pcd_mesh_data_config(1) == 0
    assert not any(buf)


# ---------------------------------------------------------------------------------------------- the module
def _write_dir(root):
    """Seven meshes: two directly in the directory, three in chair/, two in table/ (one of them a .ply one level further down)."""
    from shapegen_amd.utils import save_mesh
    os.makedirs(root / "chair")
    os.makedirs(root / "table" / "round")
    names = ["b_top.obj", "a_top.obj", "chair/c2.obj", "chair/c0.obj", "chair/c1.obj", "table/t0.obj", "table/round/t1.ply"]
    for i, name in enumerate(names):
        v, f = S.ellipsoid(i) if i % 2 else S.box(-0.5 - 0.1 * i, 0.5)
        save_mesh(str(root / name), (torch.from_numpy(v), torch.from_numpy(f)))
    (root / "chair" / "notes.txt").write_text("not a mesh")
    return names


def test_directory_walk_categories_labels_and_split(tmp_path):
    from shapegen_amd.training import split_fingerprint
    from shapegen_amd.utils import load_mesh
    root = tmp_path / "meshes"
    names = _write_dir(root)
    mods = []
    for _ in range(2):
        torch.manual_seed(24)
        dm = D.DeviceMeshDataModule(str(root), num_points=64, batch_size=4, return_labels=True, device="cpu")
        dm.setup()
        mods.append(dm)
    a, b = mods
    want = sorted(os.path.join(*n.split("/")) for n in names)
    assert a.file_list == b.file_list == want
    assert a.categories == ["", "chair", "table"]
    assert a.labels_device.tolist() == [0, 0, 1, 1, 1, 2, 2] == b.labels_device.tolist()
    assert list(a.train_dataset.indices) == list(b.train_dataset.indices) and len(a.train_dataset.indices) == 5
    assert list(a.val_dataset.indices) == list(b.val_dataset.indices) and len(a.val_dataset.indices) == 2
    assert split_fingerprint(a) == split_fingerprint(b) is not None
    # the table is the files' meshes in that order, faces local to each mesh
    assert a.offsets_host.shape == (8, 2) and a.vertices.device.type == "cpu" and a.faces.dtype == torch.int32
    for i, name in enumerate(a.file_list):
        m = load_mesh(str(root / name))
        (v0, f0), (v1, f1) = a.offsets_host[i], a.offsets_host[i + 1]
        assert torch.equal(a.vertices[v0:v1], m.vertices) and torch.equal(a.faces[f0:f1], m.faces)
    assert a.flags == S.NORMALIZE | S.JITTER
    flags = lambda **kw: D.DeviceMeshDataModule(str(root), device="cpu", **kw).flags          # noqa: E731
    assert flags(augmentations=False) == S.NORMALIZE and flags(augmentations=False, normalization=False) == 0
    assert flags(rotate=True) == S.NORMALIZE | S.JITTER | S.ROTATE
    with pytest.raises(RuntimeError, match="GPU"):
        next(iter(a.train_dataloader()))                    # no CPU path behind the loaders
    with pytest.raises(RuntimeError, match="GPU"):
        next(iter(a.val_dataloader()))
    flat = D.DeviceMeshDataModule(str(root / "chair"), device="cpu", return_labels=True)
    flat.setup()
    assert flat.categories == [""] and flat.labels_device.tolist() == [0, 0, 0]


def test_meshes_argument_and_refusals(tmp_path):
    meshes = [S.box(-1, 1), S.ellipsoid(3), S.random_triangles(5, 0), S.box(0, 2), S.ellipsoid(4)]
    dm = D.DeviceMeshDataModule(meshes=meshes, labels=[0, 1, 2, 0, 1], return_labels=True, num_points=64, device="cpu")
    dm.setup()
    assert dm.labels_device.tolist() == [0, 1, 2, 0, 1] and len(dm.train_dataset.indices) == 4 and len(dm.val_dataset.indices) == 1
    assert dm.offsets_host[-1].tolist() == [sum(len(v) for v, _ in meshes), sum(len(f) for _, f in meshes)]
    for kw in (dict(), dict(meshes=meshes, data_dir=str(tmp_path)), dict(meshes=meshes, return_labels=True), dict(meshes=meshes, num_points=0),
               dict(meshes=meshes, num_points=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            D.DeviceMeshDataModule(device="cpu", **kw)
    with pytest.raises(ValueError, match="3 labels for 5 meshes"):
        D.DeviceMeshDataModule(meshes=meshes, labels=[0, 1, 2], device="cpu").setup()
    with pytest.raises(ValueError, match="no .obj or .ply"):
        D.DeviceMeshDataModule(str(tmp_path), device="cpu").setup()

    def refuses(name, text, match):
        root = tmp_path / name
        os.makedirs(root)
        S.write_obj(str(root / "good.obj"), S.box(-1, 1))
        (root / "zbad.obj").write_text(text)
        with pytest.raises(ValueError, match=match) as e:
            D.DeviceMeshDataModule(str(root), device="cpu").setup()
        assert "zbad.obj" in str(e.value)

    tri = "v 0 0 0\nv 1 0 0\nv 0 1 0\n"
    refuses("nofaces", tri, "no faces")
    refuses("range", tri + "f 1 2 4\n", "zbad.obj")
    refuses("flat", tri + "v 2 0 0\nf 1 2 4\nf 1 1 3\n", "total area of the mesh is 0")
    refuses("huge", "v 0 0 0\nv 3e38 0 0\nv 0 3e38 0\nf 1 2 3\n", "total area")
    refuses("nan", "v 0 0 0\nv nan 0 0\nv 0 1 0\nf 1 2 3\n", "total area")
    v, f = S.box(-1, 1)
    for bad, match in (((v, f[:0]), "no faces"), ((v, f + 1), "face index"), ((v * 0, f), "total area")):
        with pytest.raises(ValueError, match=match) as e:
            D.DeviceMeshDataModule(meshes=[S.box(0, 1), bad], device="cpu").setup()
        assert "meshes[1]" in str(e.value)


# ---------------------------------------------------------------------------------------------- the statement against float64
def test_statement_cloud_is_centred_with_unit_radius():
    for mesh, n in ((S.ellipsoid(7), 2048), (S.box((-2, -1, -0.5), (2, 1, 0.5)), 1500), (S.random_triangles(1025, 1), 64)):
        cloud = S.cloud_fp32(*mesh, n, seed=11, offset=3 * S.CTR_SPAN, slot=2, flags=S.NORMALIZE)
        assert cloud.dtype == np.float32 and cloud.shape == (n, 3)
        c64 = cloud.astype(np.float64)
        assert np.abs(c64.mean(axis=0)).max() <= 1e-6
        assert abs(np.sqrt((c64 ** 2).sum(axis=1)).max() - 1.0) <= 1e-6
        want, _, index = S.cloud_f64(*mesh, n, 11, 3 * S.CTR_SPAN, 2, S.NORMALIZE)
        assert np.abs(c64 - want).max() <= 1e-5 and index.min() >= 0 and index.max() < len(mesh[1])
    # the summation order is the header's, not numpy's: the sum of 2500 values equals the float64 sum to rounding and is repeatable
    x = np.random.default_rng(0).uniform(-1, 1, 2500).astype(np.float32)
    assert abs(float(S.column_sum_fp32(x)) - x.astype(np.float64).sum()) <= 1e-4 and S.column_sum_fp32(x) == S.column_sum_fp32(x.copy())
    assert S.column_sum_fp32(np.arange(5000, dtype=np.float32)) == 5000 * 4999 / 2          # integers below 2^24: exact in any order


def test_statement_running_sums_and_points_against_float64():
    for faces in (1, 12, 1023, 1024, 1025, 2500):
        v, f = S.box(-1, 1) if faces == 12 else S.random_triangles(faces, faces)
        sums = S.running_sums_fp32(v, f)
        t = v.astype(np.float64)[f]
        want = np.cumsum(0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1))
        assert sums.dtype == np.float32 and sums.shape == (faces,) and np.all(np.diff(sums) >= 0)
        assert np.abs(sums - want).max() <= 1e-5 * want[-1]
        p, index, nrm = S.draw_fp32(v, f, 300, 5, 0)
        a, e0, e1 = t[index, 0], t[index, 1] - t[index, 0], t[index, 2] - t[index, 0]
        normal = np.cross(e0, e1)
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        assert np.abs(((p - a) * normal).sum(axis=1)).max() <= 1e-6            # on the plane of its triangle
        assert np.abs(nrm - normal).max() <= 1e-5


def test_statement_triangle_histogram_follows_the_areas():
    v, f = S.three_triangles_1_2_5()
    sums = S.running_sums_fp32(v, f)
    assert sums.tolist() == [1.0, 3.0, 8.0]
    n = 200_000
    counts = np.bincount(S.choose(sums, S.uniforms(n, seed=77, ctr0=9 * S.CTR_SPAN)[:, 0]), minlength=3)
    share = np.array([1, 2, 5]) / 8.0
    sigma = np.sqrt(n * share * (1 - share))
    print("counts", counts.tolist(), "expected", (n * share).tolist(), "sigma", sigma.round(1).tolist())
    assert counts.sum() == n and np.all(np.abs(counts - n * share) <= 4 * sigma)
