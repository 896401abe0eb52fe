"""`data.DeviceVoxelDataModule` without a device: packing, the numpy statement of its kernels (tests/device_data_statement.py) against
the host dataset, the split / labels / categories against the host module, the refusals, and the Philox counter layout."""
import os
import re

import numpy as np
import pytest
import torch

import device_data_statement as S
from shapegen_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_cloud(tmp_path, occ, num_points):
    """PointCloudDataset's normalised cloud of one grid (no augmentation) and, separately, its full normalised cloud."""
    root = tmp_path / f"one_{num_points}"
    os.makedirs(root, exist_ok=True)
    np.save(root / "vox_32_res_model_03001627_000.npy", occ.astype(np.float32))
    ds = D.PointCloudDataset(str(root), num_points=num_points, input_mode="voxels", output_mode="point_clouds", jitter=False, rotate=False)
    full = D.PointCloudDataset.normalize_point_cloud(D.PointCloudDataset.voxel_to_point_cloud(occ.astype(np.float32)))
    return ds[0].numpy(), full.astype(np.float32)


def test_pack_unpack_round_trip_and_scan_order():
    occ = np.stack([S.grid_with_count(m, m) for m in (0, 1, 2, 777, 32768)])
    packed = D.pack_grids(occ)
    assert packed.shape == (5, 1024) and packed.dtype == np.uint32
    assert np.array_equal(D.unpack_grids(packed), occ)
    for g, w in zip(occ, packed):
        assert np.array_equal(S.pack(g), w) and np.array_equal(S.unpack(w), g)
        assert np.array_equal(S.scan_points(w), D.PointCloudDataset.voxel_to_point_cloud(g.astype(np.float32)))
    one = np.zeros((32, 32, 32), bool)
    one[3, 5, 7] = True                                   # word z * 32 + y, bit x
    assert D.pack_grids(one[None])[0, 3 * 32 + 5] == 1 << 7 and D.pack_grids(one[None]).sum() == 1 << 7
    assert np.array_equal(D.unpack_grids(np.full((1, 1024), 0xFFFFFFFF, np.uint32)), np.ones((1, 32, 32, 32), bool))


def test_philox_statement_is_philox4x32_10():
    """Known-answer vectors of Philox4x32-10 (Random123 kat_vectors: zero counter / zero key, all ones, and the digits-of-pi one; the
    last two have non-zero keys, which pins the key-bump constants), then this project's placement of the 64-bit counter and seed
    in the words.  This test and the three after it check the statement alone (against the vectors and the host dataset): they
    hold without the device module; the module's own tests follow them."""
    hexes = lambda r: [f"{int(v):08x}" for v in r]         # noqa: E731
    assert hexes(S.philox4x32(0, 0)[0]) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = 0xFFFFFFFF
    assert hexes(S.philox4x32_words((ones,) * 4, (ones, ones))[0]) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    pi = S.philox4x32_words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    assert hexes(pi[0]) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    # seed placement: key {lo(seed), hi(seed)}, counter {lo(ctr), hi(ctr), 0, 0}
    placed = S.philox4x32_words((0x85A308D3, 0x243F6A88, 0, 0), (0x299F31D0, 0xA4093822))
    assert np.array_equal(S.philox4x32(0x243F6A8885A308D3, 0xA4093822299F31D0), placed)
    # counter words {lo, hi, 0, 0}: two counters that differ in the high word differ
    a, b = S.philox4x32([5, 5 + (1 << 32)], 9)
    assert not np.array_equal(a, b)
    assert np.array_equal(S.philox4x32([5], 9)[0], a)


def test_exact_size_equals_the_host_dataset(tmp_path):
    occ = S.ellipsoid_grid(3)
    m = int(occ.sum())
    got, count = S.cloud_fp32(S.pack(occ), m, seed=1, offset=0, slot=0)
    host, _ = _host_cloud(tmp_path, occ, m)
    assert count == m and got.dtype == np.float32 and got.shape == host.shape == (m, 3)
    assert np.abs(got.astype(np.float64) - host.astype(np.float64)).max() <= 1e-6
    assert abs(np.linalg.norm(got.astype(np.float64), axis=1).max() - 1.0) < 1e-6


def test_larger_cloud_gives_distinct_rows_in_scan_order(tmp_path):
    occ = S.ellipsoid_grid(4)
    m, n = int(occ.sum()), 256
    assert m > n
    _, full = _host_cloud(tmp_path, occ, n)
    for seed, slot in ((1, 0), (1, 3), (77, 0)):
        got, _ = S.cloud_fp32(S.pack(occ), n, seed=seed, offset=0, slot=slot)
        rows = S.resample_ordinals(m, n, seed, slot * S.CTR_SPAN)
        assert len(np.unique(rows)) == n and np.all(np.diff(rows) > 0) and rows.min() >= 0 and rows.max() < m
        assert np.abs(got.astype(np.float64) - full[rows].astype(np.float64)).max() <= 1e-6
    a = S.resample_ordinals(m, n, 1, 0)
    assert not np.array_equal(a, S.resample_ordinals(m, n, 1, 3 * S.CTR_SPAN)) and not np.array_equal(a, S.resample_ordinals(m, n, 77, 0))
    # the subset is uniform: over many keys every point is taken about n / m of the time
    hits = np.zeros(m)
    for seed in range(200):
        hits[S.resample_ordinals(m, n, seed, 0)] += 1
    assert abs(hits.mean() / 200 - n / m) < 1e-12 and hits.min() > 0 and np.abs(hits / 200 - n / m).max() < 0.2


def test_smaller_cloud_is_kept_whole_then_drawn_from(tmp_path):
    occ = S.ellipsoid_grid(5, blobs=1, rmin=2, rmax=4)
    m, n = int(occ.sum()), 512
    assert 2 <= m < n
    _, full = _host_cloud(tmp_path, occ, n)
    got, _ = S.cloud_fp32(S.pack(occ), n, seed=2, offset=0, slot=1)
    assert np.abs(got[:m].astype(np.float64) - full.astype(np.float64)).max() <= 1e-6
    rows = S.resample_ordinals(m, n, 2, S.CTR_SPAN)
    assert np.array_equal(rows[:m], np.arange(m)) and rows[m:].min() >= 0 and rows[m:].max() < m
    assert np.array_equal(got[m:], got[:m][rows[m:]]) and len(np.unique(rows[m:])) > 1


def _modules(root, **kw):
    torch.manual_seed(24)
    host = D.PointCloudDataDirectoryModule(root, num_points=64, batch_size=4, num_workers=0, augmentations=False, **kw)
    host.setup()
    torch.manual_seed(24)
    dev = D.DeviceVoxelDataModule(root, num_points=64, batch_size=4, augmentations=False, device="cpu", **kw)
    dev.setup()
    return host, dev


def test_split_labels_and_categories_equal_the_host_module(tmp_path):
    from shapegen_amd.training import split_fingerprint
    root = str(tmp_path / "dir")
    S.write_voxel_dir(root, 11)
    host, dev = _modules(root, return_labels=True)
    assert list(dev.train_dataset.indices) == list(host.train_dataset.indices) and len(dev.train_dataset.indices) == 8
    assert list(dev.val_dataset.indices) == list(host.val_dataset.indices)
    assert split_fingerprint(dev) == split_fingerprint(host) is not None
    full = host.train_dataset.dataset
    assert dev.categories == full.categories == ["airplane", "chair", "table"]
    assert dev.labels_device.tolist() == [int(full[i][1]) for i in range(len(full))]
    assert dev.packed.shape == (11, 1024) and dev.packed.dtype == torch.int32 and dev.packed.device.type == "cpu"
    for i in (0, 5, 10):                                   # the packed rows are the host dataset's thresholded grids, file by file
        vox = D.minmax_grid(D.load_sample_file(os.path.join(root, full.file_list[i])))
        assert np.array_equal(D.unpack_grids(dev.packed_host[i:i + 1])[0], vox > 0.5) and dev.counts[i] == (vox > 0.5).sum()
    host, dev = _modules(root, relevant_object_categories=["table"])
    assert dev.categories == [] and dev.labels_device is None and dev.packed.shape[0] == 4
    assert list(dev.train_dataset.indices) == list(host.train_dataset.indices)
    with pytest.raises(RuntimeError, match="GPU"):
        next(iter(dev.train_dataloader()))                 # no CPU path behind the loaders


def test_grids_argument_and_refusals(tmp_path):
    grids = np.stack([S.ellipsoid_grid(i) for i in range(5)]).astype(np.float32)
    dm = D.DeviceVoxelDataModule(grids=grids * 4.0, labels=[0, 1, 2, 0, 1], return_labels=True, num_points=64, device="cpu")
    dm.setup()
    assert np.array_equal(D.unpack_grids(dm.packed_host), grids > 0) and dm.labels_device.tolist() == [0, 1, 2, 0, 1]
    assert len(dm.train_dataset.indices) == 4 and len(dm.val_dataset.indices) == 1
    # `augmentations` is the host module's: the dataset's jitter, never its rotation (PointCloudDataDirectoryModule leaves rotate=False)
    assert dm.flags == S.NORMALIZE | S.JITTER and (dm.jitter_sigma, dm.jitter_clip) == (0.01, 0.05)
    flags = lambda **kw: D.DeviceVoxelDataModule(grids=grids, device="cpu", **kw).flags          # noqa: E731
    assert flags(augmentations=False) == S.NORMALIZE and flags(augmentations=False, normalization=False) == 0
    assert flags(rotate=True) == S.NORMALIZE | S.JITTER | S.ROTATE and flags(augmentations=False, rotate=True) == S.NORMALIZE | S.ROTATE
    with pytest.raises(ValueError):
        D.DeviceVoxelDataModule(grids=grids, output_mode="voxels", augmentations=False, rotate=True)

    def refuses(name, voxels, match, **kw):
        root = tmp_path / name
        S.write_voxel_dir(str(root), 2)
        bad = "vox_32_res_model_04379243_bad.npz"
        np.savez(root / bad, data=voxels)
        with pytest.raises(ValueError, match=match) as e:
            D.DeviceVoxelDataModule(str(root), device="cpu", augmentations=False, **kw).setup()
        assert bad in str(e.value)

    refuses("shape", np.zeros((16, 16, 16), np.float32), r"not \(32, 32, 32\)")
    one = np.zeros((32, 32, 32), np.float32)
    one[1, 2, 3] = 1
    refuses("single", one, "1 occupied voxels")
    refuses("constant", np.full((32, 32, 32), 0.25, np.float32), "0 occupied voxels")      # the dataset's lo == hi case: all 0.25, none above 0.5
    grey = S.ellipsoid_grid(1).astype(np.float32)
    grey[0, 0, 0] = 0.3
    refuses("grey", grey, "not binary", output_mode="voxels")
    with pytest.raises(ValueError):
        D.DeviceVoxelDataModule(str(tmp_path), file_mode="point_clouds")
    with pytest.raises(ValueError):
        D.DeviceVoxelDataModule()


def test_philox_spans_are_disjoint():
    """Two slots, and the four purposes inside a slot, never share a counter, for every N up to 32768 (and M up to 32768); the
    constants are the header's."""
    header = open(os.path.join(ROOT, "include", "pcd_hip.h")).read()
    const = dict(re.findall(r"#define PCD_VOXEL_CTR_(\w+) (.+)", header))
    value = lambda t: eval(t.split("/*")[0].replace("ull", ""))           # noqa: E731  ("8192ull", "(1ull << 24)")
    assert {k: value(v) for k, v in const.items()} == {"KEY": S.CTR_KEY, "ANGLE": S.CTR_ANGLE, "JITTER": S.CTR_JITTER, "DRAW": S.CTR_DRAW,
                                                       "SPAN": S.CTR_SPAN}
    assert D.VOXEL_CTR_SPAN == S.CTR_SPAN
    for n in (1, 64, 2048, 32767, 32768):
        for offset in (0, 7 * 16 * S.CTR_SPAN):
            a, b = S.span_ranges(n, 0, offset), S.span_ranges(n, 1, offset)
            parts = [a[k] for k in ("key", "angle", "jitter", "draw")]
            for i, (lo, hi) in enumerate(parts):
                assert a["span"][0] <= lo < hi <= a["span"][1]
                for lo2, hi2 in parts[i + 1:]:
                    assert hi <= lo2 or hi2 <= lo
            assert a["span"][1] <= b["span"][0]
    # and the ranges are the ones the statement really uses
    m = 32768
    assert (m + 3) // 4 == S.KEY_COUNTERS and m == S.JITTER_COUNTERS
