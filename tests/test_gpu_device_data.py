"""The device-resident voxel dataset on the GPU: `pcd_voxel_batch_clouds` against the numpy statement (tests/device_data_statement.py)
bit for bit without augmentation and within fp32 rounding of its float64 form with it, `pcd_voxel_batch_grids`, the argument errors,
and `data.DeviceVoxelDataModule` through its loaders, `training.fit`, a resumed run and the entry script."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import device_data_statement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, OFFSET = 0x1234567, 5 * 16 * S.CTR_SPAN
COUNTS = (2, 63, 64, 65, 300, 32768)


@functools.lru_cache(maxsize=None)
def table():
    """The packed test grids, built once: random grids with COUNTS voxels, the two layout-edge pairs, two ellipsoid grids for
    N = 2048 (fewer and more voxels than that)."""
    occ = [S.grid_with_count(m, 100 + m) for m in COUNTS]
    corners = np.zeros((32, 32, 32), bool)
    corners[0, 0, 0] = corners[31, 31, 31] = True          # (word 0, bit 0) + (word 1023, bit 31)
    pair = np.zeros((32, 32, 32), bool)
    pair[17, 9, 4] = pair[17, 9, 30] = True                # two bits of one word
    small, large = S.ellipsoid_grid(8, blobs=1, rmin=4, rmax=7), S.ellipsoid_grid(9, blobs=3, rmin=7, rmax=11)
    assert 2 <= small.sum() < 2048 < large.sum()
    occ += [corners, pair, small, large]
    words = np.stack([S.pack(g) for g in occ])
    words.setflags(write=False)
    return words


def clouds(words, index, n, seed=SEED, offset=OFFSET, flags=S.NORMALIZE, sigma=0.01, clip=0.05):
    from shapegen_amd import _lib as L
    L.require_gpu()
    packed = torch.from_numpy(np.array(words).view(np.int32)).to(DEV)
    idx = torch.tensor(index, dtype=torch.int32, device=DEV)
    out = torch.full((len(index), n, 3), float("nan"), device=DEV)
    counts = torch.full((len(index),), -7, dtype=torch.int32, device=DEV)
    L.check(L.load().pcd_voxel_batch_clouds(L.ptr(packed), packed.shape[0], L.ptr(idx), len(index), n, seed, offset, flags, sigma, clip,
                                            L.ptr(out), L.ptr(counts), L.stream_ptr()), "voxel_batch_clouds")
    return out.cpu().numpy(), counts.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_unaugmented_batch_is_the_statement_bit_for_bit():
    words = table()
    index = list(range(8))
    got, counts = clouds(words, index, 64)
    assert counts.tolist() == list(COUNTS) + [2, 2]
    for b, g in enumerate(index):
        want, m = S.cloud_fp32(words[g], 64, SEED, OFFSET, b)
        assert m == counts[b] and same_bits(got[b], want), (b, m, np.abs(got[b] - want).max())
    assert np.isfinite(got).all()
    # without the normalisation the rows are the integer coordinates themselves
    raw, _ = clouds(words, [6, 7, 3], 64, flags=0)
    for b, g in enumerate((6, 7, 3)):
        assert same_bits(raw[b], S.cloud_fp32(words[g], 64, SEED, OFFSET, b, normalize=False)[0])
    assert raw[0][:2].tolist() == [[0, 0, 0], [31, 31, 31]] and raw[1][:2].tolist() == [[17, 9, 4], [17, 9, 30]]


def test_unaugmented_2048_points_fewer_and_more_voxels():
    """NOT covered here or anywhere: the radix select's tie branch with more than one key equal to the cut (`ties` > 1 in
    csrc/dataset.hip).  It needs two equal 32-bit Philox keys at the cut, which none of the test keys produce; with distinct keys
    exactly one point equals the cut and `ties` is 1."""
    words = table()
    for g, n in ((4, 64), (9, 2048)):
        k = S.keys(int(S.scan_points(words[g]).shape[0]), SEED, OFFSET + (1 if g == 9 else 4) * S.CTR_SPAN)
        assert len(np.unique(k)) == len(k)                   # distinct keys: the statement above is a fact, not a guess
    got, counts = clouds(words, [8, 9], 2048)
    for b, g in enumerate((8, 9)):
        want, m = S.cloud_fp32(words[g], 2048, SEED, OFFSET, b)
        assert m == counts[b] and same_bits(got[b], want), (b, m)
    assert counts[0] < 2048 < counts[1]


def test_a_slot_does_not_depend_on_its_companions_and_keys_move_the_subset():
    words = table()
    a, _ = clouds(words, [0, 4, 9, 1], 64)
    b, _ = clouds(words, [5, 4, 2, 1], 64)
    assert same_bits(a[1], b[1]) and same_bits(a[3], b[3]) and not same_bits(a[0], b[0])
    c, _ = clouds(words, [0, 4, 9, 1], 64, offset=OFFSET + 4 * S.CTR_SPAN)
    d, _ = clouds(words, [0, 4, 9, 1], 64, seed=SEED + 1)
    assert not same_bits(a[1], c[1]) and not same_bits(a[1], d[1]) and not same_bits(a[2], c[2]) and not same_bits(a[2], d[2])
    assert same_bits(a[0][:2], c[0][:2]) and same_bits(a[0][:2], d[0][:2]) and not same_bits(a[0], c[0])   # M = 2 < N: the cloud first, then draws
    g, _ = clouds(words, [2], 64)
    h, _ = clouds(words, [2], 64, seed=SEED + 1, offset=0)
    assert same_bits(g, h)                                                    # M = N: no draw enters
    e, _ = clouds(words, [7, 7, 7, 7, 4], 64, offset=OFFSET)                 # slot 4 of this batch = slot 0 of a batch 4 spans on
    f, _ = clouds(words, [4], 64, offset=OFFSET + 4 * S.CTR_SPAN)
    assert same_bits(e[4], f[0])


@pytest.mark.parametrize("clip", [0.05, 0.005], ids=["clip-idle", "clip-binds"])
@pytest.mark.parametrize("flags", [S.ROTATE | S.JITTER | S.NORMALIZE, S.ROTATE | S.NORMALIZE, S.JITTER | S.NORMALIZE],
                         ids=["rotate+jitter", "rotate", "jitter"])
def test_augmented_against_the_float64_statement(flags, clip):
    """Coordinates are O(1); about ten fp32 roundings of 6e-8 each plus the device's logf / sincosf leave more than 10x margin under
    the absolute 1e-5.  The subset is decided by integer keys, so rows pair up exactly.  With sigma 0.01 the dataset's clip of 0.05
    needs a normal beyond 5 and never binds here; 0.005 binds for every normal beyond 0.5, most of them.  (clip(x) is continuous,
    so a normal that lands on the other side of the bound in fp32 moves the row by rounding only.)"""
    words = table()
    index = [3, 4, 4]                                       # M = 65, 300, and 300 again under another slot's streams
    got, counts = clouds(words, index, 64, flags=flags, clip=clip)
    assert counts.tolist() == [65, 300, 300]
    if flags & S.JITTER:
        bound = np.abs(0.01 * S.normals(300, SEED, OFFSET + S.CTR_SPAN)) > clip
        assert bound.any() == (clip < 0.05) and (clip == 0.05 or bound.mean() > 0.5)
    worst = 0.0
    for b, g in enumerate(index):
        want, _ = S.cloud_f64(words[g], 64, SEED, OFFSET, b, flags, clip=clip)
        worst = max(worst, float(np.abs(got[b].astype(np.float64) - want).max()))
    print(f"flags {flags} clip {clip}: max abs difference to float64 {worst:.3e}")
    assert worst <= 1e-5
    assert np.linalg.norm(got.astype(np.float64), axis=2).max() <= 1 + 1e-5
    assert not same_bits(got[1], got[2])
    again, _ = clouds(words, index, 64, flags=flags, clip=clip)
    assert same_bits(got, again)                            # fixed-order float sums: bitwise repeatable


def test_grids_kernel_unpacks_exactly():
    from shapegen_amd import _lib as L
    L.require_gpu()
    words = table()
    index = [9, 0, 5, 9, 6, 2]                              # permuted, with a repeat
    packed = torch.from_numpy(words.view(np.int32).copy()).to(DEV)
    idx = torch.tensor(index, dtype=torch.int32, device=DEV)
    out = torch.full((len(index), 1, 32, 32, 32), float("nan"), device=DEV)
    L.check(L.load().pcd_voxel_batch_grids(L.ptr(packed), packed.shape[0], L.ptr(idx), len(index), L.ptr(out), L.stream_ptr()), "grids")
    want = np.stack([S.unpack(words[g]) for g in index]).astype(np.float32)[:, None]
    assert np.array_equal(out.cpu().numpy(), want)


def test_bad_arguments_return_minus_one():
    from shapegen_amd import _lib as L
    L.require_gpu()
    lib = L.load()
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    out = torch.zeros(4 * 64 * 3, device=DEV)
    p, o = L.ptr(buf), L.ptr(out)
    good = (p, 4, p, 4, 64, 1, 0, 1, 0.01, 0.05, o, p, L.stream_ptr())
    for pos, bad in ((0, 0), (2, 0), (10, 0), (11, 0), (3, 0), (3, -1), (4, 0), (4, -5), (1, 0), (7, 8)):
        args = list(good)
        args[pos] = bad
        assert lib.pcd_voxel_batch_clouds(*args) == -1 and b"bad argument" in lib.pcd_last_error(), pos
    good = (p, 4, p, 4, o, L.stream_ptr())
    for pos, bad in ((0, 0), (2, 0), (4, 0), (3, 0), (3, -2), (1, 0)):
        args = list(good)
        args[pos] = bad
        assert lib.pcd_voxel_batch_grids(*args) == -1 and b"bad argument" in lib.pcd_last_error(), pos
    assert not out.any() and not buf.any()                  # refused before any device work


# ---------------------------------------------------------------------------------------------- the module
@functools.lru_cache(maxsize=None)
def synthetic(count):
    g = np.stack([S.ellipsoid_grid(500 + i) for i in range(count)]).astype(np.float32)
    g.setflags(write=False)
    return g


def _module(count=32, **kw):
    from shapegen_amd.data import DeviceVoxelDataModule
    return DeviceVoxelDataModule(grids=synthetic(count), num_points=64, batch_size=4, **{"augmentations": False, **kw})


def test_two_instances_yield_the_same_batches_and_match_the_statement():
    runs = []
    for _ in range(2):
        torch.manual_seed(24)
        dm = _module(11, labels=np.arange(11) % 3, return_labels=True)
        dm.setup()
        seq = [[(c.cpu(), l.cpu()) for c, l in dm.train_dataloader()] for _ in range(2)]
        runs.append((seq, [(c.cpu(), l.cpu()) for c, l in dm.val_dataloader()]))
    (a, va), (b, vb) = runs
    for ea, eb in zip(a, b):
        assert [c.shape[0] for c, _ in ea] == [4, 4] and len(ea) == len(eb)         # 8 training grids
        assert all(torch.equal(c, d) and torch.equal(l, m) for (c, l), (d, m) in zip(ea, eb))
    assert not all(torch.equal(c, d) for (c, _), (d, _) in zip(a[0], a[1]))         # the second epoch is another shuffle / key
    assert all(torch.equal(c, d) and torch.equal(l, m) for (c, l), (d, m) in zip(va, vb))
    clouds_, labels = va[0]
    assert clouds_.device.type == "cpu" and clouds_.shape == (3, 64, 3) and labels.dtype == torch.int64
    # the validation loader: in order, fixed key; each row is the statement's
    from shapegen_amd.data import VAL_KEY
    rows = list(dm.val_dataset.indices)
    assert labels.tolist() == [r % 3 for r in rows]
    for b_, r in enumerate(rows):
        assert same_bits(clouds_[b_].numpy(), S.cloud_fp32(dm.packed_host[r], 64, VAL_KEY, 0, b_)[0])
    first = next(iter(dm.train_dataloader()))
    assert first[0].is_cuda and first[1].is_cuda
    vox = _module(11, output_mode="voxels")
    vox.setup()
    batch = next(iter(vox.val_dataloader()))
    assert batch.is_cuda and batch.shape == (3, 1, 32, 32, 32)
    assert np.array_equal(batch.cpu().numpy()[:, 0], synthetic(11)[list(vox.val_dataset.indices)])


def test_module_augmentations_mean_jitter_and_rotate_is_opt_in():
    """`augmentations=True`, the constructor default, is the host module's: jitter, no rotation.  The validation loader's rows
    (in order, fixed key) are the float64 statement's under JITTER | NORMALIZE; `rotate=True` adds the rotation."""
    from shapegen_amd.data import VAL_KEY
    for rotate, flags in ((False, S.JITTER | S.NORMALIZE), (True, S.ROTATE | S.JITTER | S.NORMALIZE)):
        torch.manual_seed(24)
        dm = _module(11, **{"augmentations": True, "rotate": rotate})
        dm.setup()
        assert dm.flags == flags
        (batch,) = list(dm.val_dataloader())
        got = batch.cpu().numpy().astype(np.float64)
        for b, r in enumerate(dm.val_dataset.indices):
            want, _ = S.cloud_f64(dm.packed_host[r], 64, VAL_KEY, 0, b, flags)
            assert np.abs(got[b] - want).max() <= 1e-5, (rotate, b)
        plain, _ = S.cloud_f64(dm.packed_host[dm.val_dataset.indices[0]], 64, VAL_KEY, 0, 0, S.NORMALIZE)
        assert np.abs(got[0] - plain).max() > 1e-4             # and not the unaugmented cloud


def _fit(**kw):
    from shapegen_amd.diffusion import PointCloudDiffusion
    from shapegen_amd.training import fit
    torch.manual_seed(7)
    model = PointCloudDiffusion(num_points=64).to(DEV)
    history = fit(model, _module(32), log=lambda *_: None, **kw)
    return model, history


def _state(model):
    tr = model._trainer
    out = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    out["exp_avg"], out["exp_avg_sq"] = tr.M1.cpu().clone(), tr.M2.cpu().clone()
    return out


def test_fit_and_resume_with_the_device_module(tmp_path):
    """Two epochs on 32 synthetic grids (25 train: six batches of 4 and one of 1, all multiples of 64 rows) end with finite losses;
    one epoch, `save_last`, a fresh model and module, `ckpt_path`, one more epoch gives bitwise the weights and moments of the two
    epochs straight (the epoch permutation and key come from the global generator, restored with the loop state)."""
    straight, h = _fit(max_epochs=2)
    assert len(h) == 2 and all(np.isfinite(v) for e in h for v in e[1:3])
    want = _state(straight)
    del straight
    first, h1 = _fit(max_epochs=2, max_steps=7, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True)
    assert len(h1) == 1
    del first
    resumed, h2 = _fit(max_epochs=2, ckpt_path=str(tmp_path / "run-last.ckpt"), ckpt_dir=str(tmp_path), ckpt_name="run")
    assert [e[0] for e in h2] == [0, 1]
    got = _state(resumed)
    assert list(got) == list(want)
    assert [k for k in want if not torch.equal(want[k], got[k])] == []


def test_train_point_ddpm_device_data_entry(tmp_path):
    """`train_point_ddpm.py --device-data` on a tiny generated directory, in a fresh process."""
    S.write_voxel_dir(str(tmp_path / "vox"), 10, synsets=("03001627",))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_point_ddpm.py"), "--device-data", "--data-dir", str(tmp_path / "vox"),
                        "--category", "chair", "--num-points", "64", "--batch-size", "4", "--epochs", "1", "--max-steps", "2",
                        "--sample-steps", "2", "--out", str(tmp_path / "p")], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert np.load(tmp_path / "p" / "samples.npy").shape == (10, 64, 3)
    import glob
    assert "epoch 0: train_loss" in open(glob.glob(str(tmp_path / "train" / "logs" / "*.log"))[0]).read()
