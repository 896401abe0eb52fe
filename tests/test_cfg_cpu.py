"""Class conditioning with classifier-free guidance, the parts that need no GPU: the boundary (symbols, version), argument
validation on the host, the state_dict / checkpoint contract with and without classes, the data layer's labels, label dropout
and the float statement (tests/cfg_statement.py) against the unconditional oracle."""
import os
import re

import numpy as np
import pytest
import torch

import cfg_statement as S
from helpers import point_sd
from oracle import torch_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcd_step_select_labels", "pcd_cfg_combine", "pcd_embed_add_rows", "pcd_embed_rows_backward")


def _model(num_classes=0, **kw):
    from shapegen_amd.diffusion import PointCloudDiffusion
    return PointCloudDiffusion(num_points=32, num_classes=num_classes, **kw)


def test_symbols_declared_exported_bound_version_2():
    from shapegen_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcd_hip.h")).read(), flags=re.S)
    _lib.build()
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib._SIGS and hasattr(lib, name), name
    assert "#define PCD_ABI_VERSION 2" in header and lib.pcd_abi_version() == _lib.ABI_VERSION == 2
    # argument errors are reported before any device work (pointers are never dereferenced on the host)
    p = 64
    assert lib.pcd_cfg_combine(0, p, p, 0, 12, 4, 0) == -1 and lib.pcd_cfg_combine(p, p, p, 2, 12, 4, 0) == -1
    assert lib.pcd_cfg_combine(p, p, p, 0, 0, 4, 0) == -1
    assert lib.pcd_step_select_labels(p, 5, p, 64, p, p, 4, p, 3, 4, p, 4, 1, p, 0) == -1          # null_row outside the table
    assert lib.pcd_step_select_labels(p, 5, p, 64, p, p, 4, 0, 3, 3, p, 4, 1, p, 0) == -1          # no labels
    assert lib.pcd_embed_add_rows(p, p, p, 0, 256, 4, 0) == -1 and lib.pcd_embed_rows_backward(p, p, 5, 256, 0, p, 0) == -1
    assert b"bad argument" in lib.pcd_last_error()


def test_label_and_scale_validation():
    m, m0 = _model(3), _model(0)
    for bad in ([0.0, 1.0, 2.0], [True, False, True], [0, 1, 4], [0, -1, 2], [0, 1], [[0, 1, 2]]):
        with pytest.raises(ValueError):
            m._guide(bad, 1.0, 3)
    for bad in (float("nan"), float("inf"), torch.tensor([1.0, 2.0]), torch.ones(3, 1), torch.tensor([1.0, float("nan"), 2.0])):
        with pytest.raises(ValueError):
            m._guide([0, 1, 3], bad, 3)
    with pytest.raises(ValueError, match="without classes"):
        m0._guide([0, 1, 2], 1.0, 3)
    with pytest.raises(ValueError, match="without classes"):
        m0.sample(3, 32, num_steps=2, labels=torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError):
        m0._guide(None, 2.0, 3)
    assert m0._guide(None, 1.0, 3) is None and m0._guide(None, torch.ones(3), 3) is None
    lab = m.model.check_labels(None, 4)
    assert lab.dtype == torch.int32 and lab.tolist() == [3, 3, 3, 3]            # labels=None: the null class
    assert m.model.check_labels([2, 0, 3], 3).tolist() == [2, 0, 3]
    assert m.model.check_labels(torch.tensor([1, 1], dtype=torch.int64), 2).dtype == torch.int32
    with pytest.raises(ValueError):
        m.sample_dpm(3, 32, num_steps=4, labels=[0, 1, 7])                        # raised on the host, before any device work
    with pytest.raises(ValueError):
        m.complete(torch.zeros(3, 8, 3), 32, num_steps=4, labels=[0.5, 1, 2])
    from shapegen_amd.diffusion import LatentDiffusion, PointCloudDiffusion
    with pytest.raises(ValueError):
        PointCloudDiffusion(num_points=32, backbone="attention", num_classes=2)
    with pytest.raises(ValueError):
        PointCloudDiffusion(num_points=32, num_classes=-1)
    with pytest.raises(ValueError):
        PointCloudDiffusion(num_points=32, num_classes=2, p_uncond=1.5)
    with pytest.raises(ValueError):
        LatentDiffusion(torch.nn.Linear(1, 1), num_classes=2)


def test_state_dict_keys_order_and_hparams():
    m0, m = _model(0), _model(3, p_uncond=0.2)
    k0, k = list(m0.state_dict()), list(m.state_dict())
    assert len(k0) == 203 and k == k0 + ["model.class_emb.weight"]
    assert tuple(m.state_dict()["model.class_emb.weight"].shape) == (4, 256)
    assert "num_classes" not in m0.hparams and "p_uncond" not in m0.hparams
    assert m.hparams["num_classes"] == 3 and m.hparams["p_uncond"] == 0.2
    # what a torch user builds: an nn.Embedding registered after the reference's modules gives the same key, position and init
    class Twin(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.output = torch.nn.Linear(2, 2)
            self.class_emb = torch.nn.Embedding(4, 256)
    torch.manual_seed(5)
    twin = Twin()
    torch.manual_seed(5)
    torch.nn.Linear(2, 2)
    want = torch.nn.Embedding(4, 256).weight
    assert list(twin.state_dict())[-1] == "class_emb.weight" and torch.equal(twin.class_emb.weight, want)
    from shapegen_amd.networks import UNetPointNetLarge
    assert isinstance(UNetPointNetLarge(256, 256, 3).class_emb, torch.nn.Embedding)
    assert [n for n, _ in m.model.named_parameters()][-1] == "class_emb.weight"
    # loading is strict both ways
    with pytest.raises(RuntimeError):
        m.load_state_dict(m0.state_dict(), strict=True)
    with pytest.raises(RuntimeError):
        m0.load_state_dict(m.state_dict(), strict=True)


def test_checkpoints_old_and_new(tmp_path):
    from shapegen_amd.diffusion import PointCloudDiffusion
    from shapegen_amd.training import save_checkpoint
    # a file from before class conditioning: no num_classes / p_uncond in its hyper-parameters, 203 tensors
    old = str(tmp_path / "old.ckpt")
    sd = point_sd()
    torch.save({"state_dict": sd, "hyper_parameters": {"num_points": 32, "dim": 256, "time_dim": 256, "lr": 1e-4,
                                                        "noise_schedule": "cosine"}}, old)
    m0 = PointCloudDiffusion.load_from_checkpoint(old)
    assert m0.num_classes == 0 and not hasattr(m0.model, "class_emb") and len(m0.state_dict()) == 203
    assert torch.equal(m0.state_dict()["model.output.3.weight"], sd["model.output.3.weight"])
    # round trip of a class model
    m = _model(3, p_uncond=0.25)
    new = str(tmp_path / "new.ckpt")
    save_checkpoint(m, new, epoch=0)
    ck = torch.load(new, map_location="cpu", weights_only=False)
    assert ck["hyper_parameters"]["num_classes"] == 3 and ck["hyper_parameters"]["p_uncond"] == 0.25
    assert list(ck["state_dict"])[-1] == "model.class_emb.weight" and len(ck["state_dict"]) == 204
    back = PointCloudDiffusion.load_from_checkpoint(new)
    assert back.num_classes == 3 and back.p_uncond == 0.25 and back.model.num_classes == 3
    assert torch.equal(back.state_dict()["model.class_emb.weight"], m.state_dict()["model.class_emb.weight"])
    save_checkpoint(m0, str(tmp_path / "again.ckpt"), epoch=0)
    assert "num_classes" not in torch.load(str(tmp_path / "again.ckpt"), weights_only=False)["hyper_parameters"]


def test_dataset_labels(tmp_path):
    from shapegen_amd.data import PointCloudDataDirectoryModule, PointCloudDataModule, PointCloudDataset
    ids = {"03001627": "chair", "02691156": "airplane", "04379243": "table"}
    rng = np.random.default_rng(0)
    names = []
    for i, syn in enumerate(["03001627", "02691156", "04379243", "03001627", "02691156"]):
        name = f"model_normalized_solid_{i}_{syn}_abc{i}.npz"
        np.savez(tmp_path / name, data=(rng.random((8, 8, 8)) > 0.6).astype(np.float32))
        names.append(name)
    ds = PointCloudDataset(str(tmp_path), num_points=16, output_mode="point_clouds", jitter=False, return_labels=True)
    assert ds.categories == ["airplane", "chair", "table"]
    for i in range(len(ds)):
        cloud, label = ds[i]
        assert cloud.shape == (16, 3) and label.dtype == torch.int64 and label.dim() == 0
        assert ds.categories[int(label)] == ids[ds.file_list[i].split("_")[4]]
    # labels index the categories that survive the filter
    ds2 = PointCloudDataset(str(tmp_path), num_points=16, output_mode="point_clouds", jitter=False, return_labels=True,
                            relevant_object_categories=["table", "chair"])
    assert ds2.categories == ["chair", "table"] and len(ds2) == 3
    assert sorted(int(ds2[i][1]) for i in range(3)) == [0, 0, 1]
    # default off: an item is the tensor it was
    plain = PointCloudDataset(str(tmp_path), num_points=16, output_mode="point_clouds", jitter=False)
    assert isinstance(plain[0], torch.Tensor) and plain.categories == []
    with pytest.raises(ValueError):
        PointCloudDataset(str(tmp_path), input_mode="point_clouds", return_labels=True)
    dm = PointCloudDataDirectoryModule(str(tmp_path), num_points=16, batch_size=2, num_workers=0, augmentations=False, return_labels=True)
    dm.setup()
    clouds, labels = next(iter(dm.train_dataloader()))
    assert clouds.shape == (2, 16, 3) and labels.shape == (2,) and labels.dtype == torch.int64 and dm.categories == ds.categories
    mem = PointCloudDataModule(np.zeros((10, 16, 3), np.float32), batch_size=4, labels=np.arange(10) % 3)
    mem.setup()
    c, l = next(iter(mem.train_dataloader()))
    assert c.shape == (4, 16, 3) and l.dtype == torch.int64 and l.shape == (4,)
    mem0 = PointCloudDataModule(np.zeros((10, 16, 3), np.float32), batch_size=4)
    mem0.setup()
    assert len(next(iter(mem0.train_dataloader()))) == 1                         # batches are what they were
    with pytest.raises(ValueError):
        PointCloudDataModule(np.zeros((10, 16, 3), np.float32), labels=[0, 1])


def test_label_dropout_is_seeded_and_absent_without_classes():
    m = _model(3, p_uncond=0.5)
    labels = torch.arange(64) % 3
    torch.manual_seed(11)
    a = m._training_labels(labels, 64, True)
    torch.manual_seed(11)
    b = m._training_labels(labels, 64, True)
    assert torch.equal(a, b)
    dropped = a == 3
    assert 8 < int(dropped.sum()) < 56 and torch.equal(a[~dropped].long(), labels[~dropped])
    # the draw is torch.rand(B) < p_uncond on the model's device, one draw
    torch.manual_seed(11)
    assert torch.equal(dropped, torch.rand(64) < 0.5)
    # validation: labels as given, no draw
    state = torch.get_rng_state()
    assert torch.equal(m._training_labels(labels, 64, False).long(), labels) and torch.equal(torch.get_rng_state(), state)
    # p_uncond 0 / 1
    assert torch.equal(_model(3, p_uncond=0.0)._training_labels(labels, 64, True).long(), labels)
    assert bool((_model(3, p_uncond=1.0)._training_labels(labels, 64, True) == 3).all())
    # a model without classes draws nothing: the random stream of an unconditional run is what it was
    m0 = _model(0)
    state = torch.get_rng_state()
    assert m0._training_labels(None, 64, True) is None and torch.equal(torch.get_rng_state(), state)
    with pytest.raises(ValueError):
        m0._training_labels(labels, 64, True)
    assert m0._split_batch(torch.zeros(2, 3))[1] is None and m._split_batch([torch.zeros(2, 3), torch.tensor([0, 1])])[1].tolist() == [0, 1]


def test_guidance_shard_slices_labels_and_scales():
    from shapegen_amd import dist as D
    assert D._guidance_shard(None, 1.0, 2, 4) == {}
    kw = D._guidance_shard(torch.tensor([0, 1, 2, 3]), torch.tensor([1.0, 2.0, 3.0, 4.0]), 1, 3)
    assert kw["labels"].tolist() == [1, 2] and kw["guidance_scale"].tolist() == [2.0, 3.0]
    kw = D._guidance_shard([0, 1, 2, 3], 2.0, 2, 4)
    assert kw["labels"].tolist() == [2, 3] and kw["guidance_scale"] == 2.0


def test_statement_with_null_labels_and_zero_null_row_is_the_unconditional_oracle():
    sd = point_sd()
    g = torch.Generator().manual_seed(3)
    E = torch.randn(4, 256, generator=g)
    E[3] = 0.0
    x, t = torch.randn(2, 32, 3, generator=g), torch.tensor([0.3, 0.8])
    inner = O.time_mlp
    with torch.no_grad():
        want = O.unet_pointnet_large(sd, "model.", x, t)
        assert torch.equal(S.eps_of(sd, "model.", E, [3, 3], x, t), want)
        assert O.time_mlp is inner                                               # the oracle is restored
        assert not torch.equal(S.eps_of(sd, "model.", E, [0, 3], x, t)[0], want[0])
        assert torch.equal(S.eps_of(sd, "model.", E, [0, 3], x, t)[1], want[1])  # shapes are independent in eval mode
        x_T = torch.randn(2, 32, 3, generator=g)
        uncond = O.ddim_sample(lambda a, b: O.unet_pointnet_large(sd, "model.", a, b), x_T, 3)
        assert torch.equal(S.sample("ddim", sd, "model.", E, [3, 3], 1.0, x_T, 3), uncond)
        # guidance between two equal predictions changes nothing beyond rounding: eu + w (eu - eu) = eu
        assert torch.equal(S.sample("ddim", sd, "model.", E, [3, 3], 2.0, x_T, 3), uncond)
    with pytest.raises(RuntimeError):
        with S.class_term(E, [0, 0]):
            raise RuntimeError("x")
    assert O.time_mlp is inner
    # the training statement: E's gradient exists, rows of unused classes are exactly zero, the others are not
    xt, tt, nz = torch.randn(2, 32, 3, generator=g), torch.tensor([0.2, 0.7]), torch.randn(2, 32, 3, generator=g)
    loss, grads = S.training_step({k: v.clone() for k, v in sd.items()}, "model.", E, [1, 3], xt, tt, nz)
    ge = grads["model.class_emb.weight"]
    assert ge.shape == (4, 256) and bool((ge[0] == 0).all() and (ge[2] == 0).all()) and float(ge[1].abs().max()) > 0 and float(ge[3].abs().max()) > 0
    assert len(grads) == 123 and torch.isfinite(loss)
