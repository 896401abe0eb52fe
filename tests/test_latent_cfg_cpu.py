"""Class-conditional latent diffusion, the parts that need no GPU: construction and the state-dict / checkpoint contract, the
refusals (host-side validation before any device work), the float statement (tests/latent_cfg_statement.py) against itself
and the unconditional oracle, the training batch split with its label drop, and the argument checks of the two guided
entries of the persistent launch."""
import os
import re

import pytest
import torch

import latent_cfg_statement as S
from helpers import latent_sd, rel_l2
from oracle import torch_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcd_latent_persist_ddim_guided", "pcd_latent_persist_forward_guided")


class _Vae(torch.nn.Module):
    """A stand-in for the frozen VAE: two parameters, encode / reparameterize on the host."""

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(2, 2)

    def encode(self, x):
        return x.reshape(x.shape[0], -1)[:, :256], torch.zeros(x.shape[0], 256)

    def reparameterize(self, mu, logvar):
        return mu


def _model(num_classes=3, **kw):
    from shapegen_amd.diffusion import ConditionalLatentDiffusion
    return ConditionalLatentDiffusion(_Vae(), num_classes, **kw)


def _plain():
    from shapegen_amd.diffusion import LatentDiffusion
    return LatentDiffusion(_Vae())


def test_construction_and_state_dict_order():
    from shapegen_amd.diffusion import ConditionalLatentDiffusion, LatentDiffusion
    from shapegen_amd.networks import SimpleLatentUNetPointNet
    m0, m = _plain(), _model(3, p_uncond=0.2)
    assert isinstance(m, LatentDiffusion) and issubclass(ConditionalLatentDiffusion, LatentDiffusion)
    k0, k = list(m0.state_dict()), list(m.state_dict())
    assert k == k0 + ["model.class_emb.weight"]
    assert tuple(m.state_dict()["model.class_emb.weight"].shape) == (4, 256)
    assert [n for n, _ in m.model.named_parameters()][-1] == "class_emb.weight"
    assert isinstance(m.model.class_emb, torch.nn.Embedding)
    # a denoiser without classes is what it was
    d0 = SimpleLatentUNetPointNet(256, 512, 256, 0.1)
    assert list(d0.state_dict()) == [key[len("model."):] for key in k0 if key.startswith("model.")]
    assert not hasattr(d0, "class_emb") and d0.num_classes == 0
    assert list(SimpleLatentUNetPointNet(256, 512, 256, 0.1, num_classes=0).state_dict()) == list(d0.state_dict())
    assert "num_classes" not in m0.hparams and "p_uncond" not in m0.hparams
    assert m.hparams["num_classes"] == 3 and m.hparams["p_uncond"] == 0.2 and m.num_classes == 3 and m.model.num_classes == 3
    with pytest.raises(RuntimeError):
        m.load_state_dict(m0.state_dict(), strict=True)
    with pytest.raises(RuntimeError):
        m0.load_state_dict(m.state_dict(), strict=True)
    for bad in (dict(num_classes=0), dict(num_classes=-2), dict(num_classes=2, p_uncond=1.5)):
        with pytest.raises(ValueError):
            ConditionalLatentDiffusion(_Vae(), **bad)
    with pytest.raises(ValueError):
        SimpleLatentUNetPointNet(256, num_classes=-1)


def test_checkpoint_round_trip_raw_and_ema(tmp_path):
    from shapegen_amd.diffusion import ConditionalLatentDiffusion, LatentDiffusion
    from shapegen_amd.training import save_checkpoint
    m = _model(3, p_uncond=0.25)
    ema = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ema["model.class_emb.weight"] = ema["model.class_emb.weight"] * 0.5
    path = str(tmp_path / "cond.ckpt")
    save_checkpoint(m, path, epoch=0, extra={"ema_state_dict": ema})
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["hyper_parameters"]["num_classes"] == 3 and ck["hyper_parameters"]["p_uncond"] == 0.25
    assert list(ck["state_dict"])[-1] == "model.class_emb.weight" and tuple(ck["state_dict"]["model.class_emb.weight"].shape) == (4, 256)
    back = ConditionalLatentDiffusion.load_from_checkpoint(path, vae=_Vae())
    assert back.num_classes == 3 and back.p_uncond == 0.25 and back.model.num_classes == 3 and back.hparams == m.hparams
    assert torch.equal(back.state_dict()["model.class_emb.weight"], m.state_dict()["model.class_emb.weight"])
    avg = ConditionalLatentDiffusion.load_from_checkpoint(path, vae=_Vae(), weights="ema")
    assert torch.equal(avg.state_dict()["model.class_emb.weight"], ema["model.class_emb.weight"])
    with pytest.raises(TypeError):
        ConditionalLatentDiffusion.load_from_checkpoint(path)
    # a file of an unconditional model keeps its hyper-parameters and loads as before
    plain = str(tmp_path / "plain.ckpt")
    save_checkpoint(_plain(), plain, epoch=0)
    assert "num_classes" not in torch.load(plain, weights_only=False)["hyper_parameters"]
    assert LatentDiffusion.load_from_checkpoint(plain, vae=_Vae()).num_classes == 0


def test_refusals_on_the_host():
    from shapegen_amd.diffusion import LatentDiffusion, PointCloudDiffusion
    with pytest.raises(ValueError):
        LatentDiffusion(torch.nn.Linear(1, 1), num_classes=2)
    with pytest.raises(ValueError):
        PointCloudDiffusion(num_points=32, backbone="attention", num_classes=2)
    m, m0 = _model(3), _plain()
    # raised before any device work: these models sit on the host, where a sampler that got further would raise RuntimeError
    for bad in ([0, 1], [0.0, 1.0, 2.0], [True, False, True], [0, 1, 4], [0, -1, 2], [[0, 1, 2]]):
        for call in (lambda: m.sample(3, num_steps=4, labels=bad), lambda: m.sample2(3, num_steps=4, labels=bad),
                     lambda: m.sample3(3, num_steps=4, labels=bad), lambda: m.sample_dpm(3, num_steps=4, labels=bad)):
            with pytest.raises(ValueError):
                call()
    for bad in (float("nan"), float("inf"), torch.tensor([1.0, 2.0]), torch.ones(3, 1), torch.tensor([1.0, float("nan"), 2.0])):
        with pytest.raises(ValueError):
            m.sample(3, num_steps=4, labels=[0, 1, 3], guidance_scale=bad)
        with pytest.raises(ValueError):
            m.sample_dpm(3, num_steps=4, labels=[0, 1, 3], guidance_scale=bad)
    with pytest.raises(ValueError, match="without classes"):
        m0.sample(3, num_steps=4, labels=torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError, match="without classes"):
        m0.sample3(3, num_steps=4, labels=[0, 1, 2])
    with pytest.raises(ValueError):
        m0.sample(3, num_steps=4, guidance_scale=2.0)
    with pytest.raises(ValueError, match="without classes"):
        m0.model.check_labels([0, 1], 2)
    assert m0._guide(None, 1.0, 3) is None
    # the shared check: both denoisers reach the one method
    from shapegen_amd.networks import SimpleLatentUNetPointNet, UNetPointNetLarge
    assert SimpleLatentUNetPointNet.check_labels is UNetPointNetLarge.check_labels
    assert PointCloudDiffusion._guide is LatentDiffusion._guide
    lab = m.model.check_labels(None, 4)
    assert lab.dtype == torch.int32 and lab.tolist() == [3, 3, 3, 3]
    assert m.model.check_labels([2, 0, 3], 3).tolist() == [2, 0, 3]


def test_statement_against_itself_and_the_unconditional_oracle():
    sd = {k: v for k, v in latent_sd().items() if k.startswith("model.")}
    g = torch.Generator().manual_seed(5)
    E = torch.randn(4, 256, generator=g)
    z_T = torch.randn(3, 256, generator=g)
    inner = O.time_mlp
    with torch.no_grad():
        # all-null labels at scale 2 over a zero null row: the unguided oracle sampler (eu + 2 (eu - eu) = eu)
        E0 = E.clone()
        E0[3] = 0.0
        plain = O.ddim_sample(lambda z, t: O.latent_unet(sd, "model.", z, t), z_T, 4)
        got = S.sample("ddim", sd, "model.", E0, [3, 3, 3], 2.0, z_T, 4)
        assert rel_l2(got, plain) <= 1e-6
        # ... and over any null row: the null-class run at scale 1
        assert rel_l2(S.sample("ddim", sd, "model.", E, [3, 3, 3], 2.0, z_T, 4), S.sample("ddim", sd, "model.", E, [3, 3, 3], 1.0, z_T, 4)) <= 1e-6
        # scale 1 is the conditional-only run, exactly, for a number and for a vector of ones
        cond = O.ddim_sample(lambda z, t: S.eps_of(sd, "model.", E, [0, 2, 3], z, t), z_T, 4)
        assert torch.equal(S.sample("ddim", sd, "model.", E, [0, 2, 3], 1.0, z_T, 4), cond)
        assert torch.equal(S.sample("ddim", sd, "model.", E, [0, 2, 3], torch.ones(3), z_T, 4), cond)
        # a class changes its shape only (GroupNorm is per sample); a scale of 1 inside a vector leaves its shape conditional
        mixed = S.sample("ddim", sd, "model.", E, [0, 2, 3], torch.tensor([1.0, 2.0, 3.5]), z_T, 4)
        assert rel_l2(mixed[0], cond[0]) <= 1e-6 and rel_l2(mixed[1], cond[1]) > 1e-4
        assert rel_l2(mixed[2], cond[2]) <= 1e-6                                 # null label: eps_c = eps_u
        for kind, kw in (("dpm", {}), ("state", {"start_t": torch.ones(3) * 0.4}),
                         ("ddpm", {"noises": [torch.randn(3, 256, generator=g) for _ in range(4)]})):
            assert torch.isfinite(S.sample(kind, sd, "model.", E, [0, 2, 3], 2.0, z_T, 4, **kw)).all()
    assert O.time_mlp is inner
    # the training statement: the table's gradient exists, the row of a class without a shape is exactly zero
    z_t, t, nz = torch.randn(4, 256, generator=g), torch.rand(4, generator=g), torch.randn(4, 256, generator=g)
    mask = (torch.rand(4, 128, generator=g) >= 0.1).float()
    loss, pred, grads = S.training_step(sd, "model.", E, [1, 0, 1, 3], z_t, t, nz, mask)
    ge = grads["model.class_emb.weight"]
    assert ge.shape == (4, 256) and bool((ge[2] == 0).all()) and all(float(ge[r].abs().max()) > 0 for r in (0, 1, 3))
    assert torch.isfinite(loss) and pred.shape == (4, 256) and O.time_mlp is inner


def test_training_step_splits_the_batch_and_drops_labels_with_one_draw():
    m = _model(3, p_uncond=0.5)
    seen = []
    m.diffusion_loss = lambda z, t, labels=None: seen.append((z, t, labels)) or torch.zeros(())
    grids, labels = torch.rand(64, 1, 8, 8, 8), torch.arange(64) % 3
    torch.manual_seed(11)
    m.training_step((grids, labels))
    torch.manual_seed(11)
    t = torch.rand(64)
    dropped = torch.rand(64) < 0.5                                               # one draw, right after t's
    state = torch.get_rng_state()
    z, t_seen, lab = seen[-1]
    assert torch.equal(t_seen, t) and z.shape == (64, 256) and lab.dtype == torch.int32
    assert 8 < int(dropped.sum()) < 56 and torch.equal(lab == 3, dropped) and torch.equal(lab[~dropped].long(), labels[~dropped])
    torch.manual_seed(11)
    m.training_step([grids, labels])
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(seen[-1][2], lab)
    # validation: the labels as given, no draw beyond t's
    torch.manual_seed(11)
    m.validation_step((grids, labels))
    after = torch.get_rng_state()
    torch.manual_seed(11)
    torch.rand(64)
    assert torch.equal(seen[-1][2].long(), labels) and torch.equal(after, torch.get_rng_state())
    # a tensor batch of a class model: every label null; an unconditional model draws nothing for labels and refuses them
    m.training_step(grids)
    assert bool((seen[-1][2] == 3).all())
    m0 = _plain()
    seen0 = []
    m0.diffusion_loss = lambda z, t, labels=None: seen0.append(labels) or torch.zeros(())
    torch.manual_seed(11)
    m0.training_step(grids)
    after = torch.get_rng_state()
    torch.manual_seed(11)
    torch.rand(64)
    assert seen0 == [None] and torch.equal(after, torch.get_rng_state())
    with pytest.raises(ValueError, match="without classes"):
        m0.training_step((grids, labels))
    with pytest.raises(ValueError):
        m.training_step((grids, labels, labels))


def test_guided_entries_declared_bound_and_refuse_bad_arguments():
    from shapegen_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcd_hip.h")).read(), flags=re.S)
    _lib.build()
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib._SIGS and hasattr(lib, name), name
    assert "#define PCD_ABI_VERSION 2" in header and lib.pcd_abi_version() == _lib.ABI_VERSION == 2
    p = 256                                                      # never dereferenced: every case below is refused on the host
    ddim = lambda **kw: lib.pcd_latent_persist_ddim_guided(*[{**dict(
        h=p, z=p, x0=p, batch=8, tb=p, tb_elems=128, cb=p, rows=4, null=3, labels=p, w=p, ws=0, rates=p, rw=1, T=10, counter=p, n=10,
        ws_ptr=p, ws_bytes=1 << 20, st=0), **kw}[k] for k in ("h", "z", "x0", "batch", "tb", "tb_elems", "cb", "rows", "null", "labels",
                                                               "w", "ws", "rates", "rw", "T", "counter", "n", "ws_ptr", "ws_bytes", "st")])
    fwd = lambda **kw: lib.pcd_latent_persist_forward_guided(*[{**dict(
        h=p, z=p, batch=8, tb=p, cb=p, rows=4, null=3, labels=p, w=p, ws=0, eps=p, ws_ptr=p, ws_bytes=1 << 20, st=0), **kw}[k]
        for k in ("h", "z", "batch", "tb", "cb", "rows", "null", "labels", "w", "ws", "eps", "ws_ptr", "ws_bytes", "st")])
    for call in (ddim, fwd):
        assert call(batch=33) == -1                              # guided: at most 32 shapes (16 per stream)
        assert call(batch=65, w=0) == -1                         # labelled only: at most 64
        assert call(null=4) == -1 and call(null=-1) == -1 and call(rows=0) == -1
        assert call(ws=2) == -1 and call(ws=-1) == -1
        assert call(z=0) == -1 and call(labels=0) == -1 and call(cb=0) == -1 and call(h=0) == -1 and call(ws_ptr=0) == -1
        assert call(batch=0) == -1
    assert ddim(tb_elems=64) == -1 and ddim(tb_elems=256) == -1 and ddim(counter=0) == -1 and ddim(rates=0) == -1 and ddim(n=0) == -1
    assert ddim(rw=3) == -1
    assert fwd(eps=0) == -1 and fwd(tb=0) == -1
    assert b"bad argument" in lib.pcd_last_error()
