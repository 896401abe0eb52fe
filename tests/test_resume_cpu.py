"""Resuming a run from a checkpoint, the parts that need no GPU: the fused AdamW + EMA entry point's argument checks,
scheduler state, the conversion between the flat AdamW moments and torch.optim.AdamW's state dict, `training.fit` with
`ckpt_path` / `save_last` on a toy module (one process and two gloo ranks), and the checkpoint layout."""
import os
import random
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---------------------------------------------------------------------------------------------- 1. the C entry point
def test_adamw_ema_step_is_exported_and_checks_its_arguments():
    from shapegen_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "pcd_adamw_ema_step") and "pcd_adamw_ema_step" in _lib._SIGS
    ok = dict(p=64, g=64, m1=64, m2=64, ema=64, n=8, step=1, scale=1.0, decay=0.9)         # pointers are never dereferenced on the host

    def call(**kw):
        a = {**ok, **kw}
        return lib.pcd_adamw_ema_step(a["p"], a["g"], a["m1"], a["m2"], a["ema"], a["n"], 1e-3, 0.9, 0.999, 1e-8, 1e-2, a["step"], a["scale"],
                                      a["decay"], None)

    for bad in (dict(p=None), dict(g=None), dict(m1=None), dict(m2=None), dict(ema=None), dict(n=0), dict(step=0), dict(scale=0.0),
                dict(decay=1.0), dict(decay=-0.1)):
        assert call(**bad) == -1, bad
        assert b"bad argument" in lib.pcd_last_error(), bad


# ---------------------------------------------------------------------------------------------- 2. scheduler state
class _Lr:
    def __init__(self, lr):
        self.lr = lr


def _interrupted_equals_straight(make, metrics):
    tr = _Lr(1e-3)
    s = make(tr)
    straight = []
    for m in metrics:
        s.step(m)
        straight.append(tr.lr)
    for cut in range(len(metrics) + 1):
        tr = _Lr(1e-3)
        s = make(tr)
        got = []
        for m in metrics[:cut]:
            s.step(m)
            got.append(tr.lr)
        state = s.state_dict()
        tr2 = _Lr(1e-3)                       # fresh objects: the lr of the interrupted run comes from the state
        s2 = make(tr2)
        s2.load_state_dict({**state, "some_key_of_a_newer_torch": 1})
        for m in metrics[cut:]:
            s2.step(m)
            got.append(tr2.lr)
        assert got == straight, cut
    return straight


def test_scheduler_state_resumes_at_every_position():
    from shapegen_amd.training import CosineAnnealingLR, ReduceLROnPlateau
    metrics = [1.0, 0.9, 0.95, 0.93, 0.94, 0.5, 0.6, 0.7, 0.65, 0.55, 0.51]
    lrs = _interrupted_equals_straight(lambda tr: ReduceLROnPlateau(tr, factor=0.5, patience=2), metrics)
    assert lrs[-1] == 1e-3 * 0.25 and lrs[0] == 1e-3                                       # cut twice
    st = ReduceLROnPlateau(_Lr(1.0)).state_dict()
    assert {"best", "num_bad_epochs", "factor", "patience", "threshold"} <= set(st)
    lrs = _interrupted_equals_straight(lambda tr: CosineAnnealingLR(tr, T_max=5, eta_min=1e-6), [None] * 8)    # over its T_max
    assert abs(lrs[4] - 1e-6) < 1e-12 and lrs[5] > lrs[4]
    st = CosineAnnealingLR(_Lr(1.0), T_max=5).state_dict()
    assert {"last_epoch", "base_lrs", "T_max", "eta_min"} <= set(st)
    # torch's own objects carry these names
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=1e-3)
    assert {"last_epoch", "base_lrs", "T_max", "eta_min"} <= set(torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=5).state_dict())
    assert {"best", "num_bad_epochs", "factor", "patience", "threshold"} <= set(torch.optim.lr_scheduler.ReduceLROnPlateau(opt).state_dict())


# ---------------------------------------------------------------------------------------------- 3. optimizer-state conversion
def test_flat_moments_convert_to_torch_adamw_and_back():
    from oracle import torch_oracle as O
    from shapegen_amd.training import adamw_state_from_torch, adamw_state_to_torch
    g = torch.Generator().manual_seed(3)
    shapes = {"a.weight": (4, 3), "frozen.weight": (5,), "a.bias": (4,), "b.weight": (2, 2, 1)}
    order = list(shapes)
    layout = [(k, shapes[k]) for k in order if k != "frozen.weight"]
    n = sum(int(np.prod(s)) for _, s in layout)
    m1, m2 = torch.randn(n, generator=g) * 1e-2, torch.rand(n, generator=g) * 1e-4
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    state = adamw_state_to_torch(m1, m2, 7, layout, order, **hyper)
    assert sorted(state["state"]) == [0, 2, 3] and state["param_groups"][0]["params"] == [0, 1, 2, 3]
    # a plain round trip is exact (checked first: torch's load_state_dict keeps the tensors it is given and steps them in place)
    r1, r2, rstep, _ = adamw_state_from_torch(state, layout, order)
    assert torch.equal(r1, m1) and torch.equal(r2, m2) and rstep == 7
    with pytest.raises(RuntimeError):
        adamw_state_from_torch(state, layout, order[:-1])
    # a real torch.optim.AdamW over parameters of these shapes takes it ...
    params = {k: torch.nn.Parameter(torch.randn(*s, generator=g), requires_grad=k != "frozen.weight") for k, s in shapes.items()}
    opt = torch.optim.AdamW(list(params.values()), lr=0.5, weight_decay=0.0)
    opt.load_state_dict(state)
    assert opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["weight_decay"] == 1e-2
    # ... and one more torch step from there is the oracle's step continued from the same moments
    grads = {k: torch.randn(*s, generator=g) for k, s in layout}
    want = {k: params[k].detach().clone() for k, _ in layout}
    ostate, off = {"step": 7, "m": {}, "v": {}}, 0
    for k, s in layout:
        c = int(np.prod(s))
        ostate["m"][k], ostate["v"][k] = m1[off:off + c].view(s).clone(), m2[off:off + c].view(s).clone()
        off += c
    O.adamw_step(want, grads, ostate, **hyper)
    for k, _ in layout:
        params[k].grad = grads[k].clone()
    frozen_before = params["frozen.weight"].detach().clone()
    opt.step()
    for k, _ in layout:
        assert (params[k].detach() - want[k]).abs().max() <= 2e-6, k          # the bound tests/test_train_oracle_cpu.py holds adamw_step to
    assert torch.equal(params["frozen.weight"].detach(), frozen_before) and 1 not in opt.state_dict()["state"]
    # the reverse direction: torch's state after that step, flat again, is the oracle's
    b1, b2, step, group = adamw_state_from_torch(opt.state_dict(), layout, order)
    assert step == 8 and group["lr"] == 1e-3
    assert (b1 - torch.cat([ostate["m"][k].reshape(-1) for k, _ in layout])).abs().max() <= 2e-6
    assert (b2 - torch.cat([ostate["v"][k].reshape(-1) for k, _ in layout])).abs().max() <= 2e-6


# ---------------------------------------------------------------------------------------------- 4. fit() on a toy module
class _ToyOpt:
    """An optimizer with state: the step size and a step count travel in its state dict."""

    def __init__(self, model):
        self.model, self.lr, self.count = model, 0.5, 0

    def step(self):
        g = self.model.pending.clone()
        if dist.is_initialized():
            dist.all_reduce(g)
            g /= dist.get_world_size()
        with torch.no_grad():
            self.model.w += self.lr * g
        self.count += 1

    def state_dict(self):
        return {"lr": self.lr, "count": self.count}

    def load_state_dict(self, st):
        self.lr, self.count = st["lr"], st["count"]


class _Toy(torch.nn.Module):
    """Stands in for a HIP-trained module in `training.fit`: its steps draw from every random stream fit() restores and
    record what they drew."""

    def __init__(self):
        super().__init__()
        from shapegen_amd.training import ReduceLROnPlateau
        self.w = torch.nn.Parameter(torch.zeros(3))
        self.register_buffer("seen", torch.zeros(1))
        self.hparams = {"width": 3}
        self.current_epoch = -1
        self.drawn, self.epochs = [], []
        self._philox_offset = 0
        self._opt = _ToyOpt(self)
        self._sched = ReduceLROnPlateau(self._opt, factor=0.5, patience=0)

    @property
    def device(self):
        return torch.device("cpu")

    def configure_optimizers(self):
        return {"optimizer": self._opt, "lr_scheduler": {"scheduler": self._sched, "monitor": "val_loss"}}

    def training_step(self, batch, i):
        r = torch.rand(3)
        self.drawn.append((i, float(batch.sum()), r.clone(), random.random(), float(np.random.rand())))
        self.epochs.append(self.current_epoch)
        self.pending = r * batch.float().mean()
        self.seen += 1
        self._philox_offset += 4
        return (self.w.detach() * r).sum() + batch.float().mean()

    def validation_step(self, batch, i):
        return torch.rand(()) + 0.01 * self.w.detach().sum()


class _ShuffledData:
    """Batches in an order drawn from the global torch generator, as a DataLoader(shuffle=True) does."""

    def __init__(self, n):
        self.n = n

    def setup(self):
        pass

    def train_dataloader(self):
        return [torch.full((2, 2), float(i)) for i in torch.randperm(self.n).tolist()]

    def val_dataloader(self):
        return [torch.zeros(2, 2)]


def _seed(s=11):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _same_draws(a, b):
    return len(a) == len(b) and all(x[:2] == y[:2] and torch.equal(x[2], y[2]) and x[3:] == y[3:] for x, y in zip(a, b))


def _straight_and_resumed(tmp, data=lambda: _ShuffledData(4), resume_torch_seed=999):
    """6 epochs in one go against 3 epochs, fresh objects, 3 more; returns the two models, histories and directories."""
    from shapegen_amd.training import fit
    quiet = lambda *_: None
    kw = dict(log=quiet, save_top_k=2, ckpt_name="toy", save_last=True)
    da, db = os.path.join(tmp, "a"), os.path.join(tmp, "b")
    _seed()
    ma = _Toy()
    ha = fit(ma, data(), max_epochs=6, ckpt_dir=da, **kw)
    _seed()
    mb = _Toy()
    hb1 = fit(mb, data(), max_epochs=3, ckpt_dir=db, **kw)
    _seed(999)                               # whatever the resuming process did with its generators before fit()
    torch.manual_seed(resume_torch_seed)
    mc = _Toy()
    hc = fit(mc, data(), max_epochs=6, ckpt_dir=db, ckpt_path=os.path.join(db, "toy-last.ckpt"), **kw)
    assert hb1 == ha[:3] and hc == ha and ha[0][1] == ha[0][1]                 # the restored history continues (and no loss is NaN)
    assert _same_draws(ma.drawn, mb.drawn + mc.drawn)
    assert mc.epochs == ma.epochs[len(mb.epochs):] and mc.epochs[0] == 3 and mc.current_epoch == 5
    assert torch.equal(ma.w, mc.w) and torch.equal(ma.seen, mc.seen)
    assert ma._opt.lr == mc._opt.lr and ma._opt.count == mc._opt.count and ma._philox_offset == mc._philox_offset
    assert ma._sched.state_dict() == mc._sched.state_dict()
    return ma, mc, da, db


def test_fit_resumes_exactly(tmp_path):
    from shapegen_amd.checkpoint import read_checkpoint
    from shapegen_amd.training import CKPT_KEY, fit
    ma, mc, da, db = _straight_and_resumed(str(tmp_path))
    assert ma._opt.lr < 0.5                                                     # the plateau scheduler did cut: its state mattered
    assert sorted(os.listdir(da)) == sorted(os.listdir(db)) and len(os.listdir(da)) == 3      # top 2 + last, no temporary file left
    la, lb = (read_checkpoint(os.path.join(d, "toy-last.ckpt")) for d in (da, db))
    assert la[CKPT_KEY]["kept"] == lb[CKPT_KEY]["kept"] and len(la[CKPT_KEY]["kept"]) == 2
    assert la["epoch"] == lb["epoch"] == 5 and la["global_step"] == lb["global_step"] == 24
    assert la["optimizer_states"] == lb["optimizer_states"] and la["lr_schedulers"] == lb["lr_schedulers"]
    # a file without the private key (as Lightning writes it) still resumes epoch, step, weights, optimizer and scheduler
    mid = read_checkpoint(os.path.join(db, sorted(f for f in os.listdir(db) if "epoch" in f)[0]))
    mid.pop(CKPT_KEY)
    torch.save(mid, tmp_path / "foreign.ckpt")
    said = []
    m = _Toy()
    assert fit(m, _ShuffledData(4), max_epochs=mid["epoch"] + 1, ckpt_path=str(tmp_path / "foreign.ckpt"), log=said.append) == []
    assert torch.equal(m.w.detach(), mid["state_dict"]["w"]) and m._opt.count == mid["optimizer_states"][0]["count"]
    assert m._sched.state_dict() == mid["lr_schedulers"][0]
    assert any("RNG" in s and "not" in s for s in said)
    m = _Toy()
    hist = fit(m, _ShuffledData(4), max_epochs=mid["epoch"] + 2, ckpt_path=str(tmp_path / "foreign.ckpt"), log=lambda *_: None)
    assert [h[0] for h in hist] == [mid["epoch"] + 1] and m.epochs == [mid["epoch"] + 1] * 4


class _SplitData:
    """A data module that draws its train / validation split in setup(), like the project's own (`random_split`)."""

    def __init__(self, n=20):
        self.n = n

    def setup(self):
        ds = torch.utils.data.TensorDataset(torch.arange(self.n, dtype=torch.float32).view(self.n, 1).expand(self.n, 4).clone())
        self.train_dataset, self.val_dataset = torch.utils.data.random_split(ds, [16, self.n - 16])

    def train_dataloader(self):
        return (b[0] for b in torch.utils.data.DataLoader(self.train_dataset, batch_size=4, shuffle=True))

    def val_dataloader(self):
        return (b[0] for b in torch.utils.data.DataLoader(self.val_dataset, batch_size=4))


def test_resume_keeps_the_split_or_refuses(tmp_path):
    from shapegen_amd.training import fit, split_fingerprint
    quiet = lambda *_: None
    torch.manual_seed(5)
    d1 = _SplitData()
    fit(_Toy(), d1, max_epochs=2, ckpt_dir=str(tmp_path), ckpt_name="toy", save_last=True, log=quiet)
    last = str(tmp_path / "toy-last.ckpt")
    torch.manual_seed(5)                                                         # seeded as before: the same split, and the run goes on
    d2 = _SplitData()
    hist = fit(_Toy(), d2, max_epochs=3, ckpt_path=last, log=quiet)
    assert list(d2.train_dataset.indices) == list(d1.train_dataset.indices) and [h[0] for h in hist] == [0, 1, 2]
    assert split_fingerprint(d1) == split_fingerprint(d2) is not None and split_fingerprint(_ShuffledData(4)) is None
    torch.manual_seed(6)                                                         # seeded differently: validation shapes would be trained on
    with pytest.raises(RuntimeError, match="split"):
        fit(_Toy(), _SplitData(), max_epochs=3, ckpt_path=last, log=quiet)
    # the straight / resumed comparison holds with this data module too
    _straight_and_resumed(str(tmp_path / "cmp"), data=_SplitData, resume_torch_seed=11)    # torch seeded as the first run: same split


def _resume_worker(rank, world, port, tmp):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import shapegen_amd  # noqa: F401
    from shapegen_amd import dist as D
    from shapegen_amd.checkpoint import read_checkpoint
    from shapegen_amd.training import CKPT_KEY
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    D.init_from_env("gloo")
    ma, mc, da, db = _straight_and_resumed(tmp)              # per rank: own draws, own batches
    dist.barrier()
    assert sorted(os.listdir(da)) == sorted(os.listdir(db))
    last = read_checkpoint(os.path.join(db, "toy-last.ckpt"))
    assert len(last[CKPT_KEY]["rank_rng"]) == 2 and last[CKPT_KEY]["world"] == 2
    both = [None, None]
    dist.all_gather_object(both, [d[2] for d in ma.drawn])
    assert not torch.equal(both[0][0], both[1][0])           # the ranks do draw from different streams
    # rank 0 writes, so only rank 0 has to name a directory: the other rank still takes part in the gather and nothing hangs
    from shapegen_amd.training import fit
    solo = os.path.join(tmp, "solo")
    fit(_Toy(), _ShuffledData(4), max_epochs=1, log=lambda *_: None, ckpt_name="solo", ckpt_dir=solo if rank == 0 else None,
        save_last=rank == 0)
    dist.barrier()
    assert sorted(os.listdir(solo)) == ["solo-epoch=00-val_loss=%.2f.ckpt" % read_checkpoint(os.path.join(solo, "solo-last.ckpt"))[CKPT_KEY]["kept"][0][0],
                                        "solo-last.ckpt"]
    dist.barrier()
    dist.destroy_process_group()
    open(os.path.join(tmp, f"resume_ok{rank}"), "w").write("ok")


def test_two_rank_fit_resumes_exactly(tmp_path):
    mp.spawn(_resume_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "resume_ok0").exists() and (tmp_path / "resume_ok1").exists()


# ---------------------------------------------------------------------------------------------- 5. layout
def test_new_checkpoint_reads_back_through_the_lightning_reader(tmp_path):
    from shapegen_amd.checkpoint import load_lightning_checkpoint, read_checkpoint
    from shapegen_amd.diffusion import PointCloudDiffusion
    from shapegen_amd.training import CKPT_KEY, save_checkpoint
    m = PointCloudDiffusion(num_points=32)
    plain, full = str(tmp_path / "plain.ckpt"), str(tmp_path / "full.ckpt")
    save_checkpoint(m, plain, 3)                                                 # what fit() wrote before: no training state
    toy = _Toy()
    save_checkpoint(m, full, 3, optimizer=toy._opt, scheduler=toy._sched, loop={"kept": [], "steps": 12, "history": [], "max_epochs": 9})
    hp0, sd0 = load_lightning_checkpoint(plain)
    hp1, sd1 = load_lightning_checkpoint(full)
    assert list(hp1) == list(hp0) == list(m.hparams) and hp1 == hp0              # nothing new in hyper_parameters
    assert list(sd1) == list(sd0) and all(torch.equal(sd1[k], sd0[k]) for k in sd0)
    a, b = read_checkpoint(plain), read_checkpoint(full)
    assert set(a) <= set(b) and set(b) - set(a) == {"global_step", "optimizer_states", "lr_schedulers", CKPT_KEY}
    assert b[CKPT_KEY]["format"] == 1 and b["global_step"] == 12 and b[CKPT_KEY]["max_epochs"] == 9
    back = PointCloudDiffusion.load_from_checkpoint(full)
    assert all(torch.equal(v, sd0[k]) for k, v in back.state_dict().items())
    with pytest.raises(RuntimeError, match="ema_state_dict"):
        PointCloudDiffusion.load_from_checkpoint(full, weights="ema")            # this run kept no average
    ck = read_checkpoint(full)
    ck["ema_state_dict"] = {k: v + 1 if v.is_floating_point() else v for k, v in ck["state_dict"].items()}
    torch.save(ck, full)
    ema = PointCloudDiffusion.load_from_checkpoint(full, weights="ema")
    k = "model.enc1.conv1.weight"
    assert torch.equal(ema.state_dict()[k], sd0[k] + 1)
    assert not [f for f in os.listdir(tmp_path) if ".tmp." in f]                 # written under a temporary name, then renamed
