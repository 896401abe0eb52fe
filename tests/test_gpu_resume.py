"""Resuming a run on the GPU: the fused AdamW + EMA launch against the plain one, an interrupted and resumed run of each
of the four trainers against the uninterrupted one, sampling from the averaged weights, and the entry script."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resume_runs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---------------------------------------------------------------------------------------------- the launch
def _adamw(lib, L, p, m1, m2, g, step, ema=None, decay=0.0):
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-2, step, 1024.0)
    if ema is None:
        L.check(lib.pcd_adamw_step(p.data_ptr(), g.data_ptr(), m1.data_ptr(), m2.data_ptr(), p.numel(), *hyper, L.stream_ptr()), "adamw")
    else:
        L.check(lib.pcd_adamw_ema_step(p.data_ptr(), g.data_ptr(), m1.data_ptr(), m2.data_ptr(), ema.data_ptr(), p.numel(), *hyper, decay,
                                       L.stream_ptr()), "adamw_ema")


@pytest.mark.parametrize("n", [1000, 1_000_003])
def test_adamw_ema_step_against_adamw_step(n):
    """Three chained steps.  Parameters and moments of the EMA launch are bitwise those of the plain launch; with decay
    0.5 the average is bitwise torch's 0.5 * ema + 0.5 * p (both products exact: one rounding, whatever the compiler
    contracts); with decay 0.999 it stays within 3 k 2^-24 max(|p|, |ema|) per element of the float64 recurrence over the
    same parameter snapshots after k steps (at most three roundings per element and step); max(|p|, |ema|) is taken as the
    running maximum over the steps so far and the start value, not the current step's alone: a rounding made at an earlier
    step scales with that step's magnitudes, and an element near zero now need not have been.  The one-element-per-lane form
    the library takes for buffers that are not 16-byte aligned gives the same bits as the four-per-lane form.  Both moments
    of the plain launch are bitwise what they have always been: two rounded products and a rounded sum each, formed here by
    torch's elementwise fp32 operations (a fused multiply-add in the kernel would differ in the last bit)."""
    from shapegen_amd import _lib as L
    L.require_gpu()
    lib = L.load()
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g).to(DEV)
    e0 = (torch.randn(n, generator=g) * 0.5).to(DEV)
    grads = [(torch.randn(n, generator=g) * 1024 * 10 ** (k - 1)).to(DEV) for k in range(3)]
    z = lambda: torch.zeros(n, device=DEV)

    def shifted(t):                          # the same values 4 bytes past a 16-byte boundary
        buf = torch.empty(n + 1, device=DEV)
        assert buf.data_ptr() % 16 == 0
        buf[1:].copy_(t)
        return buf[1:]

    plain = (p0.clone(), z(), z())
    half = (p0.clone(), z(), z(), e0.clone())
    slow = (p0.clone(), z(), z(), e0.clone())
    odd = tuple(shifted(t) for t in (p0, z(), z(), e0))
    assert all(t.data_ptr() % 16 == 0 for t in plain + half + slow) and all(t.data_ptr() % 16 == 4 for t in odd)
    d = float(np.float32(0.999))                               # the decay the launch receives
    e64, mag = e0.double(), e0.abs().double()
    f32 = lambda v: float(np.float32(v))
    c1, c2 = f32(np.float32(1) - np.float32(0.9)), f32(np.float32(1) - np.float32(0.999))     # 1.f - beta as the kernel forms it
    for k, gr in enumerate(grads, start=1):
        before = half[3].clone()
        g_unscaled = gr * (1.0 / 1024.0)
        want_m1 = f32(0.9) * plain[1] + c1 * g_unscaled
        want_m2 = f32(0.999) * plain[2] + (c2 * g_unscaled) * g_unscaled
        _adamw(lib, L, *plain, step=k, g=gr)
        assert torch.equal(plain[1], want_m1) and torch.equal(plain[2], want_m2), k
        _adamw(lib, L, *half[:3], step=k, g=gr, ema=half[3], decay=0.5)
        _adamw(lib, L, *slow[:3], step=k, g=gr, ema=slow[3], decay=0.999)
        _adamw(lib, L, *odd[:3], step=k, g=shifted(gr), ema=odd[3], decay=0.999)
        for a, b, c, o in zip(plain, half, slow, odd):
            assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, o)
        assert not torch.equal(plain[0], p0) and torch.isfinite(plain[0]).all()
        assert torch.equal(half[3], 0.5 * before + 0.5 * half[0])
        assert torch.equal(odd[3], slow[3])
        e64 = d * e64 + (1.0 - d) * slow[0].double()
        mag = torch.maximum(mag, torch.maximum(slow[0].abs().double(), slow[3].abs().double()))
        err = (slow[3].double() - e64).abs()
        assert bool((err <= 3 * k * 2.0 ** -24 * mag).all()), (k, float((err / mag.clamp_min(1e-30)).max()) / 2.0 ** -24)


# ---------------------------------------------------------------------------------------------- the four trainers
# Largest relative difference of a train / validation loss between two straight runs (tests/resume_runs.py, EMA off) on
# the revision before this feature, per trainer; see the docstring below.
# The point trainer's own figure there, 2.573e-2, is the amplified non-repeatability of `pcd_vec3_outer`'s atomics (docstring),
# not the loss sum's; its loss is the same L1 kernel over the same 4 x 256 x 3 elements as the attention trainer's, so it takes
# that trainer's figure instead of a 5 % box.
LOSS_SPREAD_BEFORE = {"point": 1.938e-7, "attention": 1.938e-7, "latent": 1.277e-7, "vae": 4.974e-7}


@pytest.mark.parametrize("kind", R.KINDS)
def test_resumed_run_is_the_uninterrupted_run(kind, tmp_path):
    """Four epochs in one go (twice) against two epochs, `save_last`, fresh module / trainer / data module, `ckpt_path`,
    two more; the EMA on in all of them.  The first leg of the interrupted run is the same `fit(max_epochs=4)` call
    stopped by `max_steps` after its second epoch, as a killed run would be (the cosine schedule's T_max is the planned
    length).  The plateau scheduler is made eager (tests/resume_runs.py) so that the lr moves within the four epochs.

    Expected and asserted: the two straight runs agree bitwise in parameters, buffers, both moments and the EMA buffer,
    and so does the resumed run; lr and the per-step notes (lr, step count, current_epoch, KL weight) agree exactly, the
    first resumed step carrying epoch 2's values, not epoch 0's.  Loss values are sums of atomics and differ in their last
    bits from run to run: each is held to twice LOSS_SPREAD_BEFORE, the spread two straight runs showed on the revision
    before this feature (six straight runs with `RUNS=6 python tests/resume_runs.py`, all fifteen pairs, on one MI355X
    box; figures below).

    Six straight runs, EMA off, largest difference over all pairs:
        trainer     before this feature                              with it
        point       152 state tensors differ, loss spread 2.573e-2   bitwise equal, loss spread 1.974e-7
        attention   3 differ (<= 6e-8), loss spread 1.938e-7         bitwise equal, loss spread 1.821e-7
        latent      bitwise equal, loss spread 1.277e-7              bitwise equal, loss spread 6.463e-8
        vae         bitwise equal, loss spread 4.974e-7              bitwise equal, loss spread 5.480e-7
    Before, the point and attention trainers were not repeatable: `pcd_vec3_outer` added its per-block partials
    atomically, and at this small shape the point run amplifies the last-bit differences to percents within four epochs
    (which is why its loss box is the attention trainer's and not twice 2.573e-2).  The feature's change set gives that
    kernel an ordered sum, so the
    bitwise comparison the issue expects holds for all four and no per-tensor allowance is needed."""
    from shapegen_amd.checkpoint import read_checkpoint
    steps_per_epoch = 4 if kind in ("point", "attention") else 2
    ma, ha, na = R.run(kind, ema_decay=0.9)
    mb, hb, nb = R.run(kind, ema_decay=0.9)
    sa, sb = R.snapshot(ma), R.snapshot(mb)
    assert "ema" in sa and not torch.equal(sa["ema"], ma._trainer.P.cpu())
    print(f"{kind}: straight twice: differing tensors {R.compare(sa, sb)}, loss spread {R.loss_spread(ha, hb):.3e}")
    assert R.compare(sa, sb) == {} and na == nb and [h[3] for h in ha] == [h[3] for h in hb]
    del mb
    m1, h1, n1 = R.run(kind, ema_decay=0.9, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True, max_steps=2 * steps_per_epoch)
    assert len(h1) == 2 and n1 == na[:2 * steps_per_epoch]
    del m1
    last = str(tmp_path / "run-last.ckpt")
    ck = read_checkpoint(last)
    assert ck["epoch"] == 1 and ck["global_step"] == 2 * steps_per_epoch and "ema_state_dict" in ck
    mc, hc, nc = R.run(kind, ckpt_path=last, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True)
    sc = R.snapshot(mc)
    print(f"{kind}: resumed: differing tensors {R.compare(sa, sc)}, loss spread {R.loss_spread(ha, hc):.3e}")
    # what goes wrong without the training state: the first resumed step would note epoch 0's lr, step 0, the KL warm-up's start
    assert nc == na[2 * steps_per_epoch:] and nc[0] != na[0] and nc[0][1] == 2 * steps_per_epoch
    if kind == "vae":
        assert nc[0][2] == 2 and nc[0][3] == na[2 * steps_per_epoch][3] != na[0][3]
    assert nc[0][0] != na[0][0]                                # (the eager plateau / the cosine schedule has moved the lr by epoch 2)
    assert [h[0] for h in hc] == [0, 1, 2, 3] and [h[3] for h in hc] == [h[3] for h in ha]
    assert R.compare(sa, sc) == {}
    bound = 2 * LOSS_SPREAD_BEFORE[kind]
    assert R.loss_spread(ha, hb) <= bound and R.loss_spread(ha, hc) <= bound, (R.loss_spread(ha, hb), R.loss_spread(ha, hc), bound)
    # the optimizer state in the file is torch.optim.AdamW's: indexed like the module's parameters(), frozen ones without state
    opt_state = ck["optimizer_states"][0]
    params = list(mc.parameters())
    assert opt_state["param_groups"][0]["params"] == list(range(len(params)))
    assert sorted(opt_state["state"]) == [i for i, p in enumerate(params) if p.requires_grad]
    assert all(tuple(opt_state["state"][i]["exp_avg"].shape) == tuple(params[i].shape) for i in opt_state["state"])
    if kind == "latent":
        assert len(opt_state["state"]) < len(params)


# ---------------------------------------------------------------------------------------------- sampling from the average
def test_ema_weights_swap_in_and_out(tmp_path):
    from shapegen_amd.diffusion import PointCloudDiffusion
    model, h, _ = R.run("point", ema_decay=0.9, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True, max_steps=4)
    tr = model._trainer
    x_T = torch.randn(2, 256, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    raw = model.sample(2, 256, num_steps=4, x_T=x_T).clone()
    with tr.ema_weights():
        inside = model.sample(2, 256, num_steps=4, x_T=x_T).clone()
    assert torch.equal(model.sample(2, 256, num_steps=4, x_T=x_T), raw) and not torch.equal(inside, raw)
    last = str(tmp_path / "run-last.ckpt")
    second = PointCloudDiffusion.load_from_checkpoint(last, weights="ema").to(DEV)
    assert torch.equal(second.sample(2, 256, num_steps=4, x_T=x_T), inside)
    third = PointCloudDiffusion.load_from_checkpoint(last).to(DEV)
    assert torch.equal(third.sample(2, 256, num_steps=4, x_T=x_T), raw)
    ema_sd = tr.ema_state_dict()
    assert list(ema_sd) == list(model.model.state_dict())
    assert all(torch.equal(v.cpu(), second.state_dict()["model." + k].cpu()) for k, v in ema_sd.items())
    with pytest.raises(ZeroDivisionError):
        with tr.ema_weights():
            1 / 0
    assert torch.equal(model.sample(2, 256, num_steps=4, x_T=x_T), raw)          # an exception inside still restores
    # the trainer's own state dict round-trips into a fresh trainer, and a different layout is refused
    other, _ = R.make("point")
    fresh = other.configure_optimizers()["optimizer"]
    other.load_state_dict(model.state_dict())
    fresh.load_state_dict(tr.state_dict())
    assert fresh.step_count == tr.step_count == 4 and fresh.lr == tr.lr and fresh.ema_decay == 0.9
    assert torch.equal(fresh.M1, tr.M1) and torch.equal(fresh.M2, tr.M2) and torch.equal(fresh.EMA, tr.EMA)
    bad = dict(tr.state_dict())
    bad["layout"] = bad["layout"][1:]
    with pytest.raises(RuntimeError, match="layout"):
        fresh.load_state_dict(bad)


# ---------------------------------------------------------------------------------------------- the entry script
def test_train_point_ddpm_resume(tmp_path):
    """`--epochs 2 --save-last --ema-decay 0.99`, then `--resume` of the last file with `--epochs 3`: exactly one more
    epoch, logged as epoch 2, checkpoints into the directory of the file resumed from."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = [sys.executable, os.path.join(ROOT, "train_point_ddpm.py"), "--num-points", "256", "--batch-size", "8", "--synthetic-shapes", "40",
              "--sample-steps", "5", "--out", str(tmp_path / "p"), "--data-dir", str(tmp_path / "none"), "--save-last", "--ema-decay", "0.99"]
    r = subprocess.run(common + ["--epochs", "2"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = glob.glob(str(tmp_path / "checkpoints" / "point_ddpm" / "*" / "point_cloud_diffusion-last.ckpt"))
    assert len(last) == 1
    run_dir = os.path.dirname(last[0])
    assert len(os.listdir(run_dir)) == 3
    logs_before = set(glob.glob(str(tmp_path / "train" / "logs" / "*.log")))
    r = subprocess.run(common + ["--epochs", "3", "--resume", last[0]], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    new_logs = set(glob.glob(str(tmp_path / "train" / "logs" / "*.log"))) - logs_before
    assert len(new_logs) == 1
    log = open(new_logs.pop()).read()
    assert "epoch 2: train_loss" in log and "epoch 0: train_loss" not in log and "epoch 1: train_loss" not in log and "epoch 3:" not in log
    assert "continuing at epoch 2, step 8" in log
    assert sorted(os.listdir(run_dir))[:3] == sorted(f for f in os.listdir(run_dir) if "epoch=" in f) and len(os.listdir(run_dir)) == 4
    assert glob.glob(str(tmp_path / "checkpoints" / "point_ddpm" / "*")) == [run_dir]
    from shapegen_amd.checkpoint import read_checkpoint
    from shapegen_amd.diffusion import PointCloudDiffusion
    ck = read_checkpoint(last[0])
    assert ck["epoch"] == 2 and ck["global_step"] == 12 and ck["shapegen_amd"]["trainer"]["ema_decay"] == 0.99
    m = PointCloudDiffusion.load_from_checkpoint(last[0], weights="ema")
    assert int(m.state_dict()["model.enc1.bn1.num_batches_tracked"]) == 12       # 3 epochs x 4 batches of 8
