"""The gradient guard through the trainers, `fit`, two ranks and the entry script (kernels: tests/test_gpu_grad_guard.py)."""
import glob
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_guard_statement as S  # noqa: E402
import resume_runs as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"

# Clip norms for the accumulated runs and the two-rank run, picked between the gradient norms measured on one MI355X
# (docstrings of the tests that use them).
ACCUM = {"point": (3, 4, 21.0), "latent": (2, 2, 0.9)}          # kind: (k, micro-batches per epoch, clip norm)
DDP_CLIP = 23.0


def ulps(a, b) -> int:
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ---------------------------------------------------------------------------------------------- 7. armed and idle
@pytest.mark.parametrize("kind", R.KINDS)
def test_armed_and_idle_run_is_the_plain_run(kind):
    """`fit(gradient_clip_val=1e30)` - norm kernel and guarded AdamW on every step, never clipping - ends bitwise where the
    plain run ends, with the same lr history."""
    ma, ha, na = R.run(kind)
    sa = R.snapshot(ma)
    assert ma._trainer.guard_state is None and ma._trainer.A is None          # unarmed: nothing new was allocated
    del ma
    mb, hb, nb = R.run(kind, gradient_clip_val=1e30)
    stats = mb._trainer.guard_stats()
    assert R.compare(sa, R.snapshot(mb)) == {}
    assert [h[3] for h in ha] == [h[3] for h in hb] and na == nb
    assert stats["applied"] == mb._trainer.step_count == len(nb) and stats["skipped"] == stats["clipped"] == 0
    assert np.isfinite(stats["last_norm"]) and stats["last_norm"] > 0


# ---------------------------------------------------------------------------------------------- 8. trainer level
@pytest.mark.parametrize("kind", ["point", "latent"])
def test_trainer_clip_and_skip_against_the_statement(kind):
    """Four training steps with the clip norm at a quarter of the first step's gradient norm (the first step is clipped
    for certain, the later ones as their norms decide - the statement takes the same decisions), then a step on a gradient
    buffer the test has written a NaN into, then one more.  The guard's norm is within 2 ulp of the float64 norm of
    `trainer.grads()`; the flat parameters follow the statement applied to the trainer's own `grads()` to 2e-6 (the
    optimizer alone, as test_adamw_update_and_loss_decreases isolates it); the poisoned step changes nothing and AdamW's
    step stays the applied count.  The statement without clipping is held to be more than 2e-5 away: the first step's
    moments are built from a gradient four times smaller, which moves the later updates (1e-4 each) by tens of percent."""
    model, data = R.make(kind)
    tr = model.configure_optimizers()["optimizer"]
    model.train()
    batches = list(data.train_dataloader()) * 3

    def flat_grads():
        g = tr.grads()
        return torch.cat([g[k].reshape(-1) for k in tr.names]).cpu()

    model.training_step(batches[0], 0)
    g0 = flat_grads()
    clip = 0.25 * S.grad_norm(g0)
    tr.set_gradient_guard(clip_norm=clip)
    hyper = dict(lr=tr.lr, betas=tr.betas, eps=tr.eps, weight_decay=tr.wd)
    st, free = S.GuardedAdamW(tr.P.cpu(), max_norm=clip, **hyper), S.GuardedAdamW(tr.P.cpu(), **hyper)
    for i in range(4):
        if i:
            model.training_step(batches[i], i)
        g = flat_grads()
        tr.optimizer_step()
        st.step(g); free.step(g)
        got = tr.guard_stats()["last_norm"]
        print(f"{kind} step {i + 1}: norm {got!r} host {st.norms[-1]!r} ulps {ulps(got, st.norms[-1])}")
        assert ulps(got, st.norms[-1]) <= 2
    err, away = float((tr.P.cpu().double() - st.p).abs().max()), float((tr.P.cpu().double() - free.p).abs().max())
    print(f"{kind}: clipped {st.clipped} of 4, against the statement {err:.3e}, against the unclipped statement {away:.3e}")
    stats = tr.guard_stats()
    assert (stats["applied"], stats["clipped"], stats["skipped"]) == (4, st.clipped, 0) and st.clipped >= 1
    assert err <= 2e-6 and away > 2e-5
    # a poisoned gradient buffer: nothing moves, the step is counted as skipped
    model.training_step(batches[4], 4)
    tr.G[tr.G.numel() // 2] = float("nan")
    before = [t.clone() for t in (tr.P, tr.M1, tr.M2)]
    tr.optimizer_step()
    stats = tr.guard_stats()
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.P, tr.M1, tr.M2)))
    assert (stats["applied"], stats["skipped"], tr.step_count) == (4, 1, 5) and not np.isfinite(stats["last_norm"])
    model.training_step(batches[5], 5)
    g = flat_grads()
    tr.optimizer_step()
    st.step(g)
    assert st.t == 5 and tr.guard_stats()["applied"] == 5 and tr.step_count == 6
    assert float((tr.P.cpu().double() - st.p).abs().max()) <= 2e-6
    assert tr.state_dict()["guard"]["applied"] == 5 and tr.state_dict()["step"] == 6


# ---------------------------------------------------------------------------------------------- 9. accumulation + resume
@pytest.mark.parametrize("kind", list(ACCUM))
def test_accumulated_clipped_run_resumes_exactly(kind, tmp_path):
    """`accumulate_grad_batches` = 3 on the point run (4 micro-batches per epoch: one full step and one flush of a single
    micro-batch per epoch) and 2 on the latent run (one step per epoch), with a clip norm between the norms of the run,
    so that some steps are clipped and some are not (asserted).  Straight through against stopped by `max_steps` after
    epoch 2 and resumed from `-last.ckpt`: bitwise equal state, equal counters and norms, `global_step` in optimizer steps.

    Norms of the eight / four optimizer steps with the guard armed and idle (clip 1e30), one MI355X:
        point, k = 3   28.14 16.81 25.44 16.56 26.54 17.96 25.62 14.22   (full step, flush, ...): clip norm 21 lies in the gap
        latent, k = 2  1.182 0.952 0.860 0.700: clip norm 0.9"""
    from shapegen_amd.checkpoint import read_checkpoint
    k, micro, clip = ACCUM[kind]
    per_epoch = -(-micro // k)
    kw = dict(accumulate_grad_batches=k, gradient_clip_val=clip)
    ma, ha, na = R.run(kind, **kw)
    sa, stats_a = R.snapshot(ma), ma._trainer.guard_stats()
    print(f"{kind}: straight run {stats_a}")
    assert len(na) == R.EPOCHS * micro and ma._trainer.step_count == R.EPOCHS * per_epoch == stats_a["applied"]
    assert 0 < stats_a["clipped"] < stats_a["applied"] and stats_a["skipped"] == 0
    assert [n[1] for n in na[:micro + 1]] == [0] * min(k, micro) + [1] * (micro - min(k, micro)) + [per_epoch]    # step count moves every k
    del ma
    m1, h1, n1 = R.run(kind, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True, max_steps=2 * per_epoch, **kw)
    assert len(h1) == 2 and n1 == na[:2 * micro]
    del m1
    last = str(tmp_path / "run-last.ckpt")
    ck = read_checkpoint(last)
    assert ck["epoch"] == 1 and ck["global_step"] == 2 * per_epoch
    saved = ck["shapegen_amd"]["trainer"]
    assert saved["accumulate"] == k and saved["guard"]["clip_norm"] == clip and saved["guard"]["applied"] == 2 * per_epoch
    assert all(float(s["step"]) == 2 * per_epoch for s in ck["optimizer_states"][0]["state"].values())
    mc, hc, nc = R.run(kind, ckpt_path=last, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True)     # settings come from the file
    stats_c = mc._trainer.guard_stats()
    assert mc._trainer.accum == k and mc._trainer.clip_norm == clip
    assert nc == na[2 * micro:] and [h[3] for h in hc] == [h[3] for h in ha]
    assert R.compare(sa, R.snapshot(mc)) == {}
    assert stats_c == stats_a
    assert read_checkpoint(last)["global_step"] == R.EPOCHS * per_epoch


# ---------------------------------------------------------------------------------------------- 10. two ranks
def test_two_ranks_agree_on_clipping(tmp_path):
    """Three data-parallel steps (tests/grad_guard_ddp_worker.py) with a clip norm between the norms of the mean
    gradients (25.89, 20.80, 24.34 measured with the guard idle on one MI355X; clip norm 23): the norm is taken after the all-reduce, so both ranks clip the same steps
    with no further collective - equal parameters and counters (the worker asserts them) - and rank 0 matches the statement
    on the mean gradients to the 5e-6 of test_two_rank_training_steps_stay_in_sync."""
    out = str(tmp_path / "ddp.npy")
    with socket.socket() as sock:                      # a free rendezvous port
        sock.bind(("127.0.0.1", 0))
        port = str(sock.getsockname()[1])
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, DDP_OUT=out,
                   PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", GUARD_CLIP=repr(DDP_CLIP))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "grad_guard_ddp_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-1500:] for l in logs)
    diff, err, applied, skipped, clipped, *norms = np.load(out)
    print(f"two ranks: norms {norms}, clipped {clipped}, against the statement {err:.3e}")
    assert diff > 0                               # the two ranks really had different gradients before the exchange
    assert (applied, skipped) == (3, 0) and 0 < clipped < 3
    assert err < 5e-6


# ---------------------------------------------------------------------------------------------- 11. the entry script
def test_train_point_ddpm_with_the_guard_flags(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "train_point_ddpm.py"), "--num-points", "256", "--batch-size", "8", "--synthetic-shapes", "40",
           "--epochs", "2", "--grad-clip", "1.0", "--accumulate-grad-batches", "2", "--skip-nonfinite", "--sample-steps", "5",
           "--out", str(tmp_path / "p"), "--data-dir", str(tmp_path / "none")]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    logs = glob.glob(str(tmp_path / "train" / "logs" / "*.log"))
    assert len(logs) == 1
    log = open(logs[0]).read()
    for epoch in (0, 1):
        line = next(l for l in log.splitlines() if f"epoch {epoch}: train_loss" in l)
        assert "grad_norm" in line and "clipped" in line and "skipped 0" in line, line


# ---------------------------------------------------------------------------------------------- accumulation at trainer level
@pytest.mark.parametrize("kind", ["point", "latent"])
def test_accumulated_step_is_the_step_on_the_mean_gradient(kind):
    """k = 3: three micro-batches, then the optimizer step; then a flush with a single micro-batch, which keeps k.  The
    buffer the step sees is the fp32 sum (g1 + g2) + g3 of the trainer's own `grads()` (they are G / loss_scale, a power
    of two, so the unscaled sum is the same fp32 sum), and the gradient is that sum / k: the guard's norm is within
    2 ulp of its float64 norm (a wrong scale - a lost k, G in place of A, a stale A in the second step - is a factor, not
    ulps), and the parameters follow the statement on it to 2e-6, with the clip norm at half the first norm so that the
    scale of the gradient matters to the update."""
    k = 3
    model, data = R.make(kind)
    tr = model.configure_optimizers()["optimizer"]
    model.train()
    batches = list(data.train_dataloader()) * 2
    tr.set_accumulation(k)
    hyper = dict(lr=tr.lr, betas=tr.betas, eps=tr.eps, weight_decay=tr.wd)

    def flat_grads():
        g = tr.grads()
        return torch.cat([g[n].reshape(-1) for n in tr.names])

    total, p0 = None, tr.P.cpu()
    for i in range(k):
        model.training_step(batches[i], i)
        g = flat_grads()
        total = g if total is None else total + g             # fp32, on the device, in the kernel's order
        if i < k - 1:
            assert tr.micro_step() is False and tr.step_count == 0 and torch.equal(tr.P.cpu(), p0)
    mean = total.cpu().double() / k
    clip = 0.5 * S.grad_norm(mean)
    tr.set_gradient_guard(clip_norm=clip)
    st = S.GuardedAdamW(p0, max_norm=clip, **hyper)
    assert tr.micro_step() is True and tr.step_count == 1
    st.step(mean)
    got = tr.guard_stats()["last_norm"]
    print(f"{kind} full step: norm {got!r} host {st.norms[-1]!r} ulps {ulps(got, st.norms[-1])}")
    assert ulps(got, st.norms[-1]) <= 2 and st.clipped == 1
    assert float((tr.P.cpu().double() - st.p).abs().max()) <= 2e-6
    # the flush: one micro-batch, still divided by k; A starts again from this gradient
    model.training_step(batches[k], k)
    g4 = flat_grads().cpu().double() / k
    assert tr.micro_step() is False and tr.flush() is True and tr.flush() is False and tr.step_count == 2
    st.step(g4)
    got = tr.guard_stats()["last_norm"]
    print(f"{kind} flush: norm {got!r} host {st.norms[-1]!r} ulps {ulps(got, st.norms[-1])}")
    assert ulps(got, st.norms[-1]) <= 2
    err = float((tr.P.cpu().double() - st.p).abs().max())
    stats = tr.guard_stats()
    print(f"{kind}: against the statement {err:.3e}, {stats}")
    assert err <= 2e-6 and (stats["applied"], stats["clipped"], stats["skipped"]) == (2, st.clipped, 0)


# ---------------------------------------------------------------------------------------------- arming on resume
def test_unarmed_checkpoint_resumed_with_the_guard(tmp_path):
    """A run without the guard, stopped after two epochs, is resumed with `gradient_clip_val` (the case the guard is for:
    a run that went bad is continued under protection).  The file has no guard keys, so the caller's setting holds and
    every step of the file counts as applied: the counters, `global_step` and the torch-layout optimizer `step` of the
    checkpoints written afterwards are those of the whole run, and with a clip norm that is never reached the run ends
    bitwise where the uninterrupted plain run ends.  The same through the trainer alone: arm, then `load_state_dict`."""
    from shapegen_amd.checkpoint import read_checkpoint
    ma, ha, na = R.run("point")
    sa = R.snapshot(ma)
    del ma
    m1, h1, n1 = R.run("point", ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True, max_steps=8)
    last = str(tmp_path / "run-last.ckpt")
    ck = read_checkpoint(last)
    assert ck["global_step"] == 8 and "guard" not in ck["shapegen_amd"]["trainer"]
    other, _ = R.make("point")
    fresh = other.configure_optimizers()["optimizer"]
    fresh.set_gradient_guard(skip_nonfinite=True)
    fresh.load_state_dict(m1._trainer.state_dict())
    assert fresh.step_count == 8 and fresh.guard and fresh.guard_stats()["applied"] == 8
    del m1, other, fresh
    mc, hc, nc = R.run("point", ckpt_path=last, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True, gradient_clip_val=1e30)
    tr = mc._trainer
    stats = tr.guard_stats()
    assert tr.guard and tr.clip_norm == 1e30 and tr.step_count == 16
    assert (stats["applied"], stats["skipped"], stats["clipped"]) == (16, 0, 0)
    assert nc == na[8:] and R.compare(sa, R.snapshot(mc)) == {}
    ck = read_checkpoint(last)
    assert ck["global_step"] == 16 and ck["shapegen_amd"]["trainer"]["guard"]["applied"] == 16
    assert all(float(s["step"]) == 16 for s in ck["optimizer_states"][0]["state"].values())
