"""Small training runs of the four trainers through `training.fit`, shared by tests/test_gpu_resume.py: the same
run can be made in one go or interrupted and resumed, and leaves everything needed to compare the two.  The straight
run with the EMA off uses nothing newer than `fit(model, data_module, max_epochs, log=...)`, so the run-to-run
differences the test's bounds come from can be measured on any revision (`python tests/resume_runs.py`)."""
import os
import random
import sys

import numpy as np
import torch

KINDS = ("point", "attention", "latent", "vae")
EPOCHS = 4
DEV = "cuda"


def _eager_plateau(cls):
    """The model class with its plateau scheduler made to act within four epochs: every epoch that does not improve
    val_loss tenfold halves the lr, so a resumed run that lost the scheduler's state or the lr shows at once."""

    class Eager(cls):
        def configure_optimizers(self):
            cfg = super().configure_optimizers()
            s = cfg["lr_scheduler"]["scheduler"]
            s.patience, s.threshold = 0, 0.9
            return cfg

    Eager.__name__ = cls.__name__
    return Eager


class Batches:
    """`train` batches in an order drawn from the global torch generator per epoch (what DataLoader(shuffle=True) does),
    one validation batch."""

    def __init__(self, x: torch.Tensor, batch: int, train: int):
        self.x, self.batch, self.train = x, batch, train

    def setup(self):
        pass

    def train_dataloader(self):
        return (self.x[i * self.batch:(i + 1) * self.batch] for i in torch.randperm(self.train).tolist())

    def val_dataloader(self):
        return iter([self.x[self.train * self.batch:(self.train + 1) * self.batch]])


def _voxels(count: int, g: torch.Generator) -> torch.Tensor:
    zz, yy, xx = torch.meshgrid(*[torch.arange(32.0)] * 3, indexing="ij")
    v = torch.zeros(count, 1, 32, 32, 32)
    for i in range(count):
        c, r = torch.rand(3, generator=g) * 16 + 8, torch.rand(3, generator=g) * 6 + 3
        v[i, 0] = (((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1).float()
    return v


def make(kind: str):
    """(model on the GPU, data module) of a run, from fixed seeds: the same call gives the same start."""
    from shapegen_amd.diffusion import LatentDiffusion, PointCloudDiffusion
    from shapegen_amd.vae import VAE3DLarge
    torch.manual_seed(7)
    random.seed(7)
    np.random.seed(7)
    g = torch.Generator().manual_seed(11)
    if kind in ("point", "attention"):                       # B * N = 4 * 256: a multiple of 64, and N of 64 for the attention
        model = _eager_plateau(PointCloudDiffusion)(num_points=256, backbone="pointnet" if kind == "point" else "attention")
        data = Batches(torch.rand(20, 256, 3, generator=g) * 2 - 1, 4, 4)
    elif kind == "latent":
        model = LatentDiffusion(VAE3DLarge())
        data = Batches(_voxels(12, g), 4, 2)
    else:
        model = _eager_plateau(VAE3DLarge)()
        data = Batches(_voxels(12, g), 4, 2)
    return model.to(DEV), data


def record_steps(model) -> list:
    """Make every training_step note (lr, optimizer step count, current_epoch, KL weight) as it starts."""
    notes = []
    inner = model.training_step

    def training_step(batch, i=0):
        tr = model._trainer
        notes.append((tr.lr, tr.step_count, getattr(model, "current_epoch", None),
                      model.get_kl_weight() if hasattr(model, "get_kl_weight") else None))
        return inner(batch, i)

    model.training_step = training_step
    return notes


def snapshot(model) -> dict:
    """Parameters and buffers, both AdamW moments and the EMA buffer (if kept), on the host."""
    tr = model._trainer
    out = {"sd." + k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    out["exp_avg"], out["exp_avg_sq"] = tr.M1.cpu().clone(), tr.M2.cpu().clone()
    if getattr(tr, "EMA", None) is not None:
        out["ema"] = tr.EMA.cpu().clone()
    return out


def run(kind: str, **fit_kw):
    """One run of `EPOCHS` epochs (or as far as `max_steps` in fit_kw lets it go); returns (model, history, notes)."""
    from shapegen_amd.training import fit
    model, data = make(kind)
    notes = record_steps(model)
    history = fit(model, data, max_epochs=EPOCHS, log=lambda *_: None, **fit_kw)
    return model, history, notes


def loss_spread(ha, hb) -> float:
    """Largest relative difference of a train or validation loss between two histories of the same run."""
    worst = 0.0
    for a, b in zip(ha, hb):
        for x, y in zip(a[1:3], b[1:3]):
            worst = max(worst, abs(x - y) / max(abs(x), abs(y), 1e-30))
    return worst


def compare(sa: dict, sb: dict) -> dict:
    """Per tensor that differs: the largest absolute difference (an empty dict = bitwise equal)."""
    assert list(sa) == list(sb)
    return {k: float((sa[k].double() - sb[k].double()).abs().max()) for k in sa if not torch.equal(sa[k], sb[k])}


if __name__ == "__main__":                                   # measure: the straight run RUNS times per trainer, EMA off, all pairs
    sys.path.insert(0, os.getcwd())
    import shapegen_amd  # noqa: F401
    runs = int(os.environ.get("RUNS", 2))
    for kind in (sys.argv[1:] or KINDS):
        done = []
        for _ in range(runs):
            model, history, _ = run(kind)
            done.append((snapshot(model), history))
            del model
        pairs = [(a, b) for i, a in enumerate(done) for b in done[i + 1:]]
        diff = {}
        for (sa, _), (sb, _) in pairs:
            for k, v in compare(sa, sb).items():
                diff[k] = max(diff.get(k, 0.0), v)
        spread = max(loss_spread(ha, hb) for (_, ha), (_, hb) in pairs)
        print(f"{kind}: {runs} straight runs, all pairs: {len(diff)} tensors differ (worst {max(diff.values(), default=0.0):.3e}), "
              f"lr equal {all([h[3] for h in ha] == [h[3] for h in hb] for (_, ha), (_, hb) in pairs)}, loss spread {spread:.3e}, "
              f"val_loss {[round(h[2], 4) for h in done[0][1]]}", flush=True)
        for k, v in sorted(diff.items(), key=lambda kv: -kv[1])[:4]:
            print(f"    {k}: {v:.3e}", flush=True)
