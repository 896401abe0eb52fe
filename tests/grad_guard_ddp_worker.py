"""Worker for tests/test_gpu_grad_guard_fit.py: two ranks (both on cuda:0, gloo rendezvous on 127.0.0.1) take three
data-parallel training steps of the point denoiser on different batches with the gradient guard armed (clip norm from
GUARD_CLIP).  Every rank checks that it ends with rank 0's parameters and counters; rank 0 replays the three steps on
the mean of the gathered gradients with the float64 statement and saves [largest difference of the local gradients,
error against the statement, applied, skipped, clipped, the three norms]."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shapegen_amd  # noqa: E402,F401
import grad_guard_statement as S  # noqa: E402
from helpers import point_sd  # noqa: E402
from shapegen_amd.diffusion import PointCloudDiffusion  # noqa: E402
from shapegen_amd.training import PointTrainer  # noqa: E402

STEPS = 3


def batch(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 128, 3, generator=g) * 0.5, torch.rand(2, generator=g), torch.randn(2, 128, 3, generator=g)


def main():
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{os.environ['MASTER_PORT']}", rank=int(os.environ["RANK"]),
                            world_size=int(os.environ["WORLD_SIZE"]))
    rank, world = dist.get_rank(), dist.get_world_size()
    model = PointCloudDiffusion(num_points=128)
    model.load_state_dict(point_sd(), strict=True)
    model = model.to("cuda")
    tr = PointTrainer(model.model, lr=1e-3)
    clip = float(os.environ["GUARD_CLIP"])
    tr.set_gradient_guard(clip_norm=clip)
    p_start = tr.P.detach().cpu()
    local, norms = [], []
    for step in range(STEPS):
        x, t, n = batch(10 * step + rank)
        tr.forward(x.cuda(), t.cuda())
        tr.backward(n.cuda())
        local.append(tr.G.detach().cpu().clone())
        tr.optimizer_step()
        norms.append(tr.guard_stats()["last_norm"])
    stats = tr.guard_stats()
    flat = tr.P.detach().cpu()
    ref = flat.clone()
    dist.broadcast(ref, 0)
    assert torch.equal(flat, ref), "ranks diverged"
    mine = torch.tensor([stats["applied"], stats["skipped"], stats["clipped"]] + norms, dtype=torch.float64)
    theirs = mine.clone()
    dist.broadcast(theirs, 0)
    assert torch.equal(mine, theirs), f"ranks disagree on the guard: {mine.tolist()} / {theirs.tolist()}"
    gathered = []
    for g in local:
        parts = [torch.zeros_like(g) for _ in range(world)]
        dist.all_gather(parts, g)
        gathered.append(parts)
    if rank == 0:
        st = S.GuardedAdamW(p_start, lr=1e-3, betas=tr.betas, eps=tr.eps, weight_decay=tr.wd, max_norm=clip)
        for parts in gathered:
            st.step(sum(g.double() for g in parts) / world / tr.loss_scale)
        assert (st.applied, st.skipped, st.clipped) == (stats["applied"], stats["skipped"], stats["clipped"]), (st.norms, stats)
        np.save(os.environ["DDP_OUT"], np.array([float((gathered[0][0] - gathered[0][1]).abs().max()), float((flat.double() - st.p).abs().max()),
                                                 stats["applied"], stats["skipped"], stats["clipped"]] + norms))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
