"""Worker for tests/test_gpu_completion.py::test_complete_sharded_as_a_forced_one_rank_world: ONE rank, backend "nccl" (= RCCL),
PCD_DIST_FORCE_COLLECTIVE=1, so `dist.complete_sharded` gathers its clouds through the collective like a multi-GPU job would."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shapegen_amd  # noqa: E402,F401
from helpers import point_sd  # noqa: E402
from shapegen_amd import dist as D  # noqa: E402
from shapegen_amd.diffusion import PointCloudDiffusion  # noqa: E402


def main():
    import torch.distributed as dist
    torch.set_grad_enabled(False)
    assert D.force_collective()
    D.init_from_env("nccl")
    res = {"backend": dist.get_backend(), "world": dist.get_world_size()}
    N, T = 128, 12
    model = PointCloudDiffusion(num_points=N)
    model.load_state_dict(point_sd(), strict=True)
    model = model.to("cuda").eval()
    g = torch.Generator().manual_seed(31)
    partial = torch.randn(3, N, 3, generator=g)
    partial = partial / partial.norm(dim=2).max(dim=1).values[:, None, None]
    counts = torch.tensor([0, 37, 128])
    torch.manual_seed(7)
    model._philox_offset = 0
    sharded = D.complete_sharded(model, partial, counts, N, T, resample=2, jump=4)
    torch.manual_seed(7)
    model._philox_offset = 0
    single = model.complete(partial.cuda(), N, num_steps=T, known_counts=counts, resample=2, jump=4)
    res["drawn_equal"] = bool(torch.equal(sharded, single))
    res["gathered_copy"] = bool(sharded.data_ptr() != single.data_ptr() and sharded.device == single.device)
    x_T = torch.randn(3, N, 3, generator=g)
    torch.manual_seed(9)
    model._philox_offset = 0
    a = D.complete_sharded(model, partial, counts, N, 4, x_T_global=x_T)
    torch.manual_seed(9)
    model._philox_offset = 0
    b = model.complete(partial.cuda(), N, num_steps=4, known_counts=counts, x_T=x_T.cuda())
    res["injected_equal"] = bool(torch.equal(a, b))
    res["known_rows_equal"] = all(bool(torch.equal(sharded[i, :c].cpu(), partial[i, :c])) for i, c in enumerate(counts.tolist()))
    dist.barrier()
    dist.destroy_process_group()
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
