"""Worker for tests/test_gpu_dpm.py::test_sample_sharded_as_a_forced_one_rank_world: ONE rank, backend "nccl" (= RCCL),
PCD_DIST_FORCE_COLLECTIVE=1, so `dist.sample_sharded(sampler="sample_dpm")` gathers its clouds through the collective like a
multi-GPU job would."""
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
    N, K = 128, 12
    model = PointCloudDiffusion(num_points=N)
    model.load_state_dict(point_sd(), strict=True)
    model = model.to("cuda").eval()
    torch.manual_seed(7)
    model._philox_offset = 0
    sharded = D.sample_sharded(model, 3, N, K, sampler="sample_dpm")
    torch.manual_seed(7)
    model._philox_offset = 0
    single = model.sample_dpm(3, N, num_steps=K)
    res["drawn_equal"] = bool(torch.equal(sharded, single))
    res["gathered_copy"] = bool(sharded.data_ptr() != single.data_ptr() and sharded.device == single.device)
    res["finite"] = bool(torch.isfinite(sharded).all())
    x_T = torch.randn(3, N, 3, generator=torch.Generator().manual_seed(31))
    a = D.sample_sharded(model, 3, N, K, x_T_global=x_T, sampler="sample_dpm")
    b = model.sample_dpm(3, N, num_steps=K, x_T=x_T.cuda())
    res["injected_equal"] = bool(torch.equal(a, b))
    dist.barrier()
    dist.destroy_process_group()
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
