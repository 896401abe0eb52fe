"""Dev tool: steps/s of `PointCloudDiffusion.complete` next to `sample2` at the shape bench.py times (64 x 2048 on one
MI355X).  One step = one network evaluation: `complete` runs T = 40, jump = 10, resample = 3 (100 rows, 6 forward jumps,
half of every cloud known), `sample2` T = 100.  PASSES (default 3) alternating passes of each, warm-up call first;
B / N / PASSES / ONLY=sample2|complete in the environment."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import shapegen_amd  # noqa: F401
from shapegen_amd import specs
from shapegen_amd.diffusion import PointCloudDiffusion

B, N, PASSES = int(os.environ.get("B", 64)), int(os.environ.get("N", 2048)), int(os.environ.get("PASSES", 3))
ONLY = os.environ.get("ONLY", "")
torch.manual_seed(0)
model = PointCloudDiffusion(num_points=N)
sd = specs.synth_state_dict(specs.unet_pointnet_large_spec(prefix="model."), seed=0, gain=1.3)
model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
model = model.to("cuda").eval()
partial = torch.randn(B, N // 2, 3, device="cuda")
partial = partial / partial.norm(dim=2).max(dim=1).values[:, None, None]
T, JUMP, RESAMPLE = 40, 10, 3
rows = 100 if hasattr(model, "complete") else 0


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


legs = {"sample2": (lambda: model.sample2(B, N, num_steps=100), 100)}
if rows:
    from shapegen_amd.diffusion import completion_rows
    assert len(completion_rows(T, JUMP, RESAMPLE)) == rows
    legs["complete"] = (lambda: model.complete(partial, N, num_steps=T, resample=RESAMPLE, jump=JUMP), rows)
legs = {k: v for k, v in legs.items() if not ONLY or k == ONLY}
for fn, _ in legs.values():
    fn()                                                             # warm-up: kernels loaded, workspaces allocated
res = {k: [] for k in legs}
for _ in range(PASSES):
    for k, (fn, steps) in legs.items():
        res[k].append(timed(fn, steps))
for k, v in res.items():
    print(f"{k} B={B} N={N}: steps/s " + " / ".join(f"{x:.1f}" for x in v) + f"  median {sorted(v)[len(v) // 2]:.1f}"
          f"  spread {100 * (max(v) - min(v)) / min(v):.1f} %")
