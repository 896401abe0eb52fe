"""Dev tool: `sample_dpm` next to `sample` at the shape bench.py times (64 x 2048 on one MI355X), written to
profiles/sample_dpm_bench.json (OUT in the environment overrides the path).

 - steps/s of the "dpm" step kind and of `sample`'s, 100 steps per call, PASSES (default 3) alternating passes after a warm-up
   call, with the spread of the passes;
 - whole-call wall time of `sample_dpm(B, N, 20)` (table build, graph capture and all), with graphs and eager, next to
   20 x the per-step time, and the same at 12 and 40 steps;
 - `sample(B, N, 1000)` next to it;
 - the latent calls `LatentDiffusion.sample_dpm(B, 20)` and `sample(B, 1000)` (LATENT=0 skips them).
On a tree without `sample_dpm` only `sample` is timed, which is how the parent commit is measured in the same session."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import shapegen_amd  # noqa: F401
from shapegen_amd import specs
from shapegen_amd.diffusion import LatentDiffusion, PointCloudDiffusion

B, N, PASSES = int(os.environ.get("B", 64)), int(os.environ.get("N", 2048)), int(os.environ.get("PASSES", 3))
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sample_dpm_bench.json"))
torch.manual_seed(0)
torch.set_grad_enabled(False)
as_torch = lambda sd: {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
model = PointCloudDiffusion(num_points=N)
model.load_state_dict(as_torch(specs.synth_state_dict(specs.unet_pointnet_large_spec(prefix="model."), seed=0, gain=1.3)), strict=True)
model = model.to("cuda").eval()
has_dpm = hasattr(model, "sample_dpm")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return {"runs": [round(x, 4) for x in v], "median": round(sorted(v)[len(v) // 2], 4),
            "spread_pct": round(100 * (max(v) - min(v)) / min(v), 2)}


res = {"shape": [B, N], "passes": PASSES, "device": torch.cuda.get_device_name(0)}
legs = {"sample": lambda: model.sample(B, N, num_steps=100)}
if has_dpm:
    legs["sample_dpm"] = lambda: model.sample_dpm(B, N, num_steps=100)
for fn in legs.values():
    fn()                                                             # warm-up: kernels loaded, workspaces allocated
rate = {k: [] for k in legs}
for _ in range(PASSES):
    for k, fn in legs.items():
        rate[k].append(100 / wall(fn))
res["steps_per_s_100_step_calls"] = {k: stats(v) for k, v in rate.items()}
if has_dpm:
    per_step = 1.0 / res["steps_per_s_100_step_calls"]["sample_dpm"]["median"]
    calls = {}
    for steps in (12, 20, 40):
        row = {}
        for graphs in (True, False):
            model.use_graphs = graphs
            model.sample_dpm(B, N, num_steps=steps)
            row["graphs" if graphs else "eager"] = stats([wall(lambda: model.sample_dpm(B, N, num_steps=steps)) for _ in range(5)])
        del model.use_graphs
        row["steps_times_per_step_s"] = round(steps * per_step, 4)
        calls[str(steps)] = row
    res["sample_dpm_whole_call_s"] = calls
res["sample_1000_whole_call_s"] = stats([wall(lambda: model.sample(B, N, num_steps=1000)) for _ in range(2)])
if has_dpm:
    res["speedup_sample_1000_over_sample_dpm_20"] = round(res["sample_1000_whole_call_s"]["median"]
                                                          / res["sample_dpm_whole_call_s"]["20"]["graphs"]["median"], 1)
if os.environ.get("LATENT", "1") != "0":
    from shapegen_amd.vae import VAE3DLarge
    ldm = LatentDiffusion(VAE3DLarge())
    sd = specs.synth_state_dict(specs.latent_unet_spec(prefix="model."), seed=0, gain=1.3)
    sd.update(specs.synth_state_dict(specs.vae3d_large_spec(prefix="vae."), seed=0, gain=1.3))
    ldm.load_state_dict(as_torch(sd), strict=True)
    ldm = ldm.to("cuda").eval()
    lat = {"sample_1000": lambda: ldm.sample(B, num_steps=1000)}
    if has_dpm:
        lat["sample_dpm_20"] = lambda: ldm.sample_dpm(B, num_steps=20)
    for fn in lat.values():
        fn()
    res["latent_whole_call_s"] = {k: stats([wall(fn) for _ in range(3)]) for k, fn in lat.items()}
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
