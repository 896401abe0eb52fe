"""Dev tool: what classifier-free guidance costs per step at the shape bench.py times (64 x 2048 on one MI355X), written to
profiles/cfg_bench.json (OUT in the environment overrides the path).

Three legs, 100-step `sample2` calls, PASSES (default 3) alternating passes after a warm-up call, with the spread of the passes:
 - `unguided`: a model without classes (the call every earlier revision makes);
 - `scale_1`: a class model with labels and guidance_scale 1 (select with labels, one forward);
 - `scale_2`: the same with guidance_scale 2 (two forwards and the combine).
Expected: scale_1 costs an unguided step, scale_2 two forwards plus a few microseconds.  On a tree without class conditioning only
`unguided` is timed, which is how the parent commit is measured in the same session; PARENT_JSON names that run's file, and its
figures are copied under "parent" so that the unguided step can be held against the parent's own pass-to-pass spread.  Run each
invocation under its own time limit."""
import inspect
import json
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
STEPS, CLASSES = int(os.environ.get("STEPS", 100)), 4
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cfg_bench.json"))
torch.manual_seed(0)
torch.set_grad_enabled(False)
as_torch = lambda sd: {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
has_cfg = "num_classes" in inspect.signature(PointCloudDiffusion.__init__).parameters


def build(classes):
    spec = specs.unet_pointnet_large_spec(prefix="model.")
    if classes:
        spec = spec + [("model.class_emb.weight", (classes + 1, 256), "w")]
    model = PointCloudDiffusion(num_points=N, **({"num_classes": classes} if classes else {}))
    model.load_state_dict(as_torch(specs.synth_state_dict(spec, seed=0, gain=1.3)), strict=True)
    return model.to("cuda").eval()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return {"runs": [round(x, 3) for x in v], "median": round(sorted(v)[len(v) // 2], 3),
            "spread_pct": round(100 * (max(v) - min(v)) / min(v), 2)}


plain = build(0)
legs = {"unguided": lambda: plain.sample2(B, N, num_steps=STEPS)}
if has_cfg:
    cond = build(CLASSES)
    labels = torch.arange(B) % CLASSES
    legs["scale_1"] = lambda: cond.sample2(B, N, num_steps=STEPS, labels=labels, guidance_scale=1.0)
    legs["scale_2"] = lambda: cond.sample2(B, N, num_steps=STEPS, labels=labels, guidance_scale=2.0)
for fn in legs.values():
    fn()                                                             # warm-up: kernels loaded, workspaces allocated
ms = {k: [] for k in legs}
for _ in range(PASSES):
    for k, fn in legs.items():
        ms[k].append(1e3 * wall(fn) / STEPS)
res = {"shape": [B, N], "passes": PASSES, "steps_per_call": STEPS, "device": torch.cuda.get_device_name(0), "class_conditioning": has_cfg,
       "ms_per_step": {k: stats(v) for k, v in ms.items()}}
if has_cfg:
    u, s1, s2 = (res["ms_per_step"][k]["median"] for k in ("unguided", "scale_1", "scale_2"))
    res["scale_1_over_unguided"] = round(s1 / u, 4)
    res["scale_2_minus_two_unguided_us"] = round(1e3 * (s2 - 2 * u), 1)
parent = os.environ.get("PARENT_JSON")
if parent and os.path.isfile(parent):
    with open(parent) as f:
        res["parent"] = json.load(f)["ms_per_step"]
    res["unguided_over_parent"] = round(res["ms_per_step"]["unguided"]["median"] / res["parent"]["unguided"]["median"], 4)
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
