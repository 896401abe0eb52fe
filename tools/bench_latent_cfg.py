"""Dev tool: step time of the class-conditional latent sampler, written to profiles/latent_cfg_bench.json (OUT in the
environment overrides the path).  One process, one session: 1000-step DDIM latent loops at B = 32 (the VAE decode is not
timed), the routes alternating for ROUNDS (default 20) rounds after a warm-up round, median and range per step for

 - guided, persistent launch (two paired streams of 16 shapes);
 - guided, per-layer launches (two forwards, select, combine and update per step);
 - labelled only (scale 1), persistent launch;
 - unguided persistent launch at B = 32 and at B = 64 (the unlabelled `LatentDiffusion`: today's code, and the launch with as
   many tile rows as the guided B = 32 one);

and `sample_dpm(32, 20)` guided with `output="mesh"`, whole call.  On a tree without `ConditionalLatentDiffusion` only the
unguided legs are timed, which is how the parent commit is measured in the same session: run this file there first with OUT
set, then here with PARENT naming that file, and its `ddim_step` figures are written into this run's output under
`parent_commit_same_session`."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import shapegen_amd  # noqa: F401
from shapegen_amd import diffusion, specs
from shapegen_amd.vae import VAE3DLarge

B, STEPS, ROUNDS, K = int(os.environ.get("B", 32)), int(os.environ.get("STEPS", 1000)), int(os.environ.get("ROUNDS", 20)), 3
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "latent_cfg_bench.json"))
torch.manual_seed(0)
torch.set_grad_enabled(False)
has_cfg = hasattr(diffusion, "ConditionalLatentDiffusion")


def build(cls, *a):
    m = cls(VAE3DLarge(), *a)
    sd = specs.synth_state_dict(specs.latent_unet_spec(prefix="model."), seed=0, gain=1.3)
    sd.update(specs.synth_state_dict(specs.vae3d_large_spec(prefix="vae."), seed=0, gain=1.3))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    if a:
        sd["model.class_emb.weight"] = torch.randn(a[0] + 1, 256, generator=torch.Generator().manual_seed(31))
    m.load_state_dict(sd, strict=True)
    return m.to("cuda").eval()


def loop(m, b, persistent, **cond):
    """One latent DDIM loop of STEPS steps from a fixed start; returns seconds (the status read waits for the launch)."""
    z = z_T[:b].clone()
    guide = {"guide": m._guide(cond.get("labels"), cond.get("guidance_scale", 1.0), b)} if cond else {}
    tab = m.ddim_table(STEPS, b)
    m.use_persistent = persistent
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m._run_table(z, tab, "ddim", **guide)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if persistent and not m.use_persistent:
        raise SystemExit("the persistent launch was abandoned: this process does not have the whole GPU")
    return dt


def stats(v):
    us = sorted(1e6 * x / STEPS for x in v)
    return {"median_us_per_step": round(us[len(us) // 2], 2), "min_us_per_step": round(us[0], 2), "max_us_per_step": round(us[-1], 2),
            "rounds": len(us)}


z_T = torch.randn(64, 256, generator=torch.Generator().manual_seed(1)).to("cuda")
plain = build(diffusion.LatentDiffusion)
legs = {"unguided_persistent_b32": lambda: loop(plain, B, True), "unguided_persistent_b64": lambda: loop(plain, 2 * B, True)}
if has_cfg:
    cond = build(diffusion.ConditionalLatentDiffusion, K)
    labels = torch.arange(B) % (K + 1)
    legs["guided_persistent"] = lambda: loop(cond, B, True, labels=labels, guidance_scale=2.0)
    legs["guided_per_layer"] = lambda: loop(cond, B, False, labels=labels, guidance_scale=2.0)
    legs["labelled_persistent"] = lambda: loop(cond, B, True, labels=labels)
if not plain.model.persist_supported(B):
    raise SystemExit("needs a device the persistent launch runs on (256 CUs)")
res = {"shape": [B, 256], "steps": STEPS, "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "class_conditional_tree": has_cfg}
for fn in legs.values():
    fn()                                                                 # warm-up: kernels loaded, handles and graphs' workspaces made
times = {k: [] for k in legs}
for _ in range(ROUNDS):
    for k, fn in legs.items():
        times[k].append(fn())
res["ddim_step"] = {k: stats(v) for k, v in times.items()}
if has_cfg:
    g, p = res["ddim_step"]["guided_persistent"], res["ddim_step"]["guided_per_layer"]
    res["guided_persistent_clear_of_per_layer"] = bool(g["max_us_per_step"] < p["min_us_per_step"])
    cond.use_persistent = True

    def dpm_mesh():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cond.sample_dpm(B, num_steps=20, labels=labels, guidance_scale=2.0, output="mesh")
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    dpm_mesh()
    v = sorted(dpm_mesh() for _ in range(5))
    res["sample_dpm_20_guided_mesh_whole_call_ms"] = {"median": round(1e3 * v[2], 2), "min": round(1e3 * v[0], 2), "max": round(1e3 * v[-1], 2)}
if os.environ.get("PARENT"):
    with open(os.environ["PARENT"]) as f:
        res["parent_commit_same_session"] = json.load(f)["ddim_step"]
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
