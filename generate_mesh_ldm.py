"""Generation entry point of the latent route with surfaces out: sample latents, decode them to 32^3 occupancy grids and write one
triangle mesh per shape.

    python generate_mesh_ldm.py [--vae-ckpt FILE] [--ldm-ckpt FILE] [--num-samples 16] [--sampler ddim|dpm] [--steps N]
                                [--threshold 0.4] [--format obj|ply] [--out DIR] [--png-dir DIR]
                                [--smooth N] [--keep-largest] [--normals]
                                [--simplify-resolution R | --simplify-cell H | --target-faces N] [--placement quadric|mean] [--deduplicate]
                                [--label K --guidance W [--num-classes K]]

`--sampler dpm` (default, 20 steps) is `LatentDiffusion.sample_dpm`, `ddim` (default 1000 steps) is `sample`; both run with
`output="mesh"`, so the decoded grids go through the surface-nets kernel (`utils.voxel_tensor_to_meshes`) at `--threshold`, the
predicate of the point conversion.  The latent-diffusion checkpoint carries the VAE's weights too (`vae.*` keys); `--vae-ckpt` alone gives
a trained VAE under a denoiser with synthetic weights.  Without checkpoints (none ship with the reference) both run on deterministic
synthetic weights, so the plumbing is exercised end to end.  One file `mesh_<i>.<format>` per shape goes to `--out`; vertices are in
the [-1, 1] cube of the point clouds (a surface that reaches the grid's border closes up to one voxel pitch outside it).  Per shape
the log gives the vertex and triangle counts and whether the mesh is closed.  `--png-dir DIR` also writes `sample_<i>_3d.png` and
`sample_<i>_2d.png`, the meshes rendered on the device.  `--keep-largest`, the simplification flags (`--target-faces N` and the others of
`process_meshes.py`), `--smooth N` and `--normals` apply the steps of `process_meshes.py`, in that order, to the decoded meshes before they
are written; without them nothing changes.  `--label K --guidance W` ask a class-conditional model (`ConditionalLatentDiffusion`:
the class comes from the checkpoint's hyper-parameters; `--num-classes K` builds the synthetic-weights model with a seeded embedding
table) for class K at classifier-free guidance scale W; both are logged and written to `generation.json` next to the meshes.  One
process, one GPU.
"""
from __future__ import annotations

import argparse
import json
import logging
import os

import numpy as np
import torch

import shapegen_amd  # noqa: F401
from shapegen_amd import dist as D
from shapegen_amd import specs
from shapegen_amd.checkpoint import read_checkpoint
from shapegen_amd.diffusion import ConditionalLatentDiffusion, LatentDiffusion
from shapegen_amd.utils import mesh_is_closed, save_mesh, save_shape_pngs, setup_logger
from shapegen_amd.vae import VAE3DLarge

LOG = "generate_logger_mesh_ldm"
DEFAULT_STEPS = {"dpm": 20, "ddim": 1000}


def build_model(vae_ckpt, ldm_ckpt, num_classes=0):
    if ldm_ckpt:                                        # one read: the model class comes from the file's hyper-parameters
        ck = read_checkpoint(ldm_ckpt)
        hp = dict(ck.get("hyper_parameters", {}))
        cls = ConditionalLatentDiffusion if hp.get("num_classes") else LatentDiffusion
        model = cls(VAE3DLarge(), **{k: hp[k] for k in cls._HP_KEYS if k in hp})
        model.load_state_dict(ck["state_dict"], strict=True)
        return model, "checkpoint"
    # (the constructor re-initialises the VAE's Linear layers, the reference's quirk: weights go in after it)
    model = ConditionalLatentDiffusion(VAE3DLarge(), num_classes) if num_classes else LatentDiffusion(VAE3DLarge())
    sd = specs.synth_state_dict(specs.latent_unet_spec(prefix="model."), seed=0, gain=1.3)
    sd.update(specs.synth_state_dict(specs.vae3d_large_spec(prefix="vae."), seed=0, gain=1.3))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    if num_classes:                                     # a seeded table, whatever was drawn before
        sd["model.class_emb.weight"] = torch.randn(num_classes + 1, 256, generator=torch.Generator().manual_seed(24))
    if vae_ckpt:
        sd.update({"vae." + k: v for k, v in VAE3DLarge.load_from_checkpoint(vae_ckpt).state_dict().items()})
    model.load_state_dict(sd, strict=True)
    return model, "vae_checkpoint" if vae_ckpt else "synthetic_weights"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vae-ckpt", default=None)
    ap.add_argument("--ldm-ckpt", default=None)
    ap.add_argument("--num-samples", type=int, default=16)
    ap.add_argument("--sampler", choices=("ddim", "dpm"), default="dpm")
    ap.add_argument("--steps", type=int, default=None, help="network evaluations; default 20 for dpm, 1000 for ddim")
    ap.add_argument("--threshold", type=float, default=0.4)
    ap.add_argument("--format", choices=("obj", "ply"), default="obj")
    ap.add_argument("--out", default=os.path.join("test", "outputs", "meshes"))
    ap.add_argument("--png-dir", default=None, metavar="DIR", help="also write the reference's pictures (sample_{i}_3d.png, sample_{i}_2d.png) here")
    ap.add_argument("--smooth", type=int, default=0, metavar="N", help="rounds of Taubin smoothing of the decoded meshes")
    ap.add_argument("--keep-largest", action="store_true", help="keep only the connected component with the most faces")
    ap.add_argument("--normals", action="store_true", help="write area-weighted vertex normals with the meshes")
    ap.add_argument("--label", type=int, default=None, metavar="K", help="class of every shape (class-conditional models)")
    ap.add_argument("--guidance", type=float, default=1.0, metavar="W", help="classifier-free guidance scale (1 = conditional only)")
    ap.add_argument("--num-classes", type=int, default=0, metavar="K",
                    help="without --ldm-ckpt: build the synthetic-weights model class-conditional with K classes")
    from shapegen_amd import mesh_ops
    mesh_ops.add_simplify_arguments(ap)
    args = ap.parse_args()
    steps = args.steps if args.steps is not None else DEFAULT_STEPS[args.sampler]
    torch.manual_seed(24)
    rank, world, local = D.init_from_env()
    device = torch.device("cuda", local)
    setup_logger(LOG, os.path.join("test", "logs", "mesh_ldm_generate.log"))
    log = logging.getLogger(LOG)
    model, name = build_model(args.vae_ckpt, args.ldm_ckpt, args.num_classes)
    model = model.to(device).eval()
    guide = {}
    if args.label is not None or args.guidance != 1.0:  # (an unconditional model refuses both)
        labels = None if args.label is None else torch.full((args.num_samples,), args.label, dtype=torch.int64)
        guide = {"labels": labels, "guidance_scale": args.guidance}
    with torch.no_grad():
        if args.sampler == "dpm":
            meshes = model.sample_dpm(args.num_samples, num_steps=steps, threshold=args.threshold, output="mesh", **guide)
        else:
            meshes = model.sample(args.num_samples, num_steps=steps, threshold=args.threshold, output="mesh", **guide)
    log.info(f"{name}: {len(meshes)} meshes, sampler {args.sampler}, {steps} steps, threshold {args.threshold}"
             + (f", label {args.label}, guidance {args.guidance}" if guide else ""))
    if rank != 0:
        return
    normals = None
    simplify = mesh_ops.simplify_keywords(args)
    if args.smooth or args.keep_largest or args.normals or any(simplify[k] is not None for k in ("simplify_resolution", "simplify_cell_size",
                                                                                                   "target_faces")):
        # components, then simplification, then smoothing, then normals (process_meshes.py)
        meshes, normals = mesh_ops.process_meshes(meshes, keep_largest=args.keep_largest, smooth=args.smooth, normals=args.normals, **simplify)
    os.makedirs(args.out, exist_ok=True)
    if guide:
        with open(os.path.join(args.out, "generation.json"), "w") as f:
            json.dump({"label": args.label, "guidance": args.guidance, "num_classes": int(model.num_classes), "sampler": args.sampler,
                       "steps": steps, "num_samples": len(meshes)}, f)
    for i, mesh in enumerate(meshes):
        path = os.path.join(args.out, f"mesh_{i}.{args.format}")
        save_mesh(path, mesh, normals=None if normals is None else normals[i])
        log.info(f"mesh {i}: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} triangles, closed {mesh_is_closed(mesh)} -> {path}")
        if args.png_dir:
            save_shape_pngs(args.png_dir, i, mesh)


if __name__ == "__main__":
    main()
