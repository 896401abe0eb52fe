"""Generation entry point of the latent route with surfaces out: sample latents, decode them to 32^3 occupancy grids and write one
triangle mesh per shape.

    python generate_mesh_ldm.py [--vae-ckpt FILE] [--ldm-ckpt FILE] [--num-samples 16] [--sampler ddim|dpm] [--steps N]
                                [--threshold 0.4] [--format obj|ply] [--out DIR] [--png-dir DIR]
                                [--smooth N] [--keep-largest] [--normals]
                                [--simplify-resolution R | --simplify-cell H | --target-faces N] [--placement quadric|mean] [--deduplicate]

`--sampler dpm` (default, 20 steps) is `LatentDiffusion.sample_dpm`, `ddim` (default 1000 steps) is `sample`; both run with
`output="mesh"`, so the decoded grids go through the surface-nets kernel (`utils.voxel_tensor_to_meshes`) at `--threshold`, the
predicate of the point conversion.  The latent-diffusion checkpoint carries the VAE's weights too (`vae.*` keys); `--vae-ckpt` alone gives
a trained VAE under a denoiser with synthetic weights.  Without checkpoints (none ship with the reference) both run on deterministic
synthetic weights, so the plumbing is exercised end to end.  One file `mesh_<i>.<format>` per shape goes to `--out`; vertices are in
the [-1, 1] cube of the point clouds (a surface that reaches the grid's border closes up to one voxel pitch outside it).  Per shape
the log gives the vertex and triangle counts and whether the mesh is closed.  `--png-dir DIR` also writes `sample_<i>_3d.png` and
`sample_<i>_2d.png`, the meshes rendered on the device.  `--keep-largest`, the simplification flags (`--target-faces N` and the others of
`process_meshes.py`), `--smooth N` and `--normals` apply the steps of `process_meshes.py`, in that order, to the decoded meshes before they
are written; without them nothing changes.  One process, one GPU.
"""
from __future__ import annotations

import argparse
import logging
import os

import numpy as np
import torch

import shapegen_amd  # noqa: F401
from shapegen_amd import dist as D
from shapegen_amd import specs
from shapegen_amd.diffusion import LatentDiffusion
from shapegen_amd.utils import mesh_is_closed, save_mesh, save_shape_pngs, setup_logger
from shapegen_amd.vae import VAE3DLarge

LOG = "generate_logger_mesh_ldm"
DEFAULT_STEPS = {"dpm": 20, "ddim": 1000}


def build_model(vae_ckpt, ldm_ckpt):
    if ldm_ckpt:
        return LatentDiffusion.load_from_checkpoint(ldm_ckpt, vae=VAE3DLarge()), "checkpoint"
    model = LatentDiffusion(VAE3DLarge())              # re-initialises the VAE's Linear layers (the reference's quirk): weights go in after it
    sd = specs.synth_state_dict(specs.latent_unet_spec(prefix="model."), seed=0, gain=1.3)
    sd.update(specs.synth_state_dict(specs.vae3d_large_spec(prefix="vae."), seed=0, gain=1.3))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
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
    from shapegen_amd import mesh_ops
    mesh_ops.add_simplify_arguments(ap)
    args = ap.parse_args()
    steps = args.steps if args.steps is not None else DEFAULT_STEPS[args.sampler]
    torch.manual_seed(24)
    rank, world, local = D.init_from_env()
    device = torch.device("cuda", local)
    setup_logger(LOG, os.path.join("test", "logs", "mesh_ldm_generate.log"))
    log = logging.getLogger(LOG)
    model, name = build_model(args.vae_ckpt, args.ldm_ckpt)
    model = model.to(device).eval()
    with torch.no_grad():
        if args.sampler == "dpm":
            meshes = model.sample_dpm(args.num_samples, num_steps=steps, threshold=args.threshold, output="mesh")
        else:
            meshes = model.sample(args.num_samples, num_steps=steps, threshold=args.threshold, output="mesh")
    log.info(f"{name}: {len(meshes)} meshes, sampler {args.sampler}, {steps} steps, threshold {args.threshold}")
    if rank != 0:
        return
    normals = None
    simplify = mesh_ops.simplify_keywords(args)
    if args.smooth or args.keep_largest or args.normals or any(simplify[k] is not None for k in ("simplify_resolution", "simplify_cell_size",
                                                                                                   "target_faces")):
        # components, then simplification, then smoothing, then normals (process_meshes.py)
        meshes, normals = mesh_ops.process_meshes(meshes, keep_largest=args.keep_largest, smooth=args.smooth, normals=args.normals, **simplify)
    os.makedirs(args.out, exist_ok=True)
    for i, mesh in enumerate(meshes):
        path = os.path.join(args.out, f"mesh_{i}.{args.format}")
        save_mesh(path, mesh, normals=None if normals is None else normals[i])
        log.info(f"mesh {i}: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} triangles, closed {mesh_is_closed(mesh)} -> {path}")
        if args.png_dir:
            save_shape_pngs(args.png_dir, i, mesh)


if __name__ == "__main__":
    main()
