"""Shape completion entry point: cut validation clouds with a plane, complete the kept part with a trained
unconditional point DDPM (`PointCloudDiffusion.complete`, RePaint-style resampling) and score the result.

    python complete_point_ddpm.py [--ckpt-dir DIR] [--clouds FILE.npy] [--num-samples 16] [--num-points 2048]
                                  [--steps 1000] [--resample 10] [--jump 10] [--cut 0.0] [--png-dir DIR]
                                  [--remove-outliers [--outlier-k 16] [--outlier-ratio 2.0]] [--ply-dir DIR]
                                  [--mesh-dir DIR [--mesh-resolution 64] [--mesh-format obj|ply] [--mesh-radius-scale 1.5]]

The points of each cloud with x < `--cut` are kept, moved to the front and handed over as the partial input, so the
known counts are ragged.  Every `.ckpt` of `--ckpt-dir` is evaluated; without checkpoints (none ship with the reference)
a model with deterministic synthetic weights runs, and without `--clouds` (a (B, N, 3) .npy of unit-sphere-scaled
clouds) the synthetic ShapeNet-shaped clouds of test_point_ddpm.py are used, so the plumbing is exercised end to end.
`--png-dir DIR` also writes `sample_<i>_3d.png`, `sample_<i>_2d.png` (the completion) and `comparison_<i>.png` (original | completion).
`--remove-outliers` drops the stray points of every completion on the device (`geometry.remove_outliers`, `--outlier-k` neighbours,
`--outlier-ratio` standard deviations) and stores `filtered` / `filtered_counts` next to the untouched `completion` (the metrics stay those
of the completion as sampled); the pictures and PLY files then show the filtered clouds.  `--ply-dir DIR` writes one `sample_<i>.ply` per
completion with estimated outward normals.  `--mesh-dir DIR` writes one closed triangle mesh `sample_<i>.obj` (or `.ply`) per completion, the
filtered one under `--remove-outliers` (`geometry.cloud_to_meshes` on a grid of `--mesh-resolution` nodes per axis, closing radius
`--mesh-radius-scale` point spacings), and logs vertices, faces and enclosed nodes per shape.
Multi-GPU: launch with torch.distributed.run; shapes are sharded across ranks and metric rows are all-gathered.
"""
from __future__ import annotations

import argparse
import glob
import logging
import os

import numpy as np
import torch

import shapegen_amd  # noqa: F401
from shapegen_amd import dist as D
from shapegen_amd import specs
from shapegen_amd.diffusion import PointCloudDiffusion
from shapegen_amd.geometry import remove_outliers, save_cloud_meshes, save_cloud_plys
from shapegen_amd.utils import save_shape_pngs, setup_logger
from test_point_ddpm import synthetic_clouds

LOG = "complete_logger_point_ddpm"


def cut_clouds(clouds: torch.Tensor, cut: float):
    """Keep the points with x < cut: (partial (B, N, 3) with the kept points first and zeros behind them, counts (B,))."""
    partial = torch.zeros_like(clouds)
    counts = torch.zeros(clouds.shape[0], dtype=torch.int64)
    for b in range(clouds.shape[0]):
        kept = clouds[b][clouds[b, :, 0] < cut]
        partial[b, :kept.shape[0]] = kept
        counts[b] = kept.shape[0]
    return partial, counts


def complete_and_score(model, model_name, original, partial, counts, num_steps, resample, jump):
    """Completions of the global batch (all ranks get all of them) and the per-sample (CD, EMD, voxel BCE) rows against the originals."""
    rank, world = D.world()
    lo, hi = D.shard_range(original.shape[0], rank, world)
    with torch.no_grad():
        done = D.complete_sharded(model, partial, counts, original.shape[1], num_steps, resample=resample, jump=jump)
        rows, mean = D.evaluate_sharded(original[lo:hi].to(model.device), done[lo:hi].contiguous())
    log = logging.getLogger(LOG)
    for i, row in enumerate(rows.tolist()):
        log.info(f"{model_name} sample {i}: {int(counts[i])} of {original.shape[1]} points known, Chamfer Distance {row[0]:.3f}")
    log.info(f"{model_name}: Average Chamfer Distance between completion and original: {float(mean[0]):.3f}")
    return done, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt-dir", default=os.path.join("checkpoints", "best_run", "point_cloud_diffusion"))
    ap.add_argument("--clouds", default=None, help="(B, N, 3) .npy of validation clouds; default: synthetic clouds")
    ap.add_argument("--num-samples", type=int, default=16)
    ap.add_argument("--num-points", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--resample", type=int, default=10)
    ap.add_argument("--jump", type=int, default=10)
    ap.add_argument("--cut", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join("test", "outputs"))
    ap.add_argument("--png-dir", default=None, metavar="DIR", help="also write the reference's pictures (sample_{i}_3d.png, sample_{i}_2d.png, comparison_{i}.png) here")
    ap.add_argument("--remove-outliers", action="store_true", help="drop stray points (statistical outlier removal) and store `filtered`")
    ap.add_argument("--outlier-k", type=int, default=16, metavar="K", help="neighbours of the outlier rule and of the PLY normals")
    ap.add_argument("--outlier-ratio", type=float, default=2.0, metavar="R", help="standard deviations above the mean neighbour distance")
    ap.add_argument("--ply-dir", default=None, metavar="DIR", help="also write sample_{i}.ply with estimated outward normals here")
    ap.add_argument("--mesh-dir", default=None, metavar="DIR", help="also write one closed triangle mesh sample_{i}.obj|ply per cloud here")
    ap.add_argument("--mesh-resolution", type=int, default=64, metavar="R", help="grid nodes per axis of the cloud-to-mesh closing, 8 .. 64")
    ap.add_argument("--mesh-format", choices=("obj", "ply"), default="obj")
    ap.add_argument("--mesh-radius-scale", type=float, default=1.5, metavar="S", help="closing radius in units of the cloud's point spacing")
    args = ap.parse_args()
    if not 8 <= args.mesh_resolution <= 64:
        ap.error("--mesh-resolution must lie in 8 .. 64")
    torch.manual_seed(24)
    rank, world, local = D.init_from_env()
    device = torch.device("cuda", local)
    setup_logger(LOG, os.path.join("test", "logs", "point_ddpm_complete.log"))
    models = [(os.path.basename(path)[:-5], PointCloudDiffusion.load_from_checkpoint(path))
              for path in sorted(glob.glob(os.path.join(args.ckpt_dir, "*.ckpt")))]
    if not models:
        m = PointCloudDiffusion(num_points=args.num_points)
        sd = specs.synth_state_dict(specs.unet_pointnet_large_spec(prefix="model."), seed=0, gain=1.3)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        models.append(("synthetic_weights", m))
    if args.clouds:
        val = torch.from_numpy(np.load(args.clouds).astype(np.float32))[:args.num_samples]
        if val.dim() != 3 or val.shape[2] != 3:
            raise ValueError(f"--clouds must hold a (B, N, 3) array, got {tuple(val.shape)}")
    else:
        val = synthetic_clouds(args.num_samples, args.num_points)
    partial, counts = cut_clouds(val, args.cut)
    result = {"partial": partial.numpy(), "counts": counts.numpy()}
    for name, model in models:
        model = model.to(device).eval()
        done, rows = complete_and_score(model, name, val, partial, counts, args.steps, args.resample, args.jump)
        tag = "" if len(models) == 1 else "_" + name
        result["completion" + tag], result["metrics" + tag] = done.cpu().numpy(), rows.cpu().numpy()
        shapes, kept_counts = done, [done.shape[1]] * done.shape[0]
        if args.remove_outliers:
            shapes, kept = remove_outliers(done.contiguous(), k=args.outlier_k, std_ratio=args.outlier_ratio)
            kept_counts = kept.tolist()
            result["filtered" + tag], result["filtered_counts" + tag] = shapes.cpu().numpy(), kept.cpu().numpy()
            logging.getLogger(LOG).info(f"{name}: outlier removal (k {args.outlier_k}, ratio {args.outlier_ratio}) kept {sum(kept_counts)} of "
                                        f"{done.shape[0] * done.shape[1]} points")
        if args.png_dir and rank == 0:
            for i in range(done.shape[0]):
                save_shape_pngs(os.path.join(args.png_dir, name) if len(models) > 1 else args.png_dir, i, shapes[i, :kept_counts[i]], val[i].to(device))
        if args.ply_dir and rank == 0:
            save_cloud_plys(os.path.join(args.ply_dir, name) if len(models) > 1 else args.ply_dir, shapes, kept_counts, k=args.outlier_k)
        if args.mesh_dir and rank == 0:
            save_cloud_meshes(os.path.join(args.mesh_dir, name) if len(models) > 1 else args.mesh_dir, shapes.contiguous(), kept_counts,
                              resolution=args.mesh_resolution, radius_scale=args.mesh_radius_scale, fmt=args.mesh_format, log=logging.getLogger(LOG))
    if rank == 0:
        os.makedirs(args.out, exist_ok=True)
        np.savez_compressed(os.path.join(args.out, "completions.npz"), **result)


if __name__ == "__main__":
    main()
