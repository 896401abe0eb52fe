"""Training entry point with the reference's surface (reference train_point_ddpm.py:25-99): build the data module
(voxel files -> 2048-point clouds, batch 16), construct or load `PointCloudDiffusion`, train it, then draw 10 samples.
Training runs on the HIP trainer (`shapegen_amd.training`): fp16 MFMA GEMMs for every forward / backward product,
BatchNorm batch statistics, L1 loss, AdamW + ReduceLROnPlateau, top-k checkpoints by val_loss in the reference's
`.ckpt` layout.

    python train_point_ddpm.py [--data-dir DIR] [--category chair] [--epochs 500] [--ckpt weights.ckpt] [--max-steps N]
                               [--backbone {pointnet,attention}] [--resume last.ckpt] [--save-last] [--ema-decay D]
                               [--grad-clip NORM] [--accumulate-grad-batches K] [--skip-nonfinite]
                               [--class-conditional [--p-uncond 0.1]] [--device-data] [--mesh-data [DIR]]

`--backbone attention` trains `UNetAttentionPointExperimental` (the reference reaches it by editing diffusion.py's
import); `--ckpt` starts a new run from a checkpoint's weights (with the backbone stored in its hyper-parameters).
`--resume` continues an interrupted run exactly: weights, optimizer moments, scheduler, epoch, top-k list and random
streams come from the file, and checkpoints keep going into the directory the file lies in.  `--save-last` writes
`point_cloud_diffusion-last.ckpt` after every epoch (the file to resume from); `--ema-decay` keeps an exponential moving
average of the weights, saved next to the raw ones (`PointCloudDiffusion.load_from_checkpoint(path, weights="ema")`).
`--grad-clip` and `--accumulate-grad-batches` are `pl.Trainer(gradient_clip_val=..., accumulate_grad_batches=...)`;
`--skip-nonfinite` (implied by `--grad-clip`) drops an optimizer step whose gradient holds a NaN or an infinity.  The epoch
log line then carries the last gradient norm and the clipped / skipped counts.

`--class-conditional` trains a class-conditional model for classifier-free guidance: the data layer labels every cloud with
its category's index (`--category` takes a comma-separated list, or `all`), the model gets one embedding row per category plus
the null class, and each label is replaced by the null class with probability `--p-uncond`.  The samples drawn at the end cycle
through the classes.

`--device-data` feeds the trainer from `DeviceVoxelDataModule`: the directory is read once, the grids stay bit-packed on the GPU and
every batch is one kernel launch (Philox draws, subsets in scan order; `shapegen_amd.data`).  Without it nothing changes.

`--mesh-data DIR` feeds the trainer from `DeviceMeshDataModule`: every `.obj` / `.ply` file under DIR is read once, the triangles stay
on the GPU and every batch of every epoch is a fresh area-uniform draw of `--num-points` surface points per mesh, jittered and
normalised, in one kernel launch.  With `--class-conditional` the categories are DIR's subdirectories.  Without DIR (or when it does
not exist) the run builds boxes and ellipsoids in memory, one class each.

Without a data directory (none ships with the reference) it trains on synthetic ShapeNet-shaped clouds so the whole
loop can be exercised.
"""
from __future__ import annotations

import argparse
import os
from datetime import datetime

import numpy as np
import torch

import shapegen_amd  # noqa: F401
from shapegen_amd.data import DeviceMeshDataModule, DeviceVoxelDataModule, PointCloudDataDirectoryModule, PointCloudDataModule
from shapegen_amd.diffusion import PointCloudDiffusion
from shapegen_amd.training import fit
from shapegen_amd.utils import setup_logger


def synthetic_clouds(count: int, num_points: int, seed: int = 24) -> np.ndarray:
    """Grid-like clouds shaped like data.py:213-254 output: voxel coordinates of blobs, centred, unit radius."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    out = np.zeros((count, num_points, 3), np.float32)
    for i in range(count):
        c, r = rng.uniform(8, 24, (3, 3)), rng.uniform(3, 9, (3, 3))
        occ = np.zeros((32, 32, 32), bool)
        for j in range(3):
            occ |= ((zz - c[j, 0]) / r[j, 0]) ** 2 + ((yy - c[j, 1]) / r[j, 1]) ** 2 + ((xx - c[j, 2]) / r[j, 2]) ** 2 <= 1
        pts = np.stack(np.where(occ), 1).astype(np.float32)
        pts -= pts.mean(0)
        pts /= np.linalg.norm(pts, axis=1).max()
        out[i] = pts[rng.choice(len(pts), num_points, replace=len(pts) < num_points)]
    return out


SYNTHETIC_FAMILIES = 3


def synthetic_grids(count: int, seed: int = 24, families: int = 0):
    """(grids, labels) for --device-data without a data directory: the occupancy grids behind `synthetic_clouds` (families = 0, three
    ellipsoids each, labels None) or `synthetic_labelled_clouds` (family f = grid index mod `families`: f + 1 ellipsoids)."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    grids = np.zeros((count, 32, 32, 32), np.float32)
    labels = np.arange(count, dtype=np.int64) % families if families else None
    for i in range(count):
        blobs = int(labels[i]) + 1 if families else 3
        c, r = rng.uniform(8, 24, (blobs, 3)), rng.uniform(3, 9, (blobs, 3))
        for j in range(blobs):
            grids[i][((zz - c[j, 0]) / r[j, 0]) ** 2 + ((yy - c[j, 1]) / r[j, 1]) ** 2 + ((xx - c[j, 2]) / r[j, 2]) ** 2 <= 1] = 1
    return grids, labels


SYNTHETIC_MESH_FAMILIES = 2
_BOX_FACES = ((0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (2, 3, 7), (2, 7, 6), (1, 2, 6), (1, 6, 5), (0, 4, 7), (0, 7, 3))


def synthetic_meshes(count: int, seed: int = 24, rings: int = 12, segments: int = 16):
    """(meshes, labels) for --mesh-data without a directory: mesh i is a box of random extents (label 0, 12 triangles) for even i and a
    latitude / longitude ellipsoid of random semi-axes (label 1) for odd i; (vertices float32 (V, 3), faces int32 (F, 3)) pairs."""
    rng = np.random.default_rng(seed)
    meshes, labels = [], np.arange(count, dtype=np.int64) % SYNTHETIC_MESH_FAMILIES
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segments) / segments
    sphere = np.concatenate([[(0.0, 0.0, 1.0)], np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)),
                                                          np.outer(np.cos(th), np.ones(segments))], axis=2).reshape(-1, 3), [(0.0, 0.0, -1.0)]])
    at = lambda r, s: 1 + (r - 1) * segments + s % segments        # noqa: E731
    faces = []
    for s in range(segments):
        faces += [(0, at(1, s), at(1, s + 1)), (len(sphere) - 1, at(rings - 1, s + 1), at(rings - 1, s))]
        for r in range(1, rings - 1):
            faces += [(at(r, s), at(r + 1, s), at(r + 1, s + 1)), (at(r, s), at(r + 1, s + 1), at(r, s + 1))]
    for i in range(count):
        half = rng.uniform(0.3, 1.0, 3)
        if labels[i] == 0:
            lo, hi = -half, half
            v = [(lo[0], lo[1], lo[2]), (hi[0], lo[1], lo[2]), (hi[0], hi[1], lo[2]), (lo[0], hi[1], lo[2]),
                 (lo[0], lo[1], hi[2]), (hi[0], lo[1], hi[2]), (hi[0], hi[1], hi[2]), (lo[0], hi[1], hi[2])]
            meshes.append((np.asarray(v, np.float32), np.asarray(_BOX_FACES, np.int32)))
        else:
            meshes.append(((sphere * half).astype(np.float32), np.asarray(faces, np.int32)))
    return meshes, labels


def synthetic_labelled_clouds(count: int, num_points: int, seed: int = 24):
    """(clouds, labels) for --class-conditional without a data directory: `synthetic_clouds`' recipe in SYNTHETIC_FAMILIES
    shape families, family f (= cloud index mod the family count, the cloud's label) being the union of f + 1 ellipsoids."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    out = np.zeros((count, num_points, 3), np.float32)
    labels = np.arange(count, dtype=np.int64) % SYNTHETIC_FAMILIES
    for i in range(count):
        blobs = int(labels[i]) + 1
        c, r = rng.uniform(8, 24, (blobs, 3)), rng.uniform(3, 9, (blobs, 3))
        occ = np.zeros((32, 32, 32), bool)
        for j in range(blobs):
            occ |= ((zz - c[j, 0]) / r[j, 0]) ** 2 + ((yy - c[j, 1]) / r[j, 1]) ** 2 + ((xx - c[j, 2]) / r[j, 2]) ** 2 <= 1
        pts = np.stack(np.where(occ), 1).astype(np.float32)
        pts -= pts.mean(0)
        pts /= np.linalg.norm(pts, axis=1).max()
        out[i] = pts[rng.choice(len(pts), num_points, replace=len(pts) < num_points)]
    return out, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=None, help="reference-layout .ckpt whose weights start a new run (weights only: see --resume)")
    ap.add_argument("--resume", default=None, metavar="PATH",
                    help="continue the run that wrote this checkpoint: optimizer, scheduler, epoch, top-k list and RNG are restored")
    ap.add_argument("--save-last", action="store_true", help="also write <name>-last.ckpt after every epoch")
    ap.add_argument("--ema-decay", type=float, default=None, help="keep an exponential moving average of the weights")
    ap.add_argument("--grad-clip", type=float, default=None, metavar="NORM", help="clip the gradient's L2 norm (pl.Trainer(gradient_clip_val=...))")
    ap.add_argument("--accumulate-grad-batches", type=int, default=1, metavar="K", help="one optimizer step per K batches")
    ap.add_argument("--skip-nonfinite", action="store_true", help="drop an optimizer step whose gradient holds a NaN or an infinity")
    ap.add_argument("--data-dir", default=os.path.join("data", "shape_net_voxel_data_v1"))
    ap.add_argument("--category", default="chair")
    ap.add_argument("--num-points", type=int, default=2048)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--synthetic-shapes", type=int, default=160)
    ap.add_argument("--sample-steps", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join("samples", "point_cloud_diffusion"))
    ap.add_argument("--backbone", choices=("pointnet", "attention"), default="pointnet",
                    help="denoiser of a new model (a resumed checkpoint keeps its own)")
    ap.add_argument("--class-conditional", action="store_true",
                    help="train a class-conditional model (classifier-free guidance): one class per category of --category")
    ap.add_argument("--p-uncond", type=float, default=0.1, help="probability of replacing a training label by the null class")
    ap.add_argument("--device-data", action="store_true",
                    help="keep the voxel grids on the GPU and assemble every batch there in one launch (DeviceVoxelDataModule)")
    ap.add_argument("--mesh-data", nargs="?", const="", default=None, metavar="DIR",
                    help="train on fresh surface samples of the .obj / .ply meshes under DIR, kept on the GPU (DeviceMeshDataModule); "
                         "categories are DIR's subdirectories; without DIR: boxes and ellipsoids built in memory")
    args = ap.parse_args()
    if args.mesh_data is not None and args.device_data:
        ap.error("--mesh-data and --device-data are two data sources: give one")
    torch.manual_seed(24)
    timestamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    logger = setup_logger("train_point_ddpm", os.path.join("train", "logs", f"train_point_ddpm_log_{timestamp}.log"))
    num_classes = 0
    if args.mesh_data is not None and os.path.isdir(args.mesh_data):
        dm = DeviceMeshDataModule(args.mesh_data, num_points=args.num_points, batch_size=args.batch_size, return_labels=args.class_conditional)
        if args.class_conditional:
            from shapegen_amd.data import mesh_category, mesh_files
            found = sorted({mesh_category(f) for f in mesh_files(args.mesh_data)})
            num_classes = len(found)
            logger.info(f"class-conditional over {num_classes} categories: {found}")
    elif args.mesh_data is not None:
        logger.info(f"no mesh directory{' ' + repr(args.mesh_data) if args.mesh_data else ''}: training on {args.synthetic_shapes} boxes and "
                    "ellipsoids kept on the GPU")
        meshes, labels = synthetic_meshes(args.synthetic_shapes)
        dm = DeviceMeshDataModule(meshes=meshes, labels=labels, num_points=args.num_points, batch_size=args.batch_size,
                                  return_labels=args.class_conditional)
        num_classes = SYNTHETIC_MESH_FAMILIES if args.class_conditional else 0
    elif os.path.isdir(args.data_dir):
        categories = args.category.split(",")
        module = DeviceVoxelDataModule if args.device_data else PointCloudDataDirectoryModule
        dm = module(args.data_dir, num_points=args.num_points, batch_size=args.batch_size, file_mode="voxels",
                    output_mode="point_clouds", augmentations=False,
                    relevant_object_categories=categories, return_labels=args.class_conditional)
        if args.class_conditional:
            from shapegen_amd.data import PointCloudDataset
            found = PointCloudDataset(args.data_dir, input_mode="voxels", relevant_object_categories=categories, return_labels=True).categories
            num_classes = len(found)
            logger.info(f"class-conditional over {num_classes} categories: {found}")
    elif args.device_data:
        logger.info(f"{args.data_dir} not found: training on {args.synthetic_shapes} synthetic grids kept on the GPU")
        grids, labels = synthetic_grids(args.synthetic_shapes, families=SYNTHETIC_FAMILIES if args.class_conditional else 0)
        dm = DeviceVoxelDataModule(grids=grids, labels=labels, num_points=args.num_points, batch_size=args.batch_size,
                                   augmentations=False, return_labels=args.class_conditional)
        num_classes = SYNTHETIC_FAMILIES if args.class_conditional else 0
    elif args.class_conditional:
        logger.info(f"{args.data_dir} not found: training on {args.synthetic_shapes} synthetic clouds of {SYNTHETIC_FAMILIES} shape families")
        clouds, labels = synthetic_labelled_clouds(args.synthetic_shapes, args.num_points)
        dm = _Unwrap(PointCloudDataModule(clouds, batch_size=args.batch_size, labels=labels))
        num_classes = SYNTHETIC_FAMILIES
    else:
        logger.info(f"{args.data_dir} not found: training on {args.synthetic_shapes} synthetic clouds")
        dm = _Unwrap(PointCloudDataModule(synthetic_clouds(args.synthetic_shapes, args.num_points), batch_size=args.batch_size))
    if args.ckpt or args.resume:
        logger.info(f"Loading Diffusion model from checkpoint: {args.resume or args.ckpt}")
        model = PointCloudDiffusion.load_from_checkpoint(args.resume or args.ckpt)
        assert model.num_points == args.num_points
        if model.backbone != args.backbone:
            logger.info(f"checkpoint backbone {model.backbone!r} is used (--backbone {args.backbone} ignored)")
        if model.num_classes != num_classes:
            raise SystemExit(f"the checkpoint's model has {model.num_classes} classes, the data {num_classes} "
                             "(--class-conditional and --category must match the run that wrote it)")
    else:
        model = PointCloudDiffusion(num_points=args.num_points, backbone=args.backbone, num_classes=num_classes, p_uncond=args.p_uncond)
    model = model.to("cuda")
    logger.info("Starting Diffusion Training")
    # a resumed run keeps writing where the file it resumed from lies: the restored top-k list prunes the files it names
    ckpt_dir = os.path.dirname(os.path.abspath(args.resume)) if args.resume else os.path.join("checkpoints", "point_ddpm", timestamp)
    fit(model, dm, max_epochs=args.epochs, ckpt_dir=ckpt_dir, log=logger.info, max_steps=args.max_steps, ckpt_path=args.resume,
        save_last=args.save_last, ema_decay=args.ema_decay, gradient_clip_val=args.grad_clip,
        accumulate_grad_batches=args.accumulate_grad_batches, skip_nonfinite=args.skip_nonfinite)
    model.eval()
    guide = {"labels": torch.arange(10) % num_classes} if num_classes else {}
    samples = model.sample(num_samples=10, num_points=args.num_points, num_steps=args.sample_steps, **guide)   # train_point_ddpm.py:91-93
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "samples.npy"), samples.cpu().numpy())
    print(f"wrote {samples.shape[0]} clouds of {samples.shape[1]} points to {args.out}")


class _Unwrap:
    """PointCloudDataModule yields 1-tuples (TensorDataset, data.py:32); the training loop wants the tensor."""

    def __init__(self, dm):
        self.dm = dm

    def setup(self):
        self.dm.setup()
        self.train_dataset, self.val_dataset = self.dm.train_dataset, self.dm.val_dataset     # their index lists identify the split

    def train_dataloader(self):
        return (b[0] if len(b) == 1 else tuple(b) for b in self.dm.train_dataloader())      # labelled: (clouds, labels)

    def val_dataloader(self):
        return (b[0] if len(b) == 1 else tuple(b) for b in self.dm.val_dataloader())


if __name__ == "__main__":
    main()
