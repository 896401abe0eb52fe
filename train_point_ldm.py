"""Entry point kept from the reference (reference train_point_ldm.py:150-234): VAE -> VAE samples -> latent
diffusion -> latent-diffusion samples, on the HIP VAE3DLarge / latent denoiser.  `train_vae` (train_point_ldm.py:24-79)
runs on `training_vae.VAETrainer` (BCE + annealed KL, Adam, plateau scheduler), `train_diffusion` (:81-110) on the HIP
latent trainer (frozen VAE encode -> L1 loss -> AdamW + cosine schedule).

    python train_point_ldm.py [--vae-ckpt vae.ckpt | --train-vae-epochs N] [--diffusion-ckpt ldm.ckpt | --train-diffusion-epochs N]
                              [--data-dir DIR] [--category table] [--steps 1000]
                              [--resume-vae last.ckpt | --resume last.ckpt] [--save-last] [--ema-decay D]
                              [--grad-clip NORM] [--accumulate-grad-batches K] [--skip-nonfinite] [--device-data]
                              [--class-conditional [--p-uncond 0.1]]

`--vae-ckpt` / `--diffusion-ckpt` load weights only.  `--resume` continues an interrupted latent-diffusion training exactly
(`--resume-vae` the VAE's): optimizer moments, scheduler, epoch, top-k list and random streams come from the file, and
checkpoints keep going into the directory the file lies in.  `--save-last` writes `<name>-last.ckpt` after every epoch;
`--ema-decay` keeps an exponential moving average of the latent denoiser's weights next to the raw ones.
`--grad-clip`, `--accumulate-grad-batches` and `--skip-nonfinite` (gradient-norm clipping, one optimizer step per K batches,
dropping a step with a non-finite gradient) apply to both trainings.  `--device-data` feeds both from `DeviceVoxelDataModule`
(the directory read once, the grids bit-packed on the GPU, a batch unpacked by one launch).
`--class-conditional` trains a `ConditionalLatentDiffusion` for classifier-free guidance: the data layer labels every grid with its
category's index (`--category` takes a comma-separated list), one class per category, or without a data directory per synthetic
shape family; `--p-uncond` is the probability of training a shape without its label.  The VAE's training ignores the labels.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

import shapegen_amd  # noqa: F401
from shapegen_amd import specs
from shapegen_amd.diffusion import ConditionalLatentDiffusion, LatentDiffusion
from shapegen_amd.vae import VAE3DLarge as VAE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vae-ckpt", default=None, help="VAE weights (weights only)")
    ap.add_argument("--diffusion-ckpt", default=None, help="latent-diffusion weights (weights only)")
    ap.add_argument("--resume", default=None, metavar="PATH", help="continue the latent-diffusion run that wrote this checkpoint")
    ap.add_argument("--resume-vae", default=None, metavar="PATH", help="continue the VAE run that wrote this checkpoint")
    ap.add_argument("--save-last", action="store_true", help="also write <name>-last.ckpt after every epoch")
    ap.add_argument("--ema-decay", type=float, default=None, help="keep an exponential moving average of the denoiser's weights")
    ap.add_argument("--grad-clip", type=float, default=None, metavar="NORM", help="clip the gradient's L2 norm (pl.Trainer(gradient_clip_val=...))")
    ap.add_argument("--accumulate-grad-batches", type=int, default=1, metavar="K", help="one optimizer step per K batches")
    ap.add_argument("--skip-nonfinite", action="store_true", help="drop an optimizer step whose gradient holds a NaN or an infinity")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--train-vae-epochs", type=int, default=0, help="train the voxel VAE first (train_point_ldm.py:24-79, `train_vae`)")
    ap.add_argument("--train-diffusion-epochs", type=int, default=0, help="0 = the reference default (perform_diffusion_training = False)")
    ap.add_argument("--data-dir", default=os.path.join("data", "shape_net_voxel_data_v1"))
    ap.add_argument("--category", default="table")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--synthetic-shapes", type=int, default=160)
    ap.add_argument("--out", default=os.path.join("samples", "point_ldm"))
    ap.add_argument("--device-data", action="store_true",
                    help="with a data directory: keep its voxel grids on the GPU and assemble every batch there (DeviceVoxelDataModule)")
    ap.add_argument("--class-conditional", action="store_true",
                    help="train a class-conditional latent model (classifier-free guidance): one class per category of --category")
    ap.add_argument("--p-uncond", type=float, default=0.1, help="probability of replacing a training label by the null class")
    args = ap.parse_args()
    guard = dict(gradient_clip_val=args.grad_clip, accumulate_grad_batches=args.accumulate_grad_batches, skip_nonfinite=args.skip_nonfinite)
    torch.manual_seed(24)
    is_voxel_based = True                                     # train_point_ldm.py:160: VAE3DLarge path
    if args.vae_ckpt or args.resume_vae:
        vae = VAE.load_from_checkpoint(args.resume_vae or args.vae_ckpt)
    else:
        vae = VAE()
        sd = specs.synth_state_dict(specs.vae3d_large_spec(256), seed=2, gain=1.3)
        vae.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        print("no --vae-ckpt given: training is out of scope here, using synthetic VAE weights")
    vae = vae.to("cuda")
    # one data module for both fits (built only when something needs it); the number of classes comes with it
    needs_data = args.train_vae_epochs > 0 or args.train_diffusion_epochs > 0 or args.class_conditional
    data, num_classes = _data_module(args) if needs_data else (None, 0)
    if args.train_vae_epochs > 0:                            # train_point_ldm.py:24-79 (`train_vae`)
        from shapegen_amd.training import fit
        vae_dir = os.path.dirname(os.path.abspath(args.resume_vae)) if args.resume_vae else os.path.join("checkpoints", "point_ldm", "vae")
        fit(vae, _Unlabelled(data) if args.class_conditional else data, max_epochs=args.train_vae_epochs, ckpt_dir=vae_dir,
            ckpt_name="vae", ckpt_path=args.resume_vae, save_last=args.save_last, **guard)
    vae = vae.eval()
    os.makedirs(args.out, exist_ok=True)
    num_samples = 10
    samples_vae = vae.sample(num_samples=num_samples)                       # train_point_ldm.py:197
    np.savez_compressed(os.path.join(args.out, "vae_samples.npz"), **{f"sample_{i}": c.cpu().numpy() for i, c in enumerate(samples_vae)})
    print(f"Generated {num_samples} VAE samples")
    cls = ConditionalLatentDiffusion if args.class_conditional else LatentDiffusion
    if args.diffusion_ckpt or args.resume:
        diffusion = cls.load_from_checkpoint(args.resume or args.diffusion_ckpt, vae=vae, is_voxel_based=is_voxel_based)
        if diffusion.num_classes != num_classes:
            raise SystemExit(f"the checkpoint's model has {diffusion.num_classes} classes, the data {num_classes} "
                             "(--class-conditional and --category must match the run that wrote it)")
    else:
        diffusion = (ConditionalLatentDiffusion(vae, num_classes, p_uncond=args.p_uncond, is_voxel_based=is_voxel_based)
                     if args.class_conditional else LatentDiffusion(vae, is_voxel_based=is_voxel_based))
        lsd = specs.synth_state_dict(specs.latent_unet_spec(prefix="model."), seed=1, gain=1.3)
        cond = {"model.class_emb.weight": diffusion.model.class_emb.weight.detach()} if args.class_conditional else {}   # seeded above
        diffusion.load_state_dict({**{k: torch.from_numpy(np.asarray(v)) for k, v in lsd.items()},
                                   **{f"vae.{k}": v for k, v in vae.state_dict().items()}, **cond}, strict=True)
        print("no --diffusion-ckpt given: sampling the latent diffusion from synthetic weights")
    diffusion = diffusion.to("cuda")
    if args.train_diffusion_epochs > 0:                      # train_point_ldm.py:81-110 (`train_diffusion`)
        from shapegen_amd.training import fit
        ldm_dir = (os.path.dirname(os.path.abspath(args.resume)) if args.resume
                   else os.path.join("checkpoints", "point_ldm", "latent_diffusion"))
        fit(diffusion, data, max_epochs=args.train_diffusion_epochs, ckpt_dir=ldm_dir, ckpt_name="latent_diffusion",
            ckpt_path=args.resume, save_last=args.save_last, ema_decay=args.ema_decay, **guard)
    diffusion = diffusion.eval()
    guide = {"labels": torch.arange(num_samples) % num_classes} if num_classes else {}
    samples = diffusion.sample(num_samples=num_samples, num_steps=args.steps, **guide)  # train_point_ldm.py:222
    np.savez_compressed(os.path.join(args.out, "latent_diffusion_samples.npz"), **{f"sample_{i}": c.cpu().numpy() for i, c in enumerate(samples)})
    print(f"Generated {num_samples} diffusion denoised samples ({[int(c.shape[0]) for c in samples]} points)")


SYNTHETIC_FAMILIES = 3        # --class-conditional without a data directory: family f = grid index mod 3 has f + 1 ellipsoids


def _data_module(args):
    """(voxel batches, number of classes): the reference's data module (train_point_ldm.py:166-168) or synthetic occupancy grids;
    with --class-conditional the batches are (grids, labels), one class per category (or synthetic family), else 0 classes."""
    if os.path.isdir(args.data_dir):
        from shapegen_amd.data import DeviceVoxelDataModule, PointCloudDataDirectoryModule, PointCloudDataset
        module = DeviceVoxelDataModule if args.device_data else PointCloudDataDirectoryModule
        categories = args.category.split(",")
        labelled = {"return_labels": True} if args.class_conditional else {}
        dm = module(args.data_dir, num_points=2048, batch_size=args.batch_size, file_mode="voxels",
                    output_mode="voxels", augmentations=False, relevant_object_categories=categories, **labelled)
        num_classes = 0
        if args.class_conditional:                        # the categories that survive the filter, in label order
            found = PointCloudDataset(args.data_dir, input_mode="voxels", relevant_object_categories=categories, return_labels=True).categories
            num_classes = len(found)
            print(f"class-conditional over {num_classes} categories: {found}")
        return dm, num_classes
    families = SYNTHETIC_FAMILIES if args.class_conditional else 0
    print(f"{args.data_dir} not found: training on {args.synthetic_shapes} synthetic occupancy grids"
          + (f" of {families} shape families" if families else ""))
    return _SyntheticVoxels(args.synthetic_shapes, args.batch_size, families=families), families


class _Unlabelled:
    """A data module whose (grids, labels) batches leave as grids: the VAE's training ignores the labels."""

    def __init__(self, dm):
        self.dm = dm

    def __getattr__(self, name):                 # the split's index lists and whatever else identifies the data
        return getattr(self.dm, name)

    def setup(self):
        self.dm.setup()

    def train_dataloader(self):
        return (b[0] if isinstance(b, (tuple, list)) else b for b in self.dm.train_dataloader())

    def val_dataloader(self):
        return (b[0] if isinstance(b, (tuple, list)) else b for b in self.dm.val_dataloader())


class _SyntheticVoxels:
    """(B,1,32,32,32) occupancy batches of ellipsoid blobs, 80/20 train/val.  `families` > 0: grid i belongs to
    family i mod families, has family + 1 blobs, and the batches are (grids, labels)."""

    def __init__(self, count: int, batch_size: int, seed: int = 24, families: int = 0):
        rng = np.random.default_rng(seed)
        zz, yy, xx = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
        v = np.zeros((count, 1, 32, 32, 32), np.float32)
        for i in range(count):
            c, r = rng.uniform(8, 24, (3, 3)), rng.uniform(3, 9, (3, 3))
            for j in range(i % families + 1 if families else 3):
                v[i, 0][((zz - c[j, 0]) / r[j, 0]) ** 2 + ((yy - c[j, 1]) / r[j, 1]) ** 2 + ((xx - c[j, 2]) / r[j, 2]) ** 2 <= 1] = 1
        self.v, self.bs = torch.from_numpy(v), batch_size
        self.labels = torch.arange(count, dtype=torch.int64) % families if families else None

    def setup(self):
        self.n_train = int(0.8 * len(self.v))

    def _batches(self, lo, hi):
        if self.labels is None:
            return (self.v[i:i + self.bs] for i in range(lo, hi, self.bs))
        return ((self.v[i:i + self.bs], self.labels[i:i + self.bs]) for i in range(lo, hi, self.bs))

    def train_dataloader(self):
        return self._batches(0, self.n_train)

    def val_dataloader(self):
        return self._batches(self.n_train, len(self.v))


if __name__ == "__main__":
    main()
