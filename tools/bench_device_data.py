"""Host data module against `DeviceVoxelDataModule` on one GPU, on a synthetic directory this tool writes itself.

    python tools/bench_device_data.py [--shapes 2048] [--num-points 2048] [--batch-size 16] [--epochs 5] [--rounds 2] [--out profiles/device_data_bench.json]

Measures, in one process and one session:
  (a) shapes/s of `PointCloudDataDirectoryModule(num_workers=4)` iterated alone (train loader, one pass after a warm-up pass: page cache hot);
  (b) shapes/s of `DeviceVoxelDataModule` iterated alone, synchronised once at the end of the pass;
  (c) wall time per epoch of `training.fit` (point U-Net, batch x num_points) with each module, `--rounds` fits of `--epochs` epochs each in
      alternating order (host, device, host, device, ...), a fresh model per fit; every epoch time is kept, the summary is the median of
      the epochs after each fit's first (which also builds the trainer) and their range.
The host loader's worker count is the data module's default, 4; nothing here is sized by the machine's CPU count."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shapegen_amd  # noqa: E402,F401
from shapegen_amd.data import DeviceVoxelDataModule, PointCloudDataDirectoryModule  # noqa: E402


def write_directory(root: str, count: int, seed: int = 24) -> None:
    """`count` grids of three-ellipsoid unions (train_point_ddpm.py's synthetic recipe) as .npz files named like ShapeNet's."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    for i in range(count):
        c, r = rng.uniform(8, 24, (3, 3)), rng.uniform(3, 9, (3, 3))
        occ = np.zeros((32, 32, 32), bool)
        for j in range(3):
            occ |= ((zz - c[j, 0]) / r[j, 0]) ** 2 + ((yy - c[j, 1]) / r[j, 1]) ** 2 + ((xx - c[j, 2]) / r[j, 2]) ** 2 <= 1
        np.savez(os.path.join(root, f"vox_32_res_model_03001627_{i:05d}.npz"), data=occ.astype(np.float32))


def iterate(dm, passes: int) -> dict:
    """Shapes per second of the train loader alone: one warm-up pass, then the best and the mean of `passes` passes."""
    rates = []
    for k in range(passes + 1):
        t0 = time.perf_counter()
        shapes = 0
        for batch in dm.train_dataloader():
            shapes += int((batch[0] if isinstance(batch, (tuple, list)) else batch).shape[0])
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        if k:
            rates.append(shapes / (time.perf_counter() - t0))
    return {"shapes_per_pass": shapes, "passes": passes, "shapes_per_s_mean": float(np.mean(rates)), "shapes_per_s_best": float(max(rates)),
            "shapes_per_s_all": [float(r) for r in rates]}


def fit_epochs(dm, args) -> dict:
    from shapegen_amd.diffusion import PointCloudDiffusion
    from shapegen_amd.training import fit
    torch.manual_seed(24)
    model = PointCloudDiffusion(num_points=args.num_points).to("cuda")
    marks = [time.perf_counter()]

    def log(line):
        torch.cuda.synchronize()
        marks.append(time.perf_counter())

    history = fit(model, dm, max_epochs=args.epochs, log=log)
    per_epoch = [b - a for a, b in zip(marks[:-1], marks[1:])][:args.epochs]
    return {"epoch_s_all": per_epoch, "final_train_loss": history[-1][1], "final_val_loss": history[-1][2]}


def summarise(fits: list) -> dict:
    later = [t for f in fits for t in f["epoch_s_all"][1:]]
    return {"fits": fits, "epoch_s_after_first_median": float(np.median(later)) if later else None,
            "epoch_s_after_first_min": min(later) if later else None, "epoch_s_after_first_max": max(later) if later else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=2048)
    ap.add_argument("--num-points", type=int, default=2048)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_data_bench.json"))
    args = ap.parse_args()
    kw = dict(num_points=args.num_points, batch_size=args.batch_size, file_mode="voxels", output_mode="point_clouds", augmentations=False)
    result = {"shapes": args.shapes, "num_points": args.num_points, "batch_size": args.batch_size, "host_num_workers": 4,
              "files": "float32 32^3 .npz (np.savez), three-ellipsoid unions", "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_directory(root, args.shapes)
        result["write_directory_s"] = time.perf_counter() - t0

        def host():
            torch.manual_seed(24)
            dm = PointCloudDataDirectoryModule(root, num_workers=4, **kw)
            dm.setup()
            return dm

        def device():
            torch.manual_seed(24)
            dm = DeviceVoxelDataModule(root, **kw)
            t0 = time.perf_counter()
            dm.setup()
            torch.cuda.synchronize()
            result["device_setup_s"] = time.perf_counter() - t0
            return dm

        dm = device()
        result["voxels_per_shape"] = {"min": int(dm.counts.min()), "mean": float(dm.counts.mean()), "max": int(dm.counts.max())}
        result["packed_table_bytes"] = int(dm.packed.numel() * 4)
        result["a_host_loader_alone"] = iterate(host(), args.passes)
        result["b_device_loader_alone"] = iterate(dm, args.passes)
        fits = {"host": [], "device": []}
        for _ in range(args.rounds):                        # alternating, so that a drift of the box or the process hits both
            fits["host"].append(fit_epochs(host(), args))
            fits["device"].append(fit_epochs(device(), args))
        result["c_fit_order"] = "host, device" + ", host, device" * (args.rounds - 1)
        result["c_fit_host"], result["c_fit_device"] = summarise(fits["host"]), summarise(fits["device"])
    a, b = result["a_host_loader_alone"]["shapes_per_s_mean"], result["b_device_loader_alone"]["shapes_per_s_mean"]
    result["loader_ratio_device_over_host"] = b / a
    h, d = result["c_fit_host"]["epoch_s_after_first_median"], result["c_fit_device"]["epoch_s_after_first_median"]
    result["fit_epoch_ratio_host_over_device"] = (h / d) if h and d else None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
