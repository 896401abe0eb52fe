"""`DeviceMeshDataModule` on one GPU, one process, one session: its one launch, its loader alone and an epoch of `fit`, each against the
route a user of meshes had before it -- `preprocess_meshes.py --points-dir` once, then `PointCloudDataDirectoryModule(file_mode="point_clouds",
num_workers=4)` reading the cloud files on the host.

    python tools/bench_mesh_data.py [--batch 32] [--num-points 2048] [--rounds 100] [--warmup 10] [--shapes 512] [--batch-size 16]
                                    [--epochs 4] [--fit-rounds 2] [--passes 3] [--out profiles/mesh_data_bench.json]

  (1) The launch, HIP events, median and range of `--rounds` rounds after `--warmup`, on the two mesh sets of tools/bench_mesh_in.py
      (`--batch` surface-nets meshes of three-ellipsoid unions, about 3 k small triangles each; as many boxes of 12 large triangles):
      `pcd_mesh_batch_clouds` at N = `--num-points` without a chain, with normalize, with jitter + normalize (the module's default) and with
      all three, in the LDS-resident and in the regenerating form, and in the same rounds `pcd_mesh_sample_points` (its two launches), the
      yardstick profiles/mesh_in_bench.json recorded.
  (2) Shapes/s of each module's training loader iterated alone (tools/bench_device_data.py's protocol: one warm-up pass, then `--passes`
      passes, synchronised at the end of each), on `--shapes` ellipsoid-union meshes written as .obj files and on the cloud files
      `preprocess_meshes.py` makes from them.
  (3) Wall time per epoch of `training.fit` of the point denoiser with each module, `--fit-rounds` fits of `--epochs` epochs in alternating
      order, a fresh model per fit; the summary is the median and range of the epochs after each fit's first.
The host loader's worker count is 4; nothing here is sized by the machine's CPU count."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shapegen_amd  # noqa: E402,F401
from bench_device_data import fit_epochs, iterate, summarise  # noqa: E402
from bench_mesh import ellipsoid_grids, event_timed, summary  # noqa: E402
from bench_mesh_in import box_meshes  # noqa: E402
from shapegen_amd import _lib  # noqa: E402
from shapegen_amd.data import DeviceMeshDataModule, PointCloudDataDirectoryModule  # noqa: E402
from shapegen_amd.utils import _pack_meshes, save_mesh, voxel_tensor_to_meshes  # noqa: E402

CHAINS = {"no_chain": 0, "normalize": 1, "jitter_normalize": 5, "rotate_jitter_normalize": 7}


def bench_launch(meshes, n_points: int, rounds: int, warmup: int) -> dict:
    lib = _lib.load()
    b = len(meshes)
    verts, faces, offsets, rows = _pack_meshes(meshes, "bench")
    sums = torch.empty(rows[-1][1], dtype=torch.float32, device="cuda")
    sws = torch.empty(lib.pcd_mesh_sample_workspace_bytes(b, rows[-1][1]) // 4, dtype=torch.float32, device="cuda")
    index = torch.arange(b, dtype=torch.int32, device="cuda")
    pts = torch.empty(b, n_points, 3, dtype=torch.float32, device="cuda")
    stream = _lib.stream_ptr()
    _lib.check(lib.pcd_mesh_area_sums(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, sums.data_ptr(), stream), "mesh_area_sums")

    def batch(flags):
        _lib.check(lib.pcd_mesh_batch_clouds(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, sums.data_ptr(), index.data_ptr(), b,
                                             n_points, 24, 0, flags, 0.01, 0.05, pts.data_ptr(), None, None, stream), "mesh_batch_clouds")

    def sample():
        _lib.check(lib.pcd_mesh_sample_points(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, n_points, 24, 0, None, sws.data_ptr(),
                                              pts.data_ptr(), None, None, stream), "mesh_sample_points")

    def area_sums():
        _lib.check(lib.pcd_mesh_area_sums(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, sums.data_ptr(), stream), "mesh_area_sums")

    t = {f"{name}_{form}": [] for name in CHAINS for form in ("resident", "regenerating")}
    t["sampler_both_launches"], t["area_sums"] = [], []
    try:
        for k in range(warmup + rounds):
            row = {"sampler_both_launches": event_timed(sample), "area_sums": event_timed(area_sums)}
            for name, flags in CHAINS.items():
                for code, form in ((1, "resident"), (0, "regenerating")):
                    lib.pcd_mesh_data_config(code)
                    row[f"{name}_{form}"] = event_timed(lambda: batch(flags))
            if k >= warmup:
                for key, v in row.items():
                    t[key].append(v)
    finally:
        lib.pcd_mesh_data_config(1)
    return dict({k: summary(v) for k, v in t.items()}, meshes=b, triangles_total=rows[-1][1], num_points=n_points)


def write_meshes(root: str, count: int) -> int:
    """`count` surface-nets meshes of three-ellipsoid unions as .obj files; returns their triangle total."""
    triangles = 0
    for lo in range(0, count, 32):
        grids = ellipsoid_grids(min(32, count - lo), seed=24 + lo)
        for i, m in enumerate(voxel_tensor_to_meshes(grids, 0.5)):
            save_mesh(os.path.join(root, f"mesh_{lo + i:05d}.obj"), m)
            triangles += int(m.faces.shape[0])
    return triangles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shapes", type=int, default=512)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--fit-rounds", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_data_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_data.py measures on the GPU: no device is visible")
    import preprocess_meshes
    with torch.no_grad():
        nets = voxel_tensor_to_meshes(ellipsoid_grids(args.batch), 0.5)
        result = {"device": torch.cuda.get_device_name(0), "batch": args.batch,
                  "launch_order": "per round: the sampler's two launches, the area sums alone, then per chain the resident and the regenerating form",
                  "launch_surface_nets_ellipsoids": bench_launch(nets, args.num_points, args.rounds, args.warmup),
                  "launch_boxes_12_triangles": bench_launch(box_meshes(args.batch), args.num_points, args.rounds, args.warmup)}
    result.update({"shapes": args.shapes, "num_points": args.num_points, "batch_size": args.batch_size, "host_num_workers": 4})
    with tempfile.TemporaryDirectory() as root:
        src, grids, pts = (os.path.join(root, d) for d in ("meshes", "grids", "clouds"))
        os.makedirs(src)
        t0 = time.perf_counter()
        with torch.no_grad():
            result["triangles_total"] = write_meshes(src, args.shapes)
        result["write_meshes_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        with torch.no_grad():
            preprocess_meshes.main([src, grids, "--points-dir", pts, "--num-points", str(args.num_points)])
        torch.cuda.synchronize()
        result["preprocess_meshes_s"] = time.perf_counter() - t0
        args_fit = argparse.Namespace(num_points=args.num_points, epochs=args.epochs)

        def host():
            torch.manual_seed(24)
            dm = PointCloudDataDirectoryModule(pts, num_points=args.num_points, batch_size=args.batch_size, num_workers=4,
                                               file_mode="point_clouds", output_mode="point_clouds")
            dm.setup()
            return dm

        def device():
            torch.manual_seed(24)
            dm = DeviceMeshDataModule(src, num_points=args.num_points, batch_size=args.batch_size)
            t0 = time.perf_counter()
            dm.setup()
            torch.cuda.synchronize()
            result["device_setup_s"] = time.perf_counter() - t0
            return dm

        dm = device()
        result["table_bytes"] = int(dm.vertices.numel() * 4 + dm.faces.numel() * 4 + dm.offsets.numel() * 8 + dm.area_sums.numel() * 4)
        result["a_host_loader_alone"] = iterate(host(), args.passes)
        result["b_device_loader_alone"] = iterate(dm, args.passes)
        fits = {"host": [], "device": []}
        for _ in range(args.fit_rounds):                    # alternating, so that a drift of the box or the process hits both
            fits["host"].append(fit_epochs(host(), args_fit))
            fits["device"].append(fit_epochs(device(), args_fit))
        result["c_fit_order"] = "host, device" + ", host, device" * (args.fit_rounds - 1)
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
