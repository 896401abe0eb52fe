"""Mesh processing next to mesh extraction, on one GPU, one process, one session.

    python tools/bench_mesh_ops.py [--rounds 100] [--warmup 10] [--out profiles/mesh_ops_bench.json]

Inputs: the surface-nets meshes of three-ellipsoid unions (tools/bench_mesh.py's synthetic grids), 32 of them at 32^3 and 64 at 64^3.  Per
size, round by round after a warm-up, each on the host clock, synchronised:
  - the adjacency build (`mesh_adjacency`);
  - 10 Taubin rounds on that adjacency (20 launches, one per step);
  - vertex normals on that adjacency;
  - components + keep + compaction (`remove_small_components(keep_largest=True)`, which builds its own adjacency and contains the one
    host read of the counts);
  - measures on that adjacency (components included);
  - `voxel_tensor_to_meshes` on the same grids, for scale.
Every figure is the median over the rounds with the range (min, max), in microseconds.  (profiles/mesh_ops_bench_lds_form.json is this
tool's output while the library still had an LDS-resident smoothing form, one workgroup per mesh for all steps: it lost to the per-step
form at both sizes and was removed.)"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import shapegen_amd  # noqa: E402,F401
from shapegen_amd import mesh_ops  # noqa: E402
from shapegen_amd.utils import voxel_tensor_to_meshes  # noqa: E402


def ellipsoid_grids(batch: int, n: int, seed: int = 24) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(n)] * 3, indexing="ij")
    out = np.zeros((batch, 1, n, n, n), np.float32)
    for i in range(batch):
        c, r = rng.uniform(8, 24, (3, 3)) * (n / 32.0), rng.uniform(3, 9, (3, 3)) * (n / 32.0)
        for j in range(3):
            out[i, 0][((zz - c[j, 0]) / r[j, 0]) ** 2 + ((yy - c[j, 1]) / r[j, 1]) ** 2 + ((xx - c[j, 2]) / r[j, 2]) ** 2 <= 1] = 1
    return torch.from_numpy(out).cuda()


def summary(us):
    a = np.asarray(us, np.float64)
    return {"median_us": float(np.median(a)), "min_us": float(a.min()), "max_us": float(a.max()), "rounds": int(a.size)}


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def bench_set(grids: torch.Tensor, thr: float, rounds: int, warmup: int) -> dict:
    meshes = voxel_tensor_to_meshes(grids, thr)
    adj = mesh_ops.mesh_adjacency(meshes)
    steps = {"adjacency": lambda: mesh_ops.mesh_adjacency(meshes),
             "smooth_10": lambda: mesh_ops.smooth_meshes(meshes, 10, adjacency=adj),
             "normals": lambda: mesh_ops.vertex_normals(meshes, adjacency=adj),
             "components_keep_compact": lambda: mesh_ops.remove_small_components(meshes, keep_largest=True),
             "measures": lambda: mesh_ops.mesh_measures(meshes, adjacency=adj),
             "voxel_tensor_to_meshes": lambda: voxel_tensor_to_meshes(grids, thr)}
    t = {name: [] for name in steps}
    for k in range(warmup + rounds):
        for name, fn in steps.items():
            us, _ = host_timed(fn)
            if k >= warmup:
                t[name].append(us)
    nv = [m.vertices.shape[0] for m in meshes]
    return {"grids": list(grids.shape), "threshold": thr, "vertices_total": int(sum(nv)), "vertices_max": int(max(nv)),
            "triangles_total": int(sum(m.faces.shape[0] for m in meshes)), "timings": {name: summary(v) for name, v in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threshold", type=float, default=0.4)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_ops_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_ops.py measures on the GPU: no device is visible")
    torch.set_grad_enabled(False)
    result = {"device": torch.cuda.get_device_name(0), "order": "per round: " + ", ".join(
                  ["adjacency", "smooth_10", "normals", "components_keep_compact", "measures", "voxel_tensor_to_meshes"]),
              "32x32^3": bench_set(ellipsoid_grids(32, 32), args.threshold, args.rounds, args.warmup),
              "64x64^3": bench_set(ellipsoid_grids(64, 64), args.threshold, args.rounds, args.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
