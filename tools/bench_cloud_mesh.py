"""Cloud to mesh on one GPU, one process, one session: every launch of `geometry.cloud_to_meshes` on preallocated buffers, the call end to end,
and in the same rounds `pcd_knn` at k = 8 and `voxel_tensor_to_meshes` on the same field, for scale.

    python tools/bench_cloud_mesh.py [--batch 64] [--num-points 2048] [--rounds 100] [--warmup 10] [--out profiles/cloud_mesh_bench.json]

Inputs: `--num-points` surface samples of each of `--batch` three-ellipsoid meshes (`tools/bench_mesh.py`'s grids at threshold 0.5, as
`tools/bench_geometry.py` uses them).  For R = 32 and R = 64, per round, in this order, with HIP events:
  - `knn_k8`: one `pcd_knn` call of every cloud against itself with exclude_self (the spacing's input);
  - `spacing`, `shell_fill`, `depth_field`: one `pcd_cloud_spacing`, `pcd_cloud_shell_fill`, `pcd_grid_depth_field` (two launches) call;
  - `mesh_count`, `mesh_emit`: the surface-nets calls on the field at threshold 1, the outputs sized once before the rounds;
  - `map_to_bounds`, `knn_vertices`, `project`: `pcd_project_to_cloud` without lists, `pcd_knn` of the vertices in their clouds at k = 8,
    `pcd_project_to_cloud` with the lists;
  - `cloud_to_meshes`: the Python call, events round the whole call (its allocations and its one host read included);
  - `voxel_tensor_to_meshes`: the Python call on the same field at threshold 1 (count, host read, emit).
Every figure is the median over the rounds with the range (min, max), in microseconds.  A first measurement: there is no earlier figure to
compare with."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shapegen_amd  # noqa: E402,F401
from bench_mesh import ellipsoid_grids, event_timed, summary  # noqa: E402
from shapegen_amd import _lib, geometry  # noqa: E402
from shapegen_amd.utils import sample_mesh_points, voxel_tensor_to_meshes  # noqa: E402

LO, HI, K = -1.25, 1.25, 8
NAMES = ["knn_k8", "spacing", "shell_fill", "depth_field", "mesh_count", "mesh_emit", "map_to_bounds", "knn_vertices", "project",
         "cloud_to_meshes", "voxel_tensor_to_meshes"]


def bench_resolution(lib, points, counts, R, rounds, warmup):
    P, N = points.shape[0], points.shape[1]
    h = (HI - LO) / (R - 1)
    dev, stream = points.device, _lib.stream_ptr()
    d2 = torch.empty(P, N, K, dtype=torch.float32, device=dev)
    index = torch.empty(P, N, K, dtype=torch.int32, device=dev)
    radii = torch.empty(P, dtype=torch.float32, device=dev)
    shell = torch.empty(P, R, R, dtype=torch.int64, device=dev)
    outside = torch.empty(P, R, R, dtype=torch.int64, device=dev)
    info = torch.empty(P, 3, dtype=torch.int32, device=dev)
    sweeps = torch.empty(P, dtype=torch.int32, device=dev)
    v = torch.empty(P, R, R, R, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.pcd_mesh_workspace_bytes(P, R, R, R) // 4, dtype=torch.int32, device=dev)
    sizes = torch.empty(P, 2, dtype=torch.int32, device=dev)

    def knn():
        _lib.check(lib.pcd_knn(points.data_ptr(), counts.data_ptr(), N, points.data_ptr(), counts.data_ptr(), N, P, K, 1, d2.data_ptr(),
                               index.data_ptr(), stream), "knn")

    def spacing():
        _lib.check(lib.pcd_cloud_spacing(d2.data_ptr(), counts.data_ptr(), N, P, K, None, 1.5, h, 0.0, radii.data_ptr(), stream), "cloud_spacing")

    def shell_fill():
        _lib.check(lib.pcd_cloud_shell_fill(points.data_ptr(), counts.data_ptr(), N, P, R, LO, h, radii.data_ptr(), shell.data_ptr(),
                                            outside.data_ptr(), info.data_ptr(), sweeps.data_ptr(), stream), "cloud_shell_fill")

    def depth_field():
        _lib.check(lib.pcd_grid_depth_field(outside.data_ptr(), P, R, h, radii.data_ptr(), 0.0, None, v.data_ptr(), stream), "grid_depth_field")

    def mesh_count():
        _lib.check(lib.pcd_mesh_count(v.data_ptr(), P, R, R, R, 1.0, ws.data_ptr(), sizes.data_ptr(), stream), "mesh_count")

    for fn in (knn, spacing, shell_fill, depth_field, mesh_count):            # the sizes of the outputs, once
        fn()
    host = sizes.cpu()
    vmax, faces_total = int(host[:, 0].max()), int(host[:, 1].sum())
    verts = torch.zeros(P, vmax, 3, dtype=torch.float32, device=dev)
    mapped, moved = torch.empty_like(verts), torch.empty_like(verts)
    faces = torch.empty(faces_total, 3, dtype=torch.int32, device=dev)
    vcnt = sizes[:, 0].contiguous()
    offsets = torch.stack([torch.arange(P, dtype=torch.int64, device=dev) * vmax,
                           torch.cumsum(sizes[:, 1], dim=0, dtype=torch.int64) - sizes[:, 1]], dim=1).contiguous()
    vd2 = torch.empty(P, vmax, K, dtype=torch.float32, device=dev)
    vindex = torch.empty(P, vmax, K, dtype=torch.int32, device=dev)

    def mesh_emit():
        _lib.check(lib.pcd_mesh_emit(v.data_ptr(), P, R, R, R, 1.0, ws.data_ptr(), offsets.data_ptr(), verts.data_ptr(), faces.data_ptr(), stream),
                   "mesh_emit")

    def map_to_bounds():
        _lib.check(lib.pcd_project_to_cloud(verts.data_ptr(), vcnt.data_ptr(), vmax, None, None, 0, P, None, 0, (HI - LO) / 2, (LO + HI) / 2,
                                            mapped.data_ptr(), stream), "project_to_cloud")

    def knn_vertices():
        _lib.check(lib.pcd_knn(mapped.data_ptr(), vcnt.data_ptr(), vmax, points.data_ptr(), counts.data_ptr(), N, P, K, 0, vd2.data_ptr(),
                               vindex.data_ptr(), stream), "knn")

    def project():
        _lib.check(lib.pcd_project_to_cloud(mapped.data_ptr(), vcnt.data_ptr(), vmax, points.data_ptr(), counts.data_ptr(), N, P, vindex.data_ptr(),
                                            K, 1.0, 0.0, moved.data_ptr(), stream), "project_to_cloud")

    steps = [knn, spacing, shell_fill, depth_field, mesh_count, mesh_emit, map_to_bounds, knn_vertices, project,
             lambda: geometry.cloud_to_meshes(points, resolution=R, bounds=(LO, HI)),
             lambda: voxel_tensor_to_meshes(v.view(P, 1, R, R, R), 1.0)]
    t = {name: [] for name in NAMES}
    for r in range(warmup + rounds):
        row = [event_timed(fn) for fn in steps]
        if r >= warmup:
            for name, us in zip(NAMES, row):
                t[name].append(us)
    meshes, out = geometry.cloud_to_meshes(points, resolution=R, bounds=(LO, HI), return_info=True)
    result = {"resolution": R, "pitch": h, "vertices": int(host[:, 0].sum()), "faces": faces_total, "max_vertices": vmax,
              "radius_mean": float(out["radius"].mean()), "enclosed_min": int(out["enclosed"].min()), "border_max": int(out["border"].max()),
              "fill_sweeps_max": int(sweeps.max()), "empty_meshes": sum(1 for m in meshes if m.faces.shape[0] == 0)}
    result.update({name: summary(us) for name, us in t.items()})
    result["launches_sum_us"] = sum(result[name]["median_us"] for name in NAMES[:9])
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--num-points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_mesh_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_mesh.py measures on the GPU: no device is visible")
    torch.set_grad_enabled(False)
    lib = _lib.load()
    P, N = args.batch, args.num_points
    points = sample_mesh_points(voxel_tensor_to_meshes(ellipsoid_grids(P), 0.5), N, seed=0)
    counts = torch.full((P,), N, dtype=torch.int32, device="cuda")
    result = {"device": torch.cuda.get_device_name(0), "clouds": P, "num_points": N, "bounds": [LO, HI], "k": K, "radius_scale": 1.5,
              "order": "per round: " + ", ".join(NAMES)}
    for R in (32, 64):
        result[f"R{R}"] = bench_resolution(lib, points, counts, R, args.rounds, args.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
