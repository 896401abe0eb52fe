"""Cloud geometry on one GPU, one process, one session: the k-nearest kernel at k = 8 / 16 / 32 with the index-carrying single-neighbour
kernel measured in the same rounds as the yardstick, the normals, mask and compaction launches, and the two Python calls end to end.

    python tools/bench_geometry.py [--batch 64] [--num-points 2048] [--rounds 100] [--warmup 10] [--out profiles/geometry_bench.json]

Inputs: `--num-points` surface samples of each of `--batch` three-ellipsoid meshes (`tools/bench_mesh.py`'s grids at threshold 0.5, as
`tools/bench_surface_metrics.py` uses them) -- the sampler's batch.  Per round, in this order, with HIP events on preallocated buffers
unless said otherwise:
  - `knn_k8`, `knn_k16`, `knn_k32`: one `pcd_knn` call of every cloud against itself with exclude_self (one launch, no workspace);
  - `nearest_self`: one `pcd_nearest_neighbors` call of the clouds against themselves -- the memset of the keys, the nearest-neighbour launch
    and the decode launch: the same P N^2 distances, one neighbour and its index kept;
  - `normals_k16`: one `pcd_cloud_normals` call (outward: the centroid launch and the normals launch) on the k = 16 lists;
  - `outlier_mask_k16`, `compact`: one `pcd_cloud_outlier_mask` call (statistical) on the k = 16 distances, one `pcd_cloud_compact` call;
  - `remove_outliers`, `estimate_normals`: the Python calls at k = 16, events round the whole call (their allocations included).
Every figure is the median over the rounds with the range (min, max), in microseconds; `ps_per_distance` divides the medians by P N^2 and
`knn_over_nearest` is the ratio of the medians to the yardstick's."""
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

KS = (8, 16, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--num-points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geometry.py measures on the GPU: no device is visible")
    torch.set_grad_enabled(False)
    lib = _lib.load()
    P, N = args.batch, args.num_points
    points = sample_mesh_points(voxel_tensor_to_meshes(ellipsoid_grids(P), 0.5), N, seed=0)
    counts = torch.full((P,), N, dtype=torch.int32, device="cuda")
    d2 = {k: torch.empty(P, N, k, dtype=torch.float32, device="cuda") for k in KS}
    index = {k: torch.empty(P, N, k, dtype=torch.int32, device="cuda") for k in KS}
    nn_d2 = torch.empty(P, N, dtype=torch.float32, device="cuda")
    nn_index = torch.empty(P, N, dtype=torch.int32, device="cuda")
    need_nn, need_normals = lib.pcd_nearest_workspace_bytes(P, N, N), lib.pcd_cloud_normals_workspace_bytes(P)
    ws = torch.empty(max(need_nn, need_normals), dtype=torch.uint8, device="cuda")
    normals = torch.empty(P, N, 3, dtype=torch.float32, device="cuda")
    curvature = torch.empty(P, N, dtype=torch.float32, device="cuda")
    mask = torch.empty(P, N, dtype=torch.uint8, device="cuda")
    dbar = torch.empty(P, N, dtype=torch.float32, device="cuda")
    points_out, normals_out = torch.empty_like(points), torch.empty_like(normals)
    kept = torch.empty(P, dtype=torch.int32, device="cuda")
    stream = _lib.stream_ptr()

    def knn(k):
        _lib.check(lib.pcd_knn(points.data_ptr(), counts.data_ptr(), N, points.data_ptr(), counts.data_ptr(), N, P, k, 1, d2[k].data_ptr(),
                               index[k].data_ptr(), stream), "knn")

    def nearest():
        _lib.check(lib.pcd_nearest_neighbors(points.data_ptr(), counts.data_ptr(), N, points.data_ptr(), counts.data_ptr(), N, P, nn_d2.data_ptr(),
                                             nn_index.data_ptr(), ws.data_ptr(), need_nn, stream), "nearest_neighbors")

    def normals_launch():
        _lib.check(lib.pcd_cloud_normals(points.data_ptr(), counts.data_ptr(), N, P, index[16].data_ptr(), 16, _lib.PCD_NORMALS_OUTWARD, None,
                                         normals.data_ptr(), curvature.data_ptr(), ws.data_ptr(), need_normals, stream), "cloud_normals")

    def mask_launch():
        _lib.check(lib.pcd_cloud_outlier_mask(d2[16].data_ptr(), counts.data_ptr(), N, P, 16, _lib.PCD_OUTLIER_STATISTICAL, 2.0, 0.0, 1,
                                              mask.data_ptr(), dbar.data_ptr(), stream), "cloud_outlier_mask")

    def compact_launch():
        _lib.check(lib.pcd_cloud_compact(points.data_ptr(), normals.data_ptr(), mask.data_ptr(), counts.data_ptr(), N, P, points_out.data_ptr(),
                                         normals_out.data_ptr(), kept.data_ptr(), stream), "cloud_compact")

    names = [f"knn_k{k}" for k in KS] + ["nearest_self", "normals_k16", "outlier_mask_k16", "compact", "remove_outliers", "estimate_normals"]
    t = {name: [] for name in names}
    for r in range(args.warmup + args.rounds):
        row = [event_timed(lambda k=k: knn(k)) for k in KS]
        row += [event_timed(nearest), event_timed(normals_launch), event_timed(mask_launch), event_timed(compact_launch)]
        row += [event_timed(lambda: geometry.remove_outliers(points, k=16)), event_timed(lambda: geometry.estimate_normals(points, k=16, orient="outward"))]
        if r >= args.warmup:
            for name, v in zip(names, row):
                t[name].append(v)
    result = {"device": torch.cuda.get_device_name(0), "clouds": P, "num_points": N, "distances_per_call": P * N * N,
              "order": "per round: " + ", ".join(names), "kept_points": int(kept.sum()),
              "unit_normals": int(((normals.double().norm(dim=2) - 1).abs() < 1e-6).sum())}
    result.update({name: summary(v) for name, v in t.items()})
    yard = result["nearest_self"]["median_us"]
    result["ps_per_distance"] = {name: result[name]["median_us"] * 1e6 / (float(P) * N * N) for name in names[:4]}
    result["knn_over_nearest"] = {name: result[name]["median_us"] / yard for name in names[:3]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
