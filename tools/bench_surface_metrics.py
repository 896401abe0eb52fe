"""Surface metrics on one GPU, one process, one session: the index-carrying nearest-neighbour kernel, the reduction behind it and
`mesh_metrics` end to end, with the distance-only Chamfer kernel measured in the same rounds as the yardstick for what the index costs.

    python tools/bench_surface_metrics.py [--batch 32] [--num-points 10000] [--rounds 100] [--warmup 10] [--out profiles/surface_metrics_bench.json]

Inputs: the surface-nets meshes of `--batch` three-ellipsoid unions (`tools/bench_mesh.py`'s grids at threshold 0.5, as `tools/bench_mesh_in.py`
uses them), each compared with the next one of the batch, N = `--num-points` samples with normals a side.  Per round, in this order, with HIP
events on preallocated buffers unless said otherwise:
  - `nearest_both_directions`: two `pcd_nearest_neighbors` calls, a against b and b against a -- per call one memset of the keys, the
    nearest-neighbour launch and the small decode launch;
  - `surface_metrics_entry`: one `pcd_surface_metrics` call -- one memset, ONE nearest-neighbour launch for both directions, the reduction;
  - `reduction_by_difference`: the second minus the first in the same round, i.e. the reduction launch less one memset and two decode
    launches (it can come out near zero or negative: the one launch for both directions fills the chip better than two);
  - `pair_metrics_entry`: `pcd_pair_metrics` without Sinkhorn on the same clouds -- normalise, the distance-only Chamfer kernel (the same
    2 P N^2 distances), its sum, and the 32^3 voxel BCE;
  - `chamfer_per_sample`: the Python call around that entry point, events round the whole call (its small host-side tensors included);
  - `mesh_metrics`: end to end on the host clock, synchronised: sampling both sides, `surface_metrics`, both voxelizations, the IoU.
Every figure is the median over the rounds with the range (min, max), in microseconds; `ns_per_distance` divides the medians by 2 P N^2."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shapegen_amd  # noqa: E402,F401
from bench_mesh import ellipsoid_grids, event_timed, host_timed, summary  # noqa: E402
from shapegen_amd import _lib, metrics  # noqa: E402
from shapegen_amd.utils import sample_mesh_points, voxel_tensor_to_meshes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-points", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_metrics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_metrics.py measures on the GPU: no device is visible")
    torch.set_grad_enabled(False)
    lib = _lib.load()
    P, N = args.batch, args.num_points
    meshes_a = voxel_tensor_to_meshes(ellipsoid_grids(P), 0.5)
    meshes_b = meshes_a[1:] + meshes_a[:1]
    pa, na = sample_mesh_points(meshes_a, N, seed=0, return_normals=True)
    pb, nb = sample_mesh_points(meshes_b, N, seed=1, return_normals=True)
    counts = torch.full((P,), N, dtype=torch.int32, device="cuda")
    taus = (C.c_float * 3)(*metrics.DEFAULT_THRESHOLDS)
    rows = torch.empty(P, _lib.PCD_SURF_ROW_BASE + 9, dtype=torch.float32, device="cuda")
    d2 = torch.empty(P, N, dtype=torch.float32, device="cuda")
    index = torch.empty(P, N, dtype=torch.int32, device="cuda")
    need_nn, need_rows = lib.pcd_nearest_workspace_bytes(P, N, N), lib.pcd_surface_metrics_workspace_bytes(P, N, N)
    need_pair = lib.pcd_pair_metrics_workspace_bytes(P, N, N)
    ws = torch.empty(max(need_nn, need_rows, need_pair), dtype=torch.uint8, device="cuda")
    pair_rows = torch.empty(P, 3, dtype=torch.float32, device="cuda")
    log_mu = torch.log(torch.ones(P) / N + 1e-10).cuda()
    stream = _lib.stream_ptr()

    def nearest():
        for q, t in ((pa, pb), (pb, pa)):
            _lib.check(lib.pcd_nearest_neighbors(q.data_ptr(), counts.data_ptr(), N, t.data_ptr(), counts.data_ptr(), N, P, d2.data_ptr(),
                                                 index.data_ptr(), ws.data_ptr(), need_nn, stream), "nearest_neighbors")

    def surface():
        _lib.check(lib.pcd_surface_metrics(pa.data_ptr(), na.data_ptr(), counts.data_ptr(), N, pb.data_ptr(), nb.data_ptr(), counts.data_ptr(), N,
                                           P, taus, 3, rows.data_ptr(), None, None, None, None, ws.data_ptr(), need_rows, stream),
                   "surface_metrics")

    def pair():
        _lib.check(lib.pcd_pair_metrics(pa.data_ptr(), counts.data_ptr(), N, pb.data_ptr(), counts.data_ptr(), N, P, 0, 1e-2, 1e-5, 100,
                                        log_mu.data_ptr(), log_mu.data_ptr(), pair_rows.data_ptr(), ws.data_ptr(), need_pair, stream),
                   "pair_metrics")

    t = {k: [] for k in ("nearest_both_directions", "surface_metrics_entry", "reduction_by_difference", "pair_metrics_entry",
                         "chamfer_per_sample", "mesh_metrics")}
    for k in range(args.warmup + args.rounds):
        both, entry = event_timed(nearest), event_timed(surface)
        yard, call = event_timed(pair), event_timed(lambda: metrics.chamfer_per_sample(pa, pb))
        e2e, out = host_timed(lambda: metrics.mesh_metrics(meshes_a, meshes_b, num_points=N))
        if k >= args.warmup:
            for name, v in (("nearest_both_directions", both), ("surface_metrics_entry", entry), ("reduction_by_difference", entry - both),
                            ("pair_metrics_entry", yard), ("chamfer_per_sample", call), ("mesh_metrics", e2e)):
                t[name].append(v)
    result = {"device": torch.cuda.get_device_name(0), "pairs": P, "num_points": N, "distances_per_call": 2 * P * N * N,
              "triangles_total": int(sum(m.faces.shape[0] for m in meshes_a)),
              "order": "per round: " + ", ".join(t), "finite_rows": int(torch.isfinite(out).all(dim=1).sum())}
    result.update({name: summary(v) for name, v in t.items()})
    per = lambda name: result[name]["median_us"] * 1e3 / (2.0 * P * N * N)
    result["ns_per_distance"] = {"nearest_both_directions": per("nearest_both_directions"), "surface_metrics_entry": per("surface_metrics_entry"),
                                 "pair_metrics_entry": per("pair_metrics_entry")}
    result["index_over_distance_only"] = result["nearest_both_directions"]["median_us"] / result["pair_metrics_entry"]["median_us"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
