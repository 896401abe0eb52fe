"""Mesh input on one GPU, one process, one session: the voxelizer under each fill and the surface sampler.

    python tools/bench_mesh_in.py [--batch 32] [--resolution 32] [--num-points 2048] [--rounds 100] [--warmup 10] [--out profiles/mesh_in_bench.json]

Inputs: the surface-nets meshes of `--batch` three-ellipsoid unions (`tools/bench_mesh.py`'s grids at threshold 0.5: about 3 k small triangles a
shape), and the same number of meshes of 12 large triangles each (boxes of random extents inside the cube).  For each set, after a warm-up of
every shape and alternating the measurements round by round:
  - `meshes_to_voxel_tensor` end to end on the host clock, synchronised, per fill (packing the list and uploading the offsets included);
  - its one launch with HIP events on a packed batch, per fill (`pcd_mesh_voxelize` is a single kernel: accumulate, resolve and write);
  - `sample_mesh_points` end to end, and `pcd_mesh_sample_points` with events at N = `--num-points` and at N = 1.  The entry point issues its
    two launches back to back; at N = 1 the point launch is one thread per mesh, so that figure is the area / running-sum launch with one empty
    launch behind it, and the difference to the full call is what the point launch adds.
Every figure is the median over the rounds with the range (min, max), in microseconds.  There is no earlier implementation to compare against."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shapegen_amd  # noqa: E402,F401
from bench_mesh import ellipsoid_grids, event_timed, host_timed, summary  # noqa: E402
from shapegen_amd import _lib  # noqa: E402
from shapegen_amd.utils import MESH_FILLS, Mesh, _pack_meshes, meshes_to_voxel_tensor, sample_mesh_points, voxel_tensor_to_meshes  # noqa: E402

BOX_FACES = [(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (2, 3, 7), (2, 7, 6), (1, 2, 6), (1, 6, 5), (0, 4, 7), (0, 7, 3)]


def box_meshes(batch: int, seed: int = 24):
    """Closed boxes of 12 triangles, half-extents 0.3 .. 0.9 round centres near the origin."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(batch):
        c, h = rng.uniform(-0.08, 0.08, 3), rng.uniform(0.3, 0.9, 3)
        lo, hi = c - h, c + h
        v = np.asarray([(lo[0], lo[1], lo[2]), (hi[0], lo[1], lo[2]), (hi[0], hi[1], lo[2]), (lo[0], hi[1], lo[2]),
                        (lo[0], lo[1], hi[2]), (hi[0], lo[1], hi[2]), (hi[0], hi[1], hi[2]), (lo[0], hi[1], hi[2])], np.float32)
        out.append(Mesh(torch.from_numpy(v).cuda(), torch.tensor(BOX_FACES, dtype=torch.int32).cuda()))
    return out


def bench_set(meshes, r: int, n_points: int, rounds: int, warmup: int) -> dict:
    lib = _lib.load()
    b = len(meshes)
    verts, faces, offsets, rows = _pack_meshes(meshes, "bench")
    ws = torch.empty(lib.pcd_mesh_voxelize_workspace_bytes(b, r) // 4, dtype=torch.int32, device="cuda")
    vox = torch.empty(b, 1, r, r, r, dtype=torch.float32, device="cuda")
    sws = torch.empty(lib.pcd_mesh_sample_workspace_bytes(b, rows[-1][1]) // 4, dtype=torch.float32, device="cuda")
    pts = torch.empty(b, n_points, 3, dtype=torch.float32, device="cuda")
    stream = _lib.stream_ptr()

    def launch(mode):
        _lib.check(lib.pcd_mesh_voxelize(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, r, -1.0, (r - 1) / 2.0, mode, ws.data_ptr(),
                                         vox.data_ptr(), stream), "mesh_voxelize")

    def sample(n):
        _lib.check(lib.pcd_mesh_sample_points(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, n, 24, 0, None, sws.data_ptr(), pts.data_ptr(),
                                              None, None, stream), "mesh_sample_points")

    t = {fill: {"end_to_end": [], "launch": []} for fill in MESH_FILLS}
    ts = {"end_to_end": [], "both_launches": [], "both_launches_one_point": []}
    occupied = {}
    for k in range(warmup + rounds):
        for fill, mode in MESH_FILLS.items():
            e2e, grid = host_timed(lambda: meshes_to_voxel_tensor(meshes, r, fill=fill))
            one = event_timed(lambda: launch(mode))
            occupied[fill] = int(grid.sum())
            if k >= warmup:
                t[fill]["end_to_end"].append(e2e)
                t[fill]["launch"].append(one)
        e2e, _ = host_timed(lambda: sample_mesh_points(meshes, n_points, seed=24))
        full, scan = event_timed(lambda: sample(n_points)), event_timed(lambda: sample(1))
        if k >= warmup:
            ts["end_to_end"].append(e2e)
            ts["both_launches"].append(full)
            ts["both_launches_one_point"].append(scan)
    return {"meshes": b, "vertices_total": rows[-1][0], "triangles_total": rows[-1][1], "resolution": r, "occupied_voxels_total": occupied,
            "voxelize": {fill: {k: summary(v) for k, v in t[fill].items()} for fill in MESH_FILLS},
            "sample": dict({k: summary(v) for k, v in ts.items()}, num_points=n_points)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--resolution", type=int, default=32)
    ap.add_argument("--num-points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_in_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_in.py measures on the GPU: no device is visible")
    torch.set_grad_enabled(False)
    nets = voxel_tensor_to_meshes(ellipsoid_grids(args.batch), 0.5)
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch,
              "order": "per round: surface, interior, solid (end to end, then the launch), sample (end to end, both launches, both launches at N = 1)",
              "surface_nets_ellipsoids": bench_set(nets, args.resolution, args.num_points, args.rounds, args.warmup),
              "boxes_12_triangles": bench_set(box_meshes(args.batch), args.resolution, args.num_points, args.rounds, args.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
