"""Mesh simplification next to the adjacency build and mesh extraction, on one GPU, one process, one session.

    python tools/bench_mesh_simplify.py [--rounds 100] [--warmup 10] [--out profiles/mesh_simplify_bench.json]

Inputs: tools/bench_mesh_ops.py's, the surface-nets meshes of three-ellipsoid unions, 32 of them at 32^3 and 64 at 64^3.  Per size,
round by round after a warm-up, each on the host clock, synchronised:
  - `simplify_meshes` at resolution 16 and 32, quadric and mean placement (each contains the one host read of the counts);
  - `simplify_meshes(target_faces=...)` at a quarter of each mesh's faces (ten bisection rounds on the device, then the same);
  - the launches of the resolution-16 quadric run on their own: `pcd_mesh_simplify_count` and `pcd_mesh_simplify_emit` on buffers made
    once, without the host read between them;
  - `mesh_adjacency` and `voxel_tensor_to_meshes` on the same meshes and grids, for scale.
Every figure is the median over the rounds with the range (min, max), in microseconds; the face counts out are recorded with them."""
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
from bench_mesh_ops import ellipsoid_grids, host_timed, summary  # noqa: E402
from shapegen_amd import _lib, mesh_ops  # noqa: E402
from shapegen_amd.utils import voxel_tensor_to_meshes  # noqa: E402


def launches_only(meshes, resolution: int):
    """-> a function that runs the count and emit launches of a resolution run on buffers made here"""
    lib = _lib.load()
    out = mesh_ops.simplify_meshes(meshes, resolution=resolution)
    p, _ = mesh_ops._pack(meshes, "bench_mesh_simplify")
    b, (tv, tf), dev = p.batch, p.totals, p.verts.device
    nbytes = lib.pcd_mesh_simplify_workspace_bytes(b, tv, tf)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
    params = torch.full((b,), resolution, dtype=torch.int32, device=dev)
    res, vmap, counts = (torch.empty(n, dtype=torch.int32, device=dev) for n in (b, tv + 1, 2 * b))
    sizes = torch.tensor([[m.vertices.shape[0], m.faces.shape[0]] for m in out], dtype=torch.int64)
    offsets = (torch.cumsum(sizes, 0) - sizes).to(dev)
    verts = torch.empty(int(sizes[:, 0].sum()) + 1, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(int(sizes[:, 1].sum()) + 1, 3, dtype=torch.int32, device=dev)
    ptrs, dims = (p.verts.data_ptr(), p.faces.data_ptr(), p.offsets.data_ptr()), (b, tv, tf, p.max_vertices)

    def run():
        _lib.check(lib.pcd_mesh_simplify_count(*ptrs, *dims, mesh_ops.SIMPLIFY_RESOLUTION, params.data_ptr(), 0, ws.data_ptr(), nbytes,
                                               res.data_ptr(), vmap.data_ptr(), counts.data_ptr(), _lib.stream_ptr()), "count")
        _lib.check(lib.pcd_mesh_simplify_emit(*ptrs, *dims, mesh_ops.PLACEMENTS["quadric"], ws.data_ptr(), nbytes, offsets.data_ptr(),
                                              verts.data_ptr(), faces.data_ptr(), _lib.stream_ptr()), "emit")
        return p                                                             # keeps the packed inputs alive
    return run


def bench_set(grids: torch.Tensor, thr: float, rounds: int, warmup: int) -> dict:
    meshes = voxel_tensor_to_meshes(grids, thr)
    quarter = [m.faces.shape[0] // 4 for m in meshes]
    steps = {"simplify_r16_quadric": lambda: mesh_ops.simplify_meshes(meshes, resolution=16),
             "simplify_r16_mean": lambda: mesh_ops.simplify_meshes(meshes, resolution=16, placement="mean"),
             "simplify_r32_quadric": lambda: mesh_ops.simplify_meshes(meshes, resolution=32),
             "simplify_r32_mean": lambda: mesh_ops.simplify_meshes(meshes, resolution=32, placement="mean"),
             "simplify_target_quarter": lambda: mesh_ops.simplify_meshes(meshes, target_faces=quarter),
             "launches_r16_quadric": launches_only(meshes, 16),
             "adjacency": lambda: mesh_ops.mesh_adjacency(meshes),
             "voxel_tensor_to_meshes": lambda: voxel_tensor_to_meshes(grids, thr)}
    t = {name: [] for name in steps}
    faces_out = {}
    for k in range(warmup + rounds):
        for name, fn in steps.items():
            us, out = host_timed(fn)
            if k >= warmup:
                t[name].append(us)
            if k == 0 and name.startswith("simplify_"):
                faces_out[name] = int(sum(m.faces.shape[0] for m in out))
    nv = [m.vertices.shape[0] for m in meshes]
    return {"grids": list(grids.shape), "threshold": thr, "vertices_total": int(sum(nv)), "vertices_max": int(max(nv)),
            "triangles_total": int(sum(m.faces.shape[0] for m in meshes)), "triangles_out": faces_out,
            "timings": {name: summary(v) for name, v in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threshold", type=float, default=0.4)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_simplify.py measures on the GPU: no device is visible")
    torch.set_grad_enabled(False)
    result = {"device": torch.cuda.get_device_name(0),
              "order": "per round: simplify r16 quadric, r16 mean, r32 quadric, r32 mean, target quarter, launches r16 quadric, adjacency, "
                       "voxel_tensor_to_meshes",
              "32x32^3": bench_set(ellipsoid_grids(32, 32), args.threshold, args.rounds, args.warmup),
              "64x64^3": bench_set(ellipsoid_grids(64, 64), args.threshold, args.rounds, args.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
