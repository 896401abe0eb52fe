"""Mesh extraction next to the point conversion, on one GPU, one process, one session.

    python tools/bench_mesh.py [--batch 32] [--threshold 0.4] [--rounds 100] [--warmup 10] [--out profiles/mesh_bench.json]

Inputs: `--batch` grids decoded by `VAE3DLarge.decode` from fixed latents (synthetic weights, as the tests' `latent_sd`), and, because
random weights need not decode to shape-like fields, the same number of three-ellipsoid unions (test_point_ldm.py's synthetic grids).  For each
input set and each form of the kernels (`pcd_mesh_config` 1: grid staged in LDS, 0: grid read through the vector cache), alternating the forms
round by round after a warm-up of every shape:
  - `voxel_tensor_to_meshes` end to end on the host clock, synchronised (it contains the one host read of the counts);
  - its two launches on their own with HIP events (`pcd_mesh_count`, `pcd_mesh_emit` on preallocated outputs);
  - `voxel_tensor_to_point_clouds` on the same grids, the same way: end to end, and its one launch with events.
Every figure is the median over the rounds with the range (min, max), in microseconds.  The two forms' outputs are compared bit for bit."""
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
from shapegen_amd import _lib, specs  # noqa: E402
from shapegen_amd.utils import voxel_tensor_to_meshes, voxel_tensor_to_point_clouds  # noqa: E402
from shapegen_amd.vae import VAE3DLarge  # noqa: E402


def decoded_grids(batch: int) -> torch.Tensor:
    vae = VAE3DLarge()
    sd = specs.synth_state_dict(specs.vae3d_large_spec(), seed=0, gain=1.3)
    vae.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    vae = vae.to("cuda").eval()
    z = torch.randn(batch, 256, generator=torch.Generator().manual_seed(24)).cuda()
    with torch.no_grad():
        return vae.decode(z).float().contiguous()


def ellipsoid_grids(batch: int, seed: int = 24) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    out = np.zeros((batch, 1, 32, 32, 32), np.float32)
    for i in range(batch):
        c, r = rng.uniform(8, 24, (3, 3)), rng.uniform(3, 9, (3, 3))
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


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def bench_set(grids: torch.Tensor, thr: float, rounds: int, warmup: int) -> dict:
    lib = _lib.load()
    b, _, d, h, w = grids.shape
    ws = torch.empty(lib.pcd_mesh_workspace_bytes(b, d, h, w) // 4, dtype=torch.int32, device="cuda")
    counts = torch.empty(b, 2, dtype=torch.int32, device="cuda")
    pcounts = torch.empty(b, dtype=torch.int32, device="cuda")
    pts = torch.empty(b, d * h * w, 3, dtype=torch.float32, device="cuda")
    stream = _lib.stream_ptr()

    def count():
        _lib.check(lib.pcd_mesh_count(grids.data_ptr(), b, d, h, w, thr, ws.data_ptr(), counts.data_ptr(), stream), "mesh_count")

    count()
    offsets = (torch.cumsum(counts, 0, dtype=torch.int64) - counts).contiguous()
    total = counts.sum(dim=0).tolist()
    verts = torch.empty(max(total[0], 1), 3, dtype=torch.float32, device="cuda")
    faces = torch.empty(max(total[1], 1), 3, dtype=torch.int32, device="cuda")

    def emit():
        _lib.check(lib.pcd_mesh_emit(grids.data_ptr(), b, d, h, w, thr, ws.data_ptr(), offsets.data_ptr(), verts.data_ptr(), faces.data_ptr(),
                                     stream), "mesh_emit")

    def points_launch():
        _lib.check(lib.pcd_voxels_to_points(grids.data_ptr(), b, d, h, w, thr, pcounts.data_ptr(), pts.data_ptr(), stream), "voxels_to_points")

    forms = {1: "lds_staged", 0: "global_reads"}
    t = {name: {"end_to_end": [], "count_launch": [], "emit_launch": []} for name in forms.values()}
    tp = {"end_to_end": [], "launch": []}
    meshes = {}
    try:
        for k in range(warmup + rounds):
            for code, name in forms.items():
                assert lib.pcd_mesh_config(code) == 0
                e2e, meshes[name] = host_timed(lambda: voxel_tensor_to_meshes(grids, thr))
                c, e = event_timed(count), (event_timed(emit) if total[0] else 0.0)
                if k >= warmup:
                    t[name]["end_to_end"].append(e2e)
                    t[name]["count_launch"].append(c)
                    t[name]["emit_launch"].append(e)
            e2e, clouds = host_timed(lambda: voxel_tensor_to_point_clouds(grids, thr))
            lp = event_timed(points_launch)
            if k >= warmup:
                tp["end_to_end"].append(e2e)
                tp["launch"].append(lp)
    finally:
        assert lib.pcd_mesh_config(1) == 0
    same = all(torch.equal(x.vertices, y.vertices) and torch.equal(x.faces, y.faces)
               for x, y in zip(meshes["lds_staged"], meshes["global_reads"]))
    return {"grids": list(grids.shape), "threshold": thr, "occupied_voxels_total": int((grids > thr).sum()),
            "vertices_total": total[0], "triangles_total": total[1], "points_total": int(sum(c.shape[0] for c in clouds)),
            "forms_bit_equal": bool(same),
            "mesh": {name: {k: summary(v) for k, v in t[name].items()} for name in forms.values()},
            "points": {k: summary(v) for k, v in tp.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=0.4)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py measures on the GPU: no device is visible")
    torch.set_grad_enabled(False)
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "order": "per round: lds_staged, global_reads, points",
              "decoded": bench_set(decoded_grids(args.batch), args.threshold, args.rounds, args.warmup),
              "ellipsoids": bench_set(ellipsoid_grids(args.batch), args.threshold, args.rounds, args.warmup)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
