"""The renderer on one GPU, one process, one session: point clouds and meshes, one view and eight, under each tile shape.

    python tools/bench_render.py [--batch 32] [--size 256] [--num-points 2048] [--radius 1.5] [--views 1 8] [--rounds 100] [--warmup 10]
                                 [--out profiles/render_bench.json]

Inputs: `--batch` clouds of `--num-points` points drawn from the unit ball; the surface-nets meshes of as many three-ellipsoid unions
(`tools/bench_mesh.py`'s grids at threshold 0.5: about 3 k small triangles a shape); and as many boxes of 12 large triangles
(`tools/bench_mesh_in.py`).  For each set, for each of the `--views` counts (V = 1 and V = 8) of turntable views at `--size` x `--size`, after a warm-up and alternating the
measurements round by round:
  - the one launch with HIP events on a packed batch (`pcd_render_points` / `pcd_render_meshes`, all three outputs written), under the
    128 x 64 tile, under the 128 x 128 tile and under the default, which picks between them by the size of the launch (`pcd_render_config`);
  - the Python call end to end on the host clock, synchronised, under the default tile (packing, the upload of offsets, views and colours and
    the allocation of the images included).
Every figure is the median over the rounds with the range (min, max), in microseconds.  There is no earlier implementation to compare against.
If matplotlib is importable, one Agg scatter per cloud on the host (savefig to memory) is timed for one round of the batch and labelled as
context: it is not the same picture and not a baseline."""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shapegen_amd  # noqa: E402,F401
from bench_mesh import ellipsoid_grids, event_timed, host_timed, summary  # noqa: E402
from bench_mesh_in import box_meshes  # noqa: E402
from shapegen_amd import _lib, utils  # noqa: E402

TILES = {"tile_128x64": 0, "tile_128x128": 1, "tile_default": 2}


def ball_clouds(batch: int, n: int, seed: int = 24):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(batch, n, 3, generator=g)
    r = torch.rand(batch, n, 1, generator=g) ** (1.0 / 3.0)
    return list((d / d.norm(dim=-1, keepdim=True) * r * 0.95).cuda())


def bench_set(kind: str, shapes, size: int, radius: float, n_views: int, rounds: int, warmup: int) -> dict:
    lib = _lib.load()
    b = len(shapes)
    views = utils.orbit_views(n_views, 30.0, size, size).cuda().contiguous()
    light = np.asarray(utils.DEFAULT_LIGHT) / np.linalg.norm(utils.DEFAULT_LIGHT)
    style = _lib.RenderStyle(None, (_lib.f32 * 3)(*light), 0.3, (_lib.f32 * 3)(1.0, 1.0, 1.0))
    rgb = torch.empty(b, n_views, size, size, 3, dtype=torch.uint8, device="cuda")
    ids = torch.empty(b, n_views, size, size, dtype=torch.int32, device="cuda")
    depth = torch.empty(b, n_views, size, size, dtype=torch.float32, device="cuda")
    stream = _lib.stream_ptr()
    if kind == "points":
        pts = torch.cat(shapes).contiguous()
        offsets = torch.tensor(np.cumsum([0] + [c.shape[0] for c in shapes]), dtype=torch.int64).cuda()
        prims = int(pts.shape[0])

        def launch():
            _lib.check(lib.pcd_render_points(pts.data_ptr(), offsets.data_ptr(), b, views.data_ptr(), 1, n_views, size, size, radius, style,
                                             ids.data_ptr(), depth.data_ptr(), rgb.data_ptr(), stream), "render_points")

        def call():
            return utils.render_point_clouds(shapes, views, size, size, radius)
    else:
        verts, faces, offsets, rows = utils._pack_meshes(shapes, "bench")
        prims = rows[-1][1]

        def launch():
            _lib.check(lib.pcd_render_meshes(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, views.data_ptr(), 1, n_views, size, size,
                                             style, ids.data_ptr(), depth.data_ptr(), rgb.data_ptr(), stream), "render_meshes")

        def call():
            return utils.render_meshes(shapes, views, size, size)

    t = {name: [] for name in TILES}
    e2e = []
    try:
        for k in range(warmup + rounds):
            for name, code in TILES.items():
                _lib.check(lib.pcd_render_config(code), "render_config")
                one = event_timed(launch)
                if k >= warmup:
                    t[name].append(one)
            _lib.check(lib.pcd_render_config(2), "render_config")
            us, _ = host_timed(call)
            if k >= warmup:
                e2e.append(us)
    finally:
        lib.pcd_render_config(2)
    covered = float((ids >= 0).float().mean())
    return {"shapes": b, "primitives_total": prims, "views": n_views, "size": size, "covered_share": covered,
            "launch": {name: summary(v) for name, v in t.items()}, "python_end_to_end_default_tile": summary(e2e)}


def matplotlib_context(clouds, size: int):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:
        return None
    host = [c.cpu().numpy() for c in clouds]
    us = []
    for c in host:
        t0 = time.perf_counter()
        fig = plt.figure(figsize=(size / 100.0, size / 100.0), dpi=100)
        ax = fig.add_subplot(111, projection="3d")
        ax.scatter(c[:, 0], c[:, 1], c[:, 2], s=1)
        fig.savefig(io.BytesIO(), format="png")
        plt.close(fig)
        us.append((time.perf_counter() - t0) * 1e6)
    return {"what": "CONTEXT ONLY: one matplotlib Agg 3-d scatter per cloud on the host, figure to PNG in memory; a different picture, not a baseline",
            "per_cloud": summary(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--num-points", type=int, default=2048)
    ap.add_argument("--radius", type=float, default=1.5)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py measures on the GPU: no device is visible")
    torch.set_grad_enabled(False)
    clouds = ball_clouds(args.batch, args.num_points)
    sets = {"clouds": ("points", clouds), "surface_nets_ellipsoids": ("meshes", utils.voxel_tensor_to_meshes(ellipsoid_grids(args.batch), 0.5)),
            "boxes_12_triangles": ("meshes", box_meshes(args.batch))}
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "radius_px": args.radius,
              "order": "per set and view count, per round: the launch under the 128 x 64 tile, the 128 x 128 tile and the default, then the Python call"}
    for name, (kind, shapes) in sets.items():
        for v in args.views:
            result[f"{name}_views_{v}"] = bench_set(kind, shapes, args.size, args.radius, v, args.rounds, args.warmup)
    context = matplotlib_context(clouds, args.size)
    if context is not None:
        result["matplotlib_context"] = context
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
