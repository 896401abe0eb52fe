"""Pictures of saved shapes, rendered on the device (`utils.render_point_clouds`, `render_meshes`, `render_voxels`; DESIGN.md "Render").

    python render_shapes.py INPUT [INPUT ...] [--views N] [--elev 30] [--size 256] [--radius 1.5] [--grid COLS] [--threshold 0.5] [--arrays NAME ...]
                            [--out DIR]

Inputs by extension.  `.npz`: every array of it that is a batch of clouds (B, N, 3) or one cloud (N, 3) -- `generated=` as
`test_point_ddpm.py` writes it, `samples` of `generate_point_ddpm.py`, `sample_<i>` of `test_point_ldm.py` -- or of voxel grids (B, 1, D, H, W) /
(B, D, H, W) / (D, H, W), which are drawn as their surface-nets meshes at `--threshold`; other arrays, and the `metrics*` rows the scripts
store next to their shapes, are skipped (`--arrays NAME ...` picks arrays by name instead).  `.obj` / `.ply`: one mesh
(`utils.load_mesh`), normalised to the unit cube; a `.ply` that holds no faces (`utils.save_point_cloud`, `--ply-dir` of the generation
scripts) is drawn as the cloud it is, in its own coordinates like the clouds of an `.npz`.  Per shape one PNG `<input>_<array>_<i>.png` goes to `--out`: a turntable of `--views` views
at elevation `--elev`, side by side.  `--grid COLS` writes one contact sheet `<input>_<array>.png` per array instead, the first view of every
shape, COLS to a row.  No text and no axes in the pictures.  One process, one GPU.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

import shapegen_amd  # noqa: F401
from shapegen_amd import utils


def shapes_of(path: str, threshold: float, arrays=None):
    """-> list of (tag, kind, payload): kind "points" with a list of (n, 3) device tensors, "meshes" with a list of Mesh"""
    ext = os.path.splitext(path)[1].lower()
    if ext in (".obj", ".ply"):
        mesh = utils.load_mesh(path)
        if ext == ".ply" and mesh.faces.shape[0] == 0:
            return [("cloud", "points", [mesh.vertices.cuda()])]
        return [("mesh", "meshes", [utils.normalize_mesh(utils.Mesh(mesh.vertices.cuda(), mesh.faces.cuda()))])]
    if ext != ".npz":
        raise ValueError(f"render_shapes reads .npz, .obj or .ply, not {ext!r} ({path})")
    out = []
    with np.load(path) as z:
        for key in z.files:
            if (key not in arrays) if arrays else key.startswith("metrics"):
                continue
            a = z[key]
            if a.dtype.kind not in "fiub" or a.size == 0:
                continue
            if a.ndim in (2, 3) and a.shape[-1] == 3:
                clouds = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().reshape(-1, a.shape[-2], 3)
                out.append((key, "points", list(clouds)))
            elif a.ndim in (3, 4, 5) and a.shape[-1] == a.shape[-2] == a.shape[-3] and a.shape[-1] > 3 and (a.ndim < 5 or a.shape[1] == 1):
                grid = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().reshape(-1, 1, *a.shape[-3:])
                out.append((key, "meshes", utils.voxel_tensor_to_meshes(grid, threshold)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("inputs", nargs="+")
    ap.add_argument("--views", type=int, default=1, metavar="N", help="turntable views per shape")
    ap.add_argument("--elev", type=float, default=30.0)
    ap.add_argument("--size", type=int, default=256, help="height and width of one view in pixels")
    ap.add_argument("--radius", type=float, default=1.5, help="point radius in pixels")
    ap.add_argument("--grid", type=int, default=0, metavar="COLS", help="one contact sheet per array, COLS shapes to a row")
    ap.add_argument("--threshold", type=float, default=0.5, help="occupancy threshold of voxel inputs")
    ap.add_argument("--arrays", nargs="+", default=None, metavar="NAME", help="arrays of an .npz to draw (default: all that hold shapes)")
    ap.add_argument("--out", default=os.path.join("test", "visualizations"))
    args = ap.parse_args()
    views = utils.orbit_views(args.views, args.elev, args.size, args.size)
    written = 0
    for path in args.inputs:
        stem = os.path.splitext(os.path.basename(path))[0]
        for tag, kind, shapes in shapes_of(path, args.threshold, args.arrays):
            if kind == "points":
                images = utils.render_point_clouds(shapes, views, args.size, args.size, args.radius)
            else:
                images = utils.render_meshes(shapes, views, args.size, args.size)
            if args.grid > 0:
                utils.save_png(os.path.join(args.out, f"{stem}_{tag}.png"), utils.image_grid(images[:, 0], args.grid))
                written += 1
                continue
            for i in range(images.shape[0]):
                utils.save_png(os.path.join(args.out, f"{stem}_{tag}_{i}.png"), utils.image_grid(images[i], args.views))
                written += 1
    print(f"wrote {written} PNG file(s) to {args.out}")


if __name__ == "__main__":
    main()
