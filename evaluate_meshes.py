"""Score meshes against reference meshes on the device (`metrics.mesh_metrics`; DESIGN.md "Surface metrics").

    python evaluate_meshes.py GEN REF [--num-points 10000] [--thresholds 0.02 0.04 0.1] [--resolution 32] [--fill solid] [--normalize] [--seed 0]
                              [--batch 32] [--out FILE.json]

GEN and REF are two `.obj` / `.ply` files (`utils.load_mesh`), or two directories whose mesh files are paired by file stem; a stem found on
one side only is listed and skipped.  The meshes are scored in their own coordinates -- `--normalize` first centres each on its bounding box
and scales its largest half-extent to 1 (`utils.normalize_mesh`), both sides alike.  Per pair: accuracy, completeness, Chamfer-L1 / -L2,
Hausdorff, normal consistency and precision / recall / F-score at `--thresholds` on `--num-points` surface samples a side, and the IoU of the
`--fill` voxelizations at `--resolution` (0: no IoU) over [-1, 1]^3.  A pair with a mesh without faces has no metrics (NaN).  Printed: one
line per column, the mean over the pairs that have the metric and how many have not.  `--out` writes JSON: `columns`, `stems`, `rows` (one per
pair, NaN as null), `mean`, `unpaired`.  One process, one GPU.
"""
from __future__ import annotations

import argparse
import json
import math
import os

import torch

import shapegen_amd  # noqa: F401
from shapegen_amd import metrics, utils

MESH_EXTENSIONS = (".obj", ".ply")


def mesh_files(path: str) -> dict:
    """stem -> file of a mesh file, or of every mesh file of a directory (`.obj` before `.ply` where a stem has both)"""
    if os.path.isdir(path):
        found = {}
        for name in sorted(os.listdir(path)):
            stem, ext = os.path.splitext(name)
            if ext.lower() in MESH_EXTENSIONS and stem not in found:
                found[stem] = os.path.join(path, name)
        return found
    if os.path.splitext(path)[1].lower() not in MESH_EXTENSIONS:
        raise ValueError(f"evaluate_meshes reads .obj or .ply files or directories of them, not {path!r}")
    return {os.path.splitext(os.path.basename(path))[0]: path}


def pair_up(gen: str, ref: str):
    """-> [(stem, generated file, reference file)], [unpaired stems]; two single files are a pair whatever their names"""
    g, r = mesh_files(gen), mesh_files(ref)
    if not os.path.isdir(gen) and not os.path.isdir(ref):
        (stem, gf), (_, rf) = next(iter(g.items())), next(iter(r.items()))
        return [(stem, gf, rf)], []
    if os.path.isdir(gen) != os.path.isdir(ref):
        raise ValueError("GEN and REF must be two files or two directories")
    return [(s, g[s], r[s]) for s in sorted(g) if s in r], sorted(set(g) ^ set(r))


def load(path: str, normalize: bool):
    mesh = utils.load_mesh(path)
    mesh = utils.Mesh(mesh.vertices.cuda(), mesh.faces.cuda())
    return utils.normalize_mesh(mesh) if normalize else mesh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("gen", metavar="GEN", help="a generated mesh file, or a directory of them")
    ap.add_argument("ref", metavar="REF", help="the reference mesh file, or a directory paired with GEN by file stem")
    ap.add_argument("--num-points", type=int, default=10000, help="surface samples per mesh")
    ap.add_argument("--thresholds", type=float, nargs="*", default=list(metrics.DEFAULT_THRESHOLDS), metavar="T", help="F-score distances")
    ap.add_argument("--resolution", type=int, default=32, help="voxel resolution of the IoU (0: no IoU)")
    ap.add_argument("--fill", default="solid", choices=sorted(utils.MESH_FILLS))
    ap.add_argument("--normalize", action="store_true", help="normalise every mesh to the [-1, 1] cube first")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=32, help="pairs per call")
    ap.add_argument("--out", default=None, metavar="FILE.json")
    args = ap.parse_args()
    if args.batch < 1:
        ap.error("--batch must be positive")
    torch.set_grad_enabled(False)
    pairs, unpaired = pair_up(args.gen, args.ref)
    for stem in unpaired:
        print(f"unpaired, skipped: {stem}")
    if not pairs:
        raise SystemExit("evaluate_meshes: no pairs to score")
    columns = metrics.mesh_columns(args.thresholds)
    rows = []
    for at in range(0, len(pairs), args.batch):
        chunk = pairs[at:at + args.batch]
        out = metrics.mesh_metrics([load(g, args.normalize) for _, g, _ in chunk], [load(r, args.normalize) for _, _, r in chunk],
                                   num_points=args.num_points, thresholds=args.thresholds, seed=args.seed,
                                   iou_resolution=args.resolution if args.resolution > 0 else None, iou_fill=args.fill)
        rows += out.cpu().tolist()
    mean = []
    print(f"{len(pairs)} pair(s), {args.num_points} points a side")
    for c, name in enumerate(columns):
        finite = [row[c] for row in rows if math.isfinite(row[c])]
        mean.append(sum(finite) / len(finite) if finite else None)
        shown = f"{mean[-1]:.6g}" if finite else "nan"
        print(f"{name:<16} {shown:<14} ({len(rows) - len(finite)} of {len(rows)} NaN)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        clean = [[v if math.isfinite(v) else None for v in row] for row in rows]
        with open(args.out, "w") as f:
            json.dump({"columns": columns, "stems": [s for s, _, _ in pairs], "rows": clean, "mean": mean, "unpaired": unpaired,
                       "num_points": args.num_points, "thresholds": list(args.thresholds), "resolution": args.resolution, "fill": args.fill,
                       "normalize": bool(args.normalize), "seed": args.seed}, f, indent=1)
        print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
