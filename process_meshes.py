"""Mesh processing entry point: clean, smooth and measure triangle meshes on the device.

    python process_meshes.py IN OUT [--smooth N] [--lambda L] [--mu M] [--pin-boundary] [--keep-largest | --min-component-faces K]
                                    [--simplify-resolution R | --simplify-cell H | --target-faces N] [--placement quadric|mean]
                                    [--deduplicate] [--normals] [--format obj|ply] [--report FILE.json]

IN is an `.obj` / `.ply` file (`utils.load_mesh`) or a directory of them, one mesh per file stem (`.obj` before `.ply` where a stem has
both, as `evaluate_meshes.py` reads a directory); OUT is a file for a file and a directory for a directory, where every mesh is written
as `<stem>.<format>` (default: the input's format; a single OUT file is written by its own extension).  The steps run in a fixed order, each only where asked for: connected components
(`--keep-largest`, or `--min-component-faces K` to drop the components with fewer faces), then simplification by vertex clustering
(`mesh_ops.simplify_meshes`: `--simplify-resolution R` for an R^3 grid over each mesh's box, `--simplify-cell H` for cells of side H, or
`--target-faces N` for the finest grid a bisection finds that leaves at most N faces; `--placement` and `--deduplicate` as there), then `--smooth N` rounds of Taubin smoothing
(`--lambda`, `--mu`; `--mu 0` is plain Laplacian smoothing; `--pin-boundary` keeps boundary vertices), then `--normals`, the
area-weighted vertex normals, written with the mesh.  `--report` writes JSON: per stem `before` and `after`, the
`mesh_ops.mesh_measures` of the mesh as read and as written, and with simplification `resolution`, the grid resolution used.  One process, one GPU; all meshes go through each step as one batch.
"""
from __future__ import annotations

import argparse
import json
import os

import shapegen_amd  # noqa: F401
from evaluate_meshes import mesh_files               # stem -> file, of a file or a directory
from shapegen_amd import mesh_ops, utils


def measures_rows(meshes) -> list:
    """`mesh_measures` as one JSON-ready dict per mesh"""
    m = {k: v.cpu().tolist() for k, v in mesh_ops.mesh_measures(meshes).items()}
    return [{k: m[k][i] for k in m} for i in range(len(meshes))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("inp", metavar="IN", help="a mesh file, or a directory of mesh files")
    ap.add_argument("out", metavar="OUT", help="the file to write, or the directory for a directory")
    ap.add_argument("--smooth", type=int, default=0, metavar="N", help="rounds of Taubin smoothing")
    ap.add_argument("--lambda", dest="lam", type=float, default=0.5)
    ap.add_argument("--mu", type=float, default=-0.53)
    ap.add_argument("--pin-boundary", action="store_true")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--keep-largest", action="store_true")
    which.add_argument("--min-component-faces", type=int, default=None, metavar="K")
    mesh_ops.add_simplify_arguments(ap)
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--format", choices=("obj", "ply"), default=None)
    ap.add_argument("--report", default=None, metavar="FILE.json")
    args = ap.parse_args()
    files = mesh_files(args.inp)
    if not files:
        raise SystemExit(f"process_meshes: no mesh files in {args.inp}")
    stems = sorted(files)
    meshes = []
    for s in stems:
        mesh = utils.load_mesh(files[s])
        meshes.append(utils.Mesh(mesh.vertices.cuda(), mesh.faces.cuda()))
    before = measures_rows(meshes)
    info = {}
    done, normals = mesh_ops.process_meshes(meshes, keep_largest=args.keep_largest, min_faces=args.min_component_faces, smooth=args.smooth,
                                            lam=args.lam, mu=args.mu, pin_boundary=args.pin_boundary, normals=args.normals, info=info,
                                            **mesh_ops.simplify_keywords(args))
    after = measures_rows(done)
    resolutions = info["resolutions"].cpu().tolist() if "resolutions" in info else None
    for i, s in enumerate(stems):
        ext = "." + args.format if args.format else os.path.splitext(files[s])[1].lower()
        path = os.path.join(args.out, s + ext) if os.path.isdir(args.inp) else args.out
        utils.save_mesh(path, done[i], normals=None if normals is None else normals[i])
        print(f"{s}: {before[i]['vertices']} vertices, {before[i]['faces']} faces, {before[i]['components']} components -> "
              f"{after[i]['vertices']}, {after[i]['faces']}, {after[i]['components']}; closed {bool(after[i]['closed'])}"
              + (f"; grid {resolutions[i]}^3" if resolutions else "") + f" -> {path}")
    if args.report:
        os.makedirs(os.path.dirname(args.report) or ".", exist_ok=True)
        with open(args.report, "w") as out:
            json.dump({s: dict({"before": before[i], "after": after[i]}, **({"resolution": resolutions[i]} if resolutions else {}))
                       for i, s in enumerate(stems)}, out, indent=1)


if __name__ == "__main__":
    main()
