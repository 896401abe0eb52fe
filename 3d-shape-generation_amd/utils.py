"""Voxel <-> point conversions of the hot path (reference utils.py:488-539) and voxel -> mesh (surface nets, csrc/mesh.hip) on
HIP kernels, plus the small host helpers the entry points need (logger, mesh files)."""
from __future__ import annotations

import logging
import os
from typing import List, NamedTuple

import numpy as np
import torch

from . import _lib


def voxelize(points: torch.Tensor, voxel_resolution: int = 32) -> torch.Tensor:
    """utils.py:488-509: (B,N,3) in [-1,1] -> occupancy (B,R,R,R) indexed [x][y][z]."""
    if points.device.type != "cuda":
        raise RuntimeError("voxelize runs only on an MI355X device (no CPU path)")
    p = points.unsqueeze(0) if points.dim() == 2 else points
    p = p.to(torch.float32).contiguous()
    b, n, r = p.shape[0], p.shape[1], voxel_resolution
    vox = torch.empty(b, r, r, r, dtype=torch.float32, device=p.device)
    lib = _lib.load()
    _lib.check(lib.pcd_fill_zero(vox.data_ptr(), vox.numel() * 4, _lib.stream_ptr()), "fill_zero")
    _lib.check(lib.pcd_voxelize(p.data_ptr(), b, n, r, vox.data_ptr(), _lib.stream_ptr()), "voxelize")
    return vox


def voxel_tensor_to_point_clouds(voxel_grid: torch.Tensor, threshold: float = 0.5) -> List[torch.Tensor]:
    """utils.py:511-539: (B,1,D,H,W) -> python list of (n_i,3) clouds in [-1,1], points ordered by
    the row-major (z,y,x) scan of `torch.where`, columns [x,y,z].  Empty grids give (0,3)."""
    if voxel_grid.device.type != "cuda":
        raise RuntimeError("voxel_tensor_to_point_clouds runs only on an MI355X device (no CPU path)")
    b, _, d, h, w = voxel_grid.shape
    v = voxel_grid.to(torch.float32).contiguous()
    counts = torch.empty(b, dtype=torch.int32, device=v.device)
    pts = torch.empty(b, d * h * w, 3, dtype=torch.float32, device=v.device)
    _lib.check(_lib.load().pcd_voxels_to_points(v.data_ptr(), b, d, h, w, float(threshold), counts.data_ptr(),
                                                pts.data_ptr(), _lib.stream_ptr()), "voxels_to_points")
    cnt = counts.cpu().tolist()          # the ragged python list forces one host sync, as in the reference
    return [pts[i, :cnt[i]].clone() for i in range(b)]


class Mesh(NamedTuple):
    vertices: torch.Tensor      # (V, 3) float32, rows [x, y, z]
    faces: torch.Tensor         # (F, 3) int32, rows of `vertices`, counter-clockwise seen from outside


def voxel_tensor_to_meshes(voxel_grid: torch.Tensor, threshold: float = 0.5) -> List[Mesh]:
    """(B,1,D,H,W) -> python list of `Mesh`, one closed surface-nets mesh per grid (DESIGN.md "Mesh output"): a node is inside iff
    v > threshold, as in `voxel_tensor_to_point_clouds`, and vertices come out in that function's [-1,1] coordinates, so a grid's
    mesh and its point cloud overlay.  The field is zero-padded by one node, so a surface that reaches the grid's border closes
    up to one voxel pitch 2 / (n - 1) outside [-1,1] (half a pitch for a full grid at threshold 0.5).  Empty grids give (0,3) and
    (0,3).  The meshes are views of two packed device tensors; bitwise repeatable and independent of the rest of the batch."""
    if voxel_grid.device.type != "cuda":
        raise RuntimeError("voxel_tensor_to_meshes runs only on an MI355X device (no CPU path)")
    b, _, d, h, w = voxel_grid.shape
    v = voxel_grid.to(torch.float32).contiguous()
    lib = _lib.load()
    ws = torch.empty(max(lib.pcd_mesh_workspace_bytes(b, d, h, w), 4) // 4, dtype=torch.int32, device=v.device)
    counts = torch.empty(b, 2, dtype=torch.int32, device=v.device)
    _lib.check(lib.pcd_mesh_count(v.data_ptr(), b, d, h, w, float(threshold), ws.data_ptr(), counts.data_ptr(), _lib.stream_ptr()),
               "mesh_count")
    ends = torch.cumsum(counts, dim=0, dtype=torch.int64)
    offsets = (ends - counts).contiguous()
    cnt = counts.cpu().tolist()          # the packed outputs are sized on the host: one sync, as in voxel_tensor_to_point_clouds
    nv, nf = [c[0] for c in cnt], [c[1] for c in cnt]
    verts = torch.empty(sum(nv), 3, dtype=torch.float32, device=v.device)
    faces = torch.empty(sum(nf), 3, dtype=torch.int32, device=v.device)
    if sum(nv) > 0:
        _lib.check(lib.pcd_mesh_emit(v.data_ptr(), b, d, h, w, float(threshold), ws.data_ptr(), offsets.data_ptr(), verts.data_ptr(),
                                     faces.data_ptr(), _lib.stream_ptr()), "mesh_emit")
    return [Mesh(vs, fs) for vs, fs in zip(torch.split(verts, nv), torch.split(faces, nf))]


def _mesh_arrays(mesh):
    vertices, faces = mesh
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    return v, f


def mesh_is_closed(mesh) -> bool:
    """Host check: every directed edge of the triangles occurs as often as its reverse (closed and consistently oriented)."""
    v, f = _mesh_arrays(mesh)
    if f.shape[0] == 0:
        return True
    a = f[:, [0, 1, 2]].reshape(-1).astype(np.int64)
    b = f[:, [1, 2, 0]].reshape(-1).astype(np.int64)
    n = max(int(v.shape[0]), int(f.max()) + 1)
    return bool(np.array_equal(np.sort(a * n + b), np.sort(b * n + a)))


def save_mesh(path: str, mesh) -> None:
    """Write `mesh` = (vertices (V,3), faces (F,3)), CPU or device tensors, by the extension of `path`: `.obj` (text, `v x y z` lines with 9
    significant digits -- float32 round-trips -- and 1-based `f a b c` lines) or `.ply` (binary little-endian, `float x y z` and
    `list uchar int vertex_indices`).  Host only."""
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".obj", ".ply"):
        raise ValueError(f"save_mesh writes .obj or .ply, not {ext!r} ({path})")
    v, f = _mesh_arrays(mesh)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if ext == ".obj":
        with open(path, "w") as out:
            out.write(f"# {v.shape[0]} vertices, {f.shape[0]} triangles\n")
            out.writelines(f"v {float(x):.9g} {float(y):.9g} {float(z):.9g}\n" for x, y, z in v)
            out.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f.tolist())
        return
    rows = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rows["n"] = 3
    rows["idx"] = f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
        out.write(rows.tobytes())


def setup_logger(name: str, log_file: str, level=logging.INFO) -> logging.Logger:
    """File + console logger (reference utils.py:354-385 behaviour)."""
    os.makedirs(os.path.dirname(log_file) or ".", exist_ok=True)
    logger = logging.getLogger(name)
    logger.setLevel(level)
    if not logger.handlers:
        fmt = logging.Formatter("%(asctime)s - %(levelname)s - %(message)s")
        for h in (logging.FileHandler(log_file), logging.StreamHandler()):
            h.setFormatter(fmt)
            logger.addHandler(h)
    return logger
