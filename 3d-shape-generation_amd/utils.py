"""Voxel <-> point conversions of the hot path (reference utils.py:488-539), voxel -> mesh (surface nets, csrc/mesh.hip) and mesh -> voxel /
mesh -> points (csrc/mesh_in.hip) on HIP kernels, plus the small host helpers the entry points need (logger, mesh files)."""
from __future__ import annotations

import logging
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

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


# ------------------------------------------------------------------ mesh files in
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_PLY_COUNT_TYPES = ("u1", "i1", "u2", "i2", "i4", "u4")          # uchar, char, ushort, short, int, uint
_PLY_ITEM_TYPES = ("i4", "u4", "i2", "u2")                       # int, uint, short, ushort


def _fan(corners: Sequence[int], faces: list) -> None:
    for i in range(1, len(corners) - 1):
        faces.append((corners[0], corners[i], corners[i + 1]))


def _load_obj(path: str) -> Tuple[np.ndarray, np.ndarray]:
    verts, faces = [], []
    with open(path, "r") as src:
        for number, line in enumerate(src, 1):
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{number}: a vertex line with fewer than 3 coordinates")
                try:
                    verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
                except ValueError:
                    raise ValueError(f"{path}:{number}: a vertex coordinate is not a number") from None
            elif tok[0] == "f":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{number}: a face with fewer than 3 corners")
                corners = []
                for t in tok[1:]:
                    try:
                        i = int(t.split("/")[0])
                    except ValueError:
                        raise ValueError(f"{path}:{number}: face token {t!r} does not start with a vertex index") from None
                    i = i - 1 if i > 0 else len(verts) + i          # 1-based; negative: relative to the vertices read so far
                    if i < 0 or i >= len(verts):
                        raise ValueError(f"{path}:{number}: vertex index {t.split('/')[0]} is out of range ({len(verts)} vertices so far)")
                    corners.append(i)
                _fan(corners, faces)
    return np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)


def _load_ply(path: str) -> Tuple[np.ndarray, np.ndarray]:
    with open(path, "rb") as src:
        raw = src.read()
    end = raw.find(b"end_header")
    nl = raw.find(b"\n", end)
    if not raw.startswith(b"ply") or end < 0 or nl < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' ... 'end_header')")
    fmt, elements = None, []                                     # elements: [name, count, [(kind, name, type...)]]
    for line in raw[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property" and elements:
            try:
                if tok[1] == "list":
                    elements[-1][2].append(("list", tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
                else:
                    elements[-1][2].append(("scalar", tok[2], _PLY_TYPES[tok[1]]))
            except KeyError as e:
                raise ValueError(f"{path}: unknown property type {e.args[0]!r}") from None
    if fmt == "binary_big_endian":
        raise ValueError(f"{path}: binary_big_endian PLY files are not read (ascii and binary_little_endian are)")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: unknown PLY format {fmt!r}")
    names = [e[0] for e in elements]
    if names[:1] != ["vertex"] or (len(names) > 1 and names[1] != "face"):
        raise ValueError(f"{path}: expected the elements 'vertex' then 'face', found {names}")
    _, nv, vprops = elements[0]
    if any(p[0] == "list" for p in vprops):
        raise ValueError(f"{path}: a list property on the vertex element")
    vtypes = {p[1]: p[2] for p in vprops}
    for axis in "xyz":
        if vtypes.get(axis) not in ("f4", "f8"):
            raise ValueError(f"{path}: vertex property {axis!r} must be float or double")
    nf, fprops = (elements[1][1], elements[1][2]) if len(elements) > 1 else (0, [])
    if len(elements) > 1:
        if len(fprops) != 1 or fprops[0][0] != "list" or fprops[0][1] not in ("vertex_indices", "vertex_index"):
            raise ValueError(f"{path}: the face element must carry exactly one list property vertex_indices / vertex_index "
                             f"(additional face properties are not read)")
        if fprops[0][2] not in _PLY_COUNT_TYPES or fprops[0][3] not in _PLY_ITEM_TYPES:
            raise ValueError(f"{path}: unsupported vertex_indices list types")
    body = raw[nl + 1:]
    faces: list = []
    try:
        if fmt == "ascii":
            lines = body.decode("ascii", "replace").split("\n")
            cols = [p[1] for p in vprops]
            ix = [cols.index(a) for a in "xyz"]
            rows = [lines[i].split() for i in range(nv)]
            verts = np.asarray([[float(r[k]) for k in ix] for r in rows], np.float64).reshape(-1, 3)
            polys = [[int(t) for t in lines[nv + i].split()] for i in range(nf)]
            polys = [(p[0], p[1:1 + p[0]]) if p else (0, []) for p in polys]
        else:
            vdt = np.dtype([(p[1], "<" + p[2]) for p in vprops])
            if len(body) < nv * vdt.itemsize:
                raise ValueError(f"{path}: the file ends inside the vertex element")
            table = np.frombuffer(body, dtype=vdt, count=nv)
            verts = np.stack([table[a].astype(np.float64) for a in "xyz"], axis=1).reshape(-1, 3)
            polys, at = [], nv * vdt.itemsize
            if nf:
                cdt, idt = np.dtype("<" + fprops[0][2]), np.dtype("<" + fprops[0][3])
                tri = np.dtype([("n", cdt), ("i", idt, (3,))])           # the common case, all triangles: one view
                if len(body) - at >= nf * tri.itemsize and bool((np.frombuffer(body, tri, nf, at)["n"] == 3).all()):
                    polys = [(3, row) for row in np.frombuffer(body, tri, nf, at)["i"].astype(np.int64).tolist()]
                else:
                    for _ in range(nf):
                        n = int(np.frombuffer(body, cdt, 1, at)[0])
                        at += cdt.itemsize
                        if n < 0:
                            raise ValueError(f"{path}: a negative list count")
                        polys.append((n, np.frombuffer(body, idt, n, at).astype(np.int64).tolist()))
                        at += n * idt.itemsize
    except (IndexError, ValueError) as e:
        if str(e).startswith(path):
            raise
        raise ValueError(f"{path}: the file ends early or a row is malformed ({e})") from None
    for n, corners in polys:
        if n < 3 or len(corners) != n:
            raise ValueError(f"{path}: a face with fewer than 3 corners (or a short row)")
        if min(corners) < 0 or max(corners) >= nv:
            raise ValueError(f"{path}: a vertex index is out of range ({nv} vertices)")
        _fan(corners, faces)
    return verts, np.asarray(faces, np.int64).reshape(-1, 3)


def load_mesh(path: str) -> Mesh:
    """Read a triangle mesh by the extension of `path`, the two formats `save_mesh` writes; host only, CPU tensors (`.to("cuda")` on the
    fields is the caller's job).  `.obj`: `v x y z [w]` and `f` lines with `i`, `i/t`, `i//n` or `i/t/n` tokens, 1-based, negative indices
    relative to the vertices read so far; every other line type is ignored.  `.ply`: `ascii` or `binary_little_endian`, element `vertex` with
    `float` / `double` `x y z` (other scalar properties skipped), then element `face` with the one list property `vertex_indices` /
    `vertex_index`; later elements are left unread.  Polygons are fan-triangulated as (c0, ci, ci+1).  `ValueError`, naming the file, for an
    out-of-range index, a face with fewer than 3 corners, an unknown extension, a big-endian PLY or a face element with further properties."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        v, f = _load_obj(path)
    elif ext == ".ply":
        v, f = _load_ply(path)
    else:
        raise ValueError(f"load_mesh reads .obj or .ply, not {ext!r} ({path})")
    return Mesh(torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f.astype(np.int32)))


def normalize_mesh(mesh, margin: float = 0.0) -> Mesh:
    """Centre the bounding box of `mesh` on the origin and scale its largest half-extent to 1 - margin (fp32, on the tensors' device); a mesh
    without extent (or without vertices) is only centred.  What `preprocess_meshes.py` does before it voxelizes."""
    v, f = mesh
    v = v.to(torch.float32)
    if v.shape[0] == 0:
        return Mesh(v, f)
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    half = float(((hi - lo) * 0.5).max())
    v = v - (lo + hi) * 0.5
    return Mesh(v * ((1.0 - float(margin)) / half) if half > 0.0 else v, f)


# ------------------------------------------------------------------ meshes -> grids, meshes -> clouds (csrc/mesh_in.hip)
MESH_FILLS = {"surface": 0, "interior": 1, "solid": 2}           # include/pcd_hip.h PCD_MESH_FILL_*


def _pack_meshes(meshes, what: str):
    """-> vertices fp32 [sum V][3], faces int32 [sum F][3], offsets int64 [B + 1][2] on the meshes' device (the packing of pcd_mesh_emit)."""
    meshes = list(meshes)
    if not meshes:
        raise ValueError(f"{what}: no meshes")
    vs, fs, rows = [], [], [(0, 0)]
    for i, m in enumerate(meshes):
        v, f = m
        if v.device.type != "cuda" or f.device.type != "cuda":
            raise RuntimeError(f"{what} runs only on an MI355X device (no CPU path)")
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError(f"{what}: mesh {i} is not (V, 3) vertices and (F, 3) faces")
        vs.append(v.to(torch.float32))
        fs.append(f.to(torch.int32))
        rows.append((rows[-1][0] + v.shape[0], rows[-1][1] + f.shape[0]))
    dev = vs[0].device
    verts = torch.cat(vs).contiguous() if rows[-1][0] else torch.zeros(1, 3, dtype=torch.float32, device=dev)
    faces = torch.cat(fs).contiguous() if rows[-1][1] else torch.zeros(1, 3, dtype=torch.int32, device=dev)
    offsets = torch.tensor(rows, dtype=torch.int64).to(dev, non_blocking=True)
    return verts, faces, offsets, rows


def meshes_to_voxel_tensor(meshes, resolution: int = 32, fill: str = "solid", bounds=(-1.0, 1.0)) -> torch.Tensor:
    """List of `Mesh` / (vertices, faces) pairs on the device -> (B, 1, R, R, R) float32 occupancy indexed [z][y][x], the inverse of
    `voxel_tensor_to_meshes` (DESIGN.md "Mesh input"): node i of an axis sits at lo + i (hi - lo) / (R - 1), for the default bounds the
    2 i / (R - 1) - 1 map of the other conversions.  `fill`: "surface" (nodes whose unit cube a triangle touches), "interior" (nonzero
    winding number, decided exactly at the node) or "solid" (their union).  Integer atomics only: bitwise repeatable and independent of
    the rest of the batch; no host synchronisation.  A mesh without faces gives an empty grid."""
    if fill not in MESH_FILLS:
        raise ValueError(f"fill must be one of {sorted(MESH_FILLS)}, got {fill!r}")
    lo, hi = float(bounds[0]), float(bounds[1])
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        raise ValueError(f"bounds must be finite with hi > lo, got {bounds!r}")
    r = int(resolution)
    if r != resolution or r < 2 or r > 64:
        raise ValueError(f"resolution must be an integer in 2..64, got {resolution!r}")
    verts, faces, offsets, rows = _pack_meshes(meshes, "meshes_to_voxel_tensor")
    b = len(rows) - 1
    lib = _lib.load()
    ws = torch.empty(max(lib.pcd_mesh_voxelize_workspace_bytes(b, r), 4) // 4, dtype=torch.int32, device=verts.device)
    vox = torch.empty(b, 1, r, r, r, dtype=torch.float32, device=verts.device)
    _lib.check(lib.pcd_mesh_voxelize(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, r, lo, (r - 1) / (hi - lo), MESH_FILLS[fill],
                                     ws.data_ptr(), vox.data_ptr(), _lib.stream_ptr()), "mesh_voxelize")
    return vox


def sample_mesh_points(meshes, num_points: int, seed: Optional[int] = None, return_normals: bool = False, return_faces: bool = False,
                       uniforms: Optional[torch.Tensor] = None):
    """List of `Mesh` / (vertices, faces) pairs on the device -> (B, num_points, 3) float32 points drawn uniformly by area from each surface,
    in the vertices' coordinates; with `return_normals` also the (B, num_points, 3) unit face normals (zero on a zero-area face), with
    `return_faces` the (B, num_points) int32 face rows, in that order.  The draws are Philox streams under `seed` (None: a seed from the
    global torch generator, as `DeviceVoxelDataModule` draws its keys); point i of every mesh uses counter i, so a mesh gets in a batch
    the points it gets alone.  `uniforms` (B, num_points, 3) in [0, 1) replaces the draws (tests).  A mesh without faces raises ValueError."""
    n = int(num_points)
    if n <= 0:
        raise ValueError(f"num_points must be positive, got {num_points!r}")
    verts, faces, offsets, rows = _pack_meshes(meshes, "sample_mesh_points")
    b = len(rows) - 1
    for i in range(b):
        if rows[i + 1][1] == rows[i][1] or rows[i + 1][0] == rows[i][0]:
            raise ValueError(f"sample_mesh_points: mesh {i} of the list has no faces")
    if seed is None:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
    u = None
    if uniforms is not None:
        if uniforms.device != verts.device or tuple(uniforms.shape) != (b, n, 3):
            raise ValueError(f"uniforms must be a ({b}, {n}, 3) tensor on the meshes' device")
        u = uniforms.to(torch.float32).contiguous()
    lib = _lib.load()
    ws = torch.empty(max(lib.pcd_mesh_sample_workspace_bytes(b, rows[-1][1]), 4) // 4, dtype=torch.float32, device=verts.device)
    points = torch.empty(b, n, 3, dtype=torch.float32, device=verts.device)
    normals = torch.empty(b, n, 3, dtype=torch.float32, device=verts.device) if return_normals else None
    index = torch.empty(b, n, dtype=torch.int32, device=verts.device) if return_faces else None
    _lib.check(lib.pcd_mesh_sample_points(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, n, int(seed) & 0xFFFFFFFFFFFFFFFF, 0,
                                          _lib.ptr(u), ws.data_ptr(), points.data_ptr(), _lib.ptr(normals), _lib.ptr(index),
                                          _lib.stream_ptr()), "mesh_sample_points")
    out = (points,) + ((normals,) if return_normals else ()) + ((index,) if return_faces else ())
    return out[0] if len(out) == 1 else out


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
