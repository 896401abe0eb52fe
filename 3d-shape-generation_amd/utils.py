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


def save_mesh(path: str, mesh, normals=None) -> None:
    """Write `mesh` = (vertices (V,3), faces (F,3)), CPU or device tensors, by the extension of `path`: `.obj` (text, `v x y z` lines with 9
    significant digits -- float32 round-trips -- and 1-based `f a b c` lines) or `.ply` (binary little-endian, `float x y z` and
    `list uchar int vertex_indices`).  With `normals` (V,3), one per vertex (`mesh_ops.vertex_normals`), the `.obj` also gets `vn` lines
    and `f a//a b//b c//c`, the `.ply` `float nx ny nz` on the vertex element.  Host only."""
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".obj", ".ply"):
        raise ValueError(f"save_mesh writes .obj or .ply, not {ext!r} ({path})")
    v, f = _mesh_arrays(mesh)
    n = None
    if normals is not None:
        n = np.ascontiguousarray(torch.as_tensor(normals).detach().cpu().numpy(), dtype="<f4")
        if n.shape != v.shape:
            raise ValueError(f"save_mesh: normals must be one row per vertex, {v.shape}, got {n.shape}")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if ext == ".obj":
        with open(path, "w") as out:
            out.write(f"# {v.shape[0]} vertices, {f.shape[0]} triangles\n")
            out.writelines(f"v {float(x):.9g} {float(y):.9g} {float(z):.9g}\n" for x, y, z in v)
            if n is None:
                out.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f.tolist())
            else:
                out.writelines(f"vn {float(x):.9g} {float(y):.9g} {float(z):.9g}\n" for x, y, z in n)
                out.writelines(f"f {a + 1}//{a + 1} {b + 1}//{b + 1} {c + 1}//{c + 1}\n" for a, b, c in f.tolist())
        return
    rows = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rows["n"] = 3
    rows["idx"] = f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n"
              + ("" if n is None else "property float nx\nproperty float ny\nproperty float nz\n") +
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write((v if n is None else np.concatenate([v, n], axis=1)).tobytes())
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


# ------------------------------------------------------------------ point-cloud files
def save_point_cloud(path: str, points, normals=None, ascii: bool = False) -> None:
    """Write a cloud (N, 3), CPU or device tensor, as a PLY file: element `vertex` with `float x y z` and, with `normals` (N, 3), `float nx ny
    nz`; binary little-endian, or text with 9 significant digits (float32 round-trips) under `ascii=True`.  Host only."""
    if os.path.splitext(path)[1].lower() != ".ply":
        raise ValueError(f"save_point_cloud writes .ply, not {os.path.splitext(path)[1]!r} ({path})")
    table = np.ascontiguousarray(torch.as_tensor(points).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    names = ["x", "y", "z"]
    if normals is not None:
        nrm = np.ascontiguousarray(torch.as_tensor(normals).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
        if nrm.shape != table.shape:
            raise ValueError(f"normals {nrm.shape} must be shaped like the points {table.shape}")
        table = np.ascontiguousarray(np.concatenate([table, nrm], axis=1))
        names += ["nx", "ny", "nz"]
    header = (f"ply\nformat {'ascii' if ascii else 'binary_little_endian'} 1.0\nelement vertex {table.shape[0]}\n"
              + "".join(f"property float {n}\n" for n in names) + "end_header\n")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        if ascii:
            out.write("".join(" ".join(f"{float(v):.9g}" for v in row) + "\n" for row in table).encode("ascii"))
        else:
            out.write(table.tobytes())


def load_point_cloud(path: str):
    """Read the vertex element of a PLY file, `ascii` or `binary_little_endian`, as a cloud: -> (points (N, 3) float32, normals (N, 3) float32
    or None), CPU tensors.  `x y z` (and `nx ny nz`, all three or none) must be `float` or `double` properties; other scalar vertex
    properties are skipped, and whatever follows the vertex element -- the faces of a mesh file -- is left unread.  `ValueError`, naming
    the file, for a file that is not such a PLY or that ends inside the vertex element."""
    if os.path.splitext(path)[1].lower() != ".ply":
        raise ValueError(f"load_point_cloud reads .ply, not {os.path.splitext(path)[1]!r} ({path})")
    with open(path, "rb") as src:
        raw = src.read()
    end = raw.find(b"end_header")
    nl = raw.find(b"\n", end)
    if not raw.startswith(b"ply") or end < 0 or nl < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' ... 'end_header')")
    fmt, count, props, element = None, None, [], None
    for line in raw[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format" and len(tok) > 1:
            fmt = tok[1]
        elif tok[0] == "element" and len(tok) > 2:
            element = tok[1]
            if element == "vertex" and count is None:
                try:
                    count = int(tok[2])
                except ValueError:
                    raise ValueError(f"{path}: the vertex count {tok[2]!r} is not a number") from None
            elif count is None:
                raise ValueError(f"{path}: the first element must be 'vertex', found {element!r}")
        elif tok[0] == "property" and element == "vertex" and len(tok) > 2:
            if tok[1] == "list":
                raise ValueError(f"{path}: a list property on the vertex element")
            if tok[1] not in _PLY_TYPES:
                raise ValueError(f"{path}: unknown property type {tok[1]!r}")
            props.append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt == "binary_big_endian":
        raise ValueError(f"{path}: binary_big_endian PLY files are not read (ascii and binary_little_endian are)")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: unknown PLY format {fmt!r}")
    if count is None or count < 0:
        raise ValueError(f"{path}: no vertex element")
    types = dict(props)
    have_normals = [a in types for a in ("nx", "ny", "nz")]
    if any(have_normals) and not all(have_normals):
        raise ValueError(f"{path}: nx, ny, nz must come all three or not at all")
    wanted = ["x", "y", "z"] + (["nx", "ny", "nz"] if all(have_normals) else [])
    for a in wanted:
        if types.get(a) not in ("f4", "f8"):
            raise ValueError(f"{path}: vertex property {a!r} must be float or double")
    body = raw[nl + 1:]
    if fmt == "ascii":
        lines = body.decode("ascii", "replace").split("\n")
        cols = [p[0] for p in props]
        ix = [cols.index(a) for a in wanted]
        try:
            table = np.asarray([[float(lines[i].split()[c]) for c in ix] for i in range(count)], np.float64).reshape(-1, len(wanted))
        except (IndexError, ValueError) as e:
            raise ValueError(f"{path}: the file ends inside the vertex element or a row is malformed ({e})") from None
    else:
        vdt = np.dtype([(n, "<" + t) for n, t in props])
        if len(body) < count * vdt.itemsize:
            raise ValueError(f"{path}: the file ends inside the vertex element")
        rows = np.frombuffer(body, dtype=vdt, count=count)
        table = np.stack([rows[a].astype(np.float64) for a in wanted], axis=1).reshape(-1, len(wanted))
    points = torch.from_numpy(np.ascontiguousarray(table[:, :3], dtype=np.float32))
    normals = torch.from_numpy(np.ascontiguousarray(table[:, 3:6], dtype=np.float32)) if all(have_normals) else None
    return points, normals


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


# ------------------------------------------------------------------ images out (csrc/render.hip)
DEFAULT_LIGHT = (-0.4, -0.6, -0.7)                               # normalised by the caller; view space, towards the surfaces that face the eye
DEFAULT_COLOR = (0.27, 0.51, 0.71)
RENDER_MAX_SIDE, RENDER_MAX_RADIUS = 2048, 64.0


def orbit_view(azim: float, elev: float, height: int, width: int, half_extent: float = 1.0, center=(0.0, 0.0, 0.0)) -> torch.Tensor:
    """(3, 4) float32 view [M | t] (DESIGN.md "Render"): an orthographic camera on a sphere round `center`, world z up, angles in degrees in
    matplotlib's convention, `half_extent` world units from the centre to the nearer image border.  Host arithmetic in float64."""
    if not (half_extent > 0.0 and np.isfinite(half_extent)):
        raise ValueError(f"half_extent must be positive and finite, got {half_extent!r}")
    a, e = np.deg2rad(float(azim)), np.deg2rad(float(elev))
    s = min(int(height), int(width)) / (2.0 * float(half_extent))
    right = np.array([-np.sin(a), np.cos(a), 0.0])
    up = np.array([-np.cos(a) * np.sin(e), -np.sin(a) * np.sin(e), np.cos(e)])
    toward = np.array([np.cos(a) * np.cos(e), np.sin(a) * np.cos(e), np.sin(e)])
    m = np.stack([s * right, -s * up, -s * toward])
    t = np.array([width / 2.0, height / 2.0, 0.0]) - m @ np.asarray(center, np.float64).reshape(3)
    return torch.from_numpy(np.concatenate([m, t[:, None]], axis=1).astype(np.float32))


def orbit_views(n: int, elev: float, height: int, width: int, half_extent: float = 1.0, center=(0.0, 0.0, 0.0),
                azim0: float = -60.0) -> torch.Tensor:
    """(n, 3, 4) float32: a turntable of `n` views at azimuths azim0 + 360 i / n."""
    if int(n) < 1:
        raise ValueError(f"orbit_views needs n >= 1, got {n!r}")
    return torch.stack([orbit_view(azim0 + 360.0 * i / int(n), elev, height, width, half_extent, center) for i in range(int(n))])


def _render_args(what, batch, views, height, width, radius, color, background, light, ambient, device):
    """Validate on the host and build (views tensor, view_sets, V, RenderStyle, the tensors it points to)."""
    h, w = int(height), int(width)
    if h != height or w != width or not (1 <= h <= RENDER_MAX_SIDE and 1 <= w <= RENDER_MAX_SIDE):
        raise ValueError(f"{what}: height and width must be integers in 1..{RENDER_MAX_SIDE}, got {height!r} x {width!r}")
    if not (0.0 < float(radius) <= RENDER_MAX_RADIUS):
        raise ValueError(f"{what}: radius must be in (0, {RENDER_MAX_RADIUS:g}] pixels, got {radius!r}")
    if not (0.0 <= float(ambient) <= 1.0):
        raise ValueError(f"{what}: ambient must be in [0, 1], got {ambient!r}")
    v = torch.as_tensor(views, dtype=torch.float32)
    if v.dim() == 2:
        v = v.unsqueeze(0)
    if v.dim() not in (3, 4) or tuple(v.shape[-2:]) != (3, 4) or v.shape[-3] < 1 or (v.dim() == 4 and v.shape[0] != batch):
        raise ValueError(f"{what}: views must be (3, 4), (V, 3, 4) or ({batch}, V, 3, 4), got {tuple(v.shape)}")
    view_sets = batch if v.dim() == 4 else 1
    n_views = int(v.shape[-3])
    v = v.to(device).contiguous()
    light = np.asarray(DEFAULT_LIGHT if light is None else light, np.float64).reshape(-1)
    if light.shape != (3,) or not np.isfinite(light).all() or not np.linalg.norm(light) > 0.0:
        raise ValueError(f"{what}: light must be a non-zero 3-vector")
    light = light / np.linalg.norm(light)
    bg = np.asarray(background, np.float64).reshape(-1)
    if bg.shape != (3,) or not ((bg >= 0.0) & (bg <= 1.0)).all():
        raise ValueError(f"{what}: background must be an RGB in [0, 1]")
    col = np.asarray(DEFAULT_COLOR if color is None else color, np.float64)
    if col.shape == (3,):
        col = np.broadcast_to(col, (batch, 3))
    if col.shape != (batch, 3) or not ((col >= 0.0) & (col <= 1.0)).all():
        raise ValueError(f"{what}: color must be an RGB in [0, 1] or one per shape ({batch}, 3)")
    colors = torch.from_numpy(np.ascontiguousarray(col, dtype=np.float32)).to(device)
    style = _lib.RenderStyle(colors.data_ptr(), (_lib.f32 * 3)(*light), float(ambient), (_lib.f32 * 3)(*bg))
    return v, view_sets, n_views, style, colors


def _render_outputs(batch, n_views, h, w, device, return_buffers):
    rgb = torch.empty(batch, n_views, h, w, 3, dtype=torch.uint8, device=device)
    ids = torch.empty(batch, n_views, h, w, dtype=torch.int32, device=device) if return_buffers else None
    depth = torch.empty(batch, n_views, h, w, dtype=torch.float32, device=device) if return_buffers else None
    return rgb, ids, depth


def render_point_clouds(clouds, views, height: int = 256, width: int = 256, radius: float = 1.5, color=None, background=(1.0, 1.0, 1.0),
                        light=None, ambient: float = 0.3, return_buffers: bool = False):
    """Depth-buffered discs (sphere impostors) of `radius` pixels (DESIGN.md "Render").  `clouds`: a (B, N, 3) tensor or a list of (n_i, 3)
    tensors on the device (the ragged output of `voxel_tensor_to_point_clouds`); an empty cloud gives a background image.  `views`: (3, 4),
    (V, 3, 4) shared by the shapes, or (B, V, 3, 4) (`orbit_view`, `orbit_views`).  -> uint8 (B, V, H, W, 3) on the device; with `return_buffers`
    also ids int32 (B, V, H, W) (the winning row of the cloud, -1 for background) and depth float32 (+inf for background).  One launch, integer
    atomics only: bitwise repeatable and independent of the rest of the batch."""
    what = "render_point_clouds"
    if torch.is_tensor(clouds):
        if clouds.dim() != 3 or clouds.shape[2] != 3:
            raise ValueError(f"{what}: a cloud tensor must be (B, N, 3), got {tuple(clouds.shape)}")
        clouds = list(clouds)
    clouds = list(clouds)
    if not clouds:
        raise ValueError(f"{what}: no clouds")
    rows = [0]
    for i, c in enumerate(clouds):
        if c.dim() != 2 or c.shape[1] != 3:
            raise ValueError(f"{what}: cloud {i} is not (n, 3)")
        if c.device.type != "cuda":
            raise RuntimeError(f"{what} runs only on an MI355X device (no CPU path)")
        rows.append(rows[-1] + c.shape[0])
    dev, b = clouds[0].device, len(clouds)
    v, view_sets, n_views, style, keep = _render_args(what, b, views, height, width, radius, color, background, light, ambient, dev)
    pts = torch.cat([c.to(torch.float32) for c in clouds]).contiguous() if rows[-1] else torch.zeros(1, 3, dtype=torch.float32, device=dev)
    offsets = torch.tensor(rows, dtype=torch.int64).to(dev, non_blocking=True)
    rgb, ids, depth = _render_outputs(b, n_views, int(height), int(width), dev, return_buffers)
    _lib.check(_lib.load().pcd_render_points(pts.data_ptr(), offsets.data_ptr(), b, v.data_ptr(), view_sets, n_views, int(height), int(width),
                                             float(radius), style, _lib.ptr(ids), _lib.ptr(depth), rgb.data_ptr(), _lib.stream_ptr()),
               "render_points")
    return (rgb, ids, depth) if return_buffers else rgb


def render_meshes(meshes, views, height: int = 256, width: int = 256, color=None, background=(1.0, 1.0, 1.0), light=None,
                  ambient: float = 0.3, return_buffers: bool = False):
    """Depth-buffered flat-shaded triangles, both faces drawn, watertight along shared edges (DESIGN.md "Render").  `meshes`: a list of `Mesh` /
    (vertices, faces) pairs on the device; a mesh without faces gives a background image.  Views and outputs as `render_point_clouds`; ids
    are face rows."""
    what = "render_meshes"
    verts, faces, offsets, rows = _pack_meshes(meshes, what)
    b = len(rows) - 1
    v, view_sets, n_views, style, keep = _render_args(what, b, views, height, width, 1.0, color, background, light, ambient, verts.device)
    rgb, ids, depth = _render_outputs(b, n_views, int(height), int(width), verts.device, return_buffers)
    _lib.check(_lib.load().pcd_render_meshes(verts.data_ptr(), faces.data_ptr(), offsets.data_ptr(), b, v.data_ptr(), view_sets, n_views,
                                             int(height), int(width), style, _lib.ptr(ids), _lib.ptr(depth), rgb.data_ptr(),
                                             _lib.stream_ptr()), "render_meshes")
    return (rgb, ids, depth) if return_buffers else rgb


def render_voxels(grid: torch.Tensor, views, threshold: float = 0.5, **kwargs):
    """(B, 1, D, H, W) grid -> images of its surface-nets meshes: `render_meshes(voxel_tensor_to_meshes(grid, threshold), views, ...)`."""
    return render_meshes(voxel_tensor_to_meshes(grid, threshold), views, **kwargs)


def image_grid(images: torch.Tensor, cols: int, pad: int = 0, background=(1.0, 1.0, 1.0)) -> torch.Tensor:
    """Contact sheet: (N, H, W, 3) uint8 (any leading shape, flattened; or one image) -> (rows (H + pad) - pad, cols (W + pad) - pad, 3), row-major, the
    last row filled up with `background`.  torch ops on the images' device."""
    if images.dim() < 3 or images.shape[-1] != 3 or images.dtype != torch.uint8:
        raise ValueError(f"image_grid takes uint8 (..., H, W, 3) images, got {images.dtype} {tuple(images.shape)}")
    cols = int(cols)
    if cols < 1 or pad < 0:
        raise ValueError(f"image_grid needs cols >= 1 and pad >= 0, got {cols!r}, {pad!r}")
    im = images.reshape(-1, *images.shape[-3:])
    n, h, w = im.shape[0], im.shape[1], im.shape[2]
    if n < 1:
        raise ValueError("image_grid: no images")
    rows = (n + cols - 1) // cols
    bg = torch.tensor([int(np.floor(255.0 * float(c) + 0.5)) for c in background], dtype=torch.uint8, device=im.device)
    sheet = bg.expand(rows, h + pad, cols, w + pad, 3).clone()
    full = bg.expand(rows * cols, h, w, 3).clone()
    full[:n] = im
    sheet[:, :h, :, :w] = full.reshape(rows, cols, h, w, 3).permute(0, 2, 1, 3, 4)
    return sheet.reshape(rows * (h + pad), cols * (w + pad), 3)[:rows * (h + pad) - pad, :cols * (w + pad) - pad].contiguous()


def save_png(path: str, image) -> None:
    """Write an (H, W, 3) uint8 image (tensor on any device, or array) as an 8-bit RGB PNG: zlib + struct, filter 0 on every row.  Host only."""
    import struct
    import zlib
    a = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"save_png writes uint8 (H, W, 3) images, got {a.dtype} {a.shape}")
    h, w = a.shape[0], a.shape[1]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), np.ascontiguousarray(a).reshape(h, w * 3)], axis=1).tobytes()

    def chunk(kind: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "wb") as out:
        out.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                  chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def axis_views(height: int, width: int, half_extent: float = 1.0) -> torch.Tensor:
    """(3, 3, 4) float32: the XY (from above), XZ (from the front) and YZ (from the side) orthographic views of the reference's 2-D panels."""
    return torch.stack([orbit_view(-90.0, 90.0, height, width, half_extent), orbit_view(-90.0, 0.0, height, width, half_extent),
                        orbit_view(0.0, 0.0, height, width, half_extent)])


def save_shape_pngs(png_dir: str, index: int, result, original=None, size: int = 256, radius: float = 1.5) -> None:
    """The reference's per-sample pictures (no text): `sample_{index}_3d.png` (one orbit view, azim -60, elev 30), `sample_{index}_2d.png`
    (XY | XZ | YZ) and, with `original`, `comparison_{index}.png` (original | result).  `result` / `original`: an (n, 3) cloud or a `Mesh` on
    the device."""
    def draw(shape, views):
        if isinstance(shape, (tuple, list)):
            return render_meshes([shape], views, size, size)[0]
        return render_point_clouds([shape], views, size, size, radius)[0]

    orbit = orbit_view(-60.0, 30.0, size, size)
    save_png(os.path.join(png_dir, f"sample_{index}_3d.png"), draw(result, orbit)[0])
    save_png(os.path.join(png_dir, f"sample_{index}_2d.png"), image_grid(draw(result, axis_views(size, size)), 3))
    if original is not None:
        save_png(os.path.join(png_dir, f"comparison_{index}.png"), image_grid(torch.stack([draw(original, orbit)[0], draw(result, orbit)[0]]), 2))


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
