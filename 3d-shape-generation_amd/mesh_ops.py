"""Mesh processing on the device (csrc/mesh_ops.hip; DESIGN.md "Mesh processing"): vertex rings, Taubin smoothing, vertex normals,
connected components, compaction and measures, and (csrc/mesh_simplify.hip; DESIGN.md "Mesh simplification") simplification by vertex
clustering, on lists of `utils.Mesh` / (vertices, faces) pairs.  No CPU path."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from .utils import Mesh, _pack_meshes

VERTEX_REFERENCED, VERTEX_BOUNDARY, VERTEX_IRREGULAR = 1, 2, 4    # include/pcd_hip.h PCD_MESH_VERTEX_*
KEEP_LARGEST, KEEP_MIN_FACES = 0, 1                              # include/pcd_hip.h PCD_MESH_KEEP_*
MEASURES = ("vertices", "edges", "faces", "boundary_edges", "irregular_edges", "components", "euler", "closed")


class MeshAdjacency(NamedTuple):
    """The vertex rings of a packed batch.  Rows are indexed by packed vertex row; the entries are local to their mesh."""
    rows_table: tuple                 # ((first vertex row, first face row), ...) of the B meshes and the totals: the packing it was built for
    nbr_start: torch.Tensor           # (sum V + 1,) int32
    nbr_index: torch.Tensor           # (6 sum F,) int32, written up to nbr_start[-1]
    nbr_counts: torch.Tensor          # (6 sum F, 2) int32 (out, in)
    inc_start: torch.Tensor           # (sum V + 1,) int32
    inc_faces: torch.Tensor           # (3 sum F,) int32, written up to inc_start[-1]
    vertex_flags: torch.Tensor        # (sum V,) int32, VERTEX_* bits

    def _span(self, i: int) -> Tuple[int, int]:
        return self.rows_table[i][0], self.rows_table[i + 1][0]

    def rows(self, i: int):
        """Mesh i: (start (V + 1,) into the next two, index (E,), counts (E, 2)) of its neighbour rows, and (start, faces) of its
        incidence rows.  One host read of the two row bounds."""
        v0, v1 = self._span(i)
        ns = self.nbr_start[v0:v1 + 1]
        cs = self.inc_start[v0:v1 + 1]
        n0, n1, c0, c1 = torch.stack([ns[0], ns[-1], cs[0], cs[-1]]).tolist()
        return (ns - n0, self.nbr_index[n0:n1], self.nbr_counts[n0:n1]), (cs - c0, self.inc_faces[c0:c1])

    def flags(self, i: int) -> torch.Tensor:
        v0, v1 = self._span(i)
        return self.vertex_flags[v0:v1]

    def boundary(self, i: int) -> torch.Tensor:
        return (self.flags(i) & VERTEX_BOUNDARY) != 0


class _Packed(NamedTuple):
    verts: torch.Tensor
    faces: torch.Tensor
    offsets: torch.Tensor
    rows: list

    @property
    def batch(self) -> int:
        return len(self.rows) - 1

    @property
    def totals(self) -> Tuple[int, int]:
        return self.rows[-1]

    @property
    def max_vertices(self) -> int:
        return max(b[0] - a[0] for a, b in zip(self.rows[:-1], self.rows[1:]))

    def split_vertices(self, t: torch.Tensor) -> List[torch.Tensor]:
        return list(torch.split(t[:self.totals[0]], [b[0] - a[0] for a, b in zip(self.rows[:-1], self.rows[1:])]))


def _pack(meshes, what: str) -> Tuple[_Packed, List[Mesh]]:
    meshes = [Mesh(*m) for m in meshes]
    return _Packed(*_pack_meshes(meshes, what)), meshes


def _i32(n: int, dev, *shape) -> torch.Tensor:
    return torch.empty((max(n, 1),) + shape, dtype=torch.int32, device=dev)


def _adjacency(p: _Packed, adjacency: Optional[MeshAdjacency], what: str) -> MeshAdjacency:
    if adjacency is not None:
        if tuple(map(tuple, p.rows)) != adjacency.rows_table or adjacency.nbr_start.device != p.verts.device:
            raise ValueError(f"{what}: adjacency was built for other meshes (sizes or device differ)")
        return adjacency
    lib = _lib.load()
    b, (tv, tf), dev = p.batch, p.totals, p.verts.device
    ws = torch.empty(max(lib.pcd_mesh_adjacency_workspace_bytes(b, tv, tf), 8) // 8, dtype=torch.int64, device=dev)
    adj = MeshAdjacency(tuple(map(tuple, p.rows)), _i32(tv + 1, dev), _i32(6 * tf, dev), _i32(6 * tf, dev, 2), _i32(tv + 1, dev),
                        _i32(3 * tf, dev), _i32(tv, dev))
    _lib.check(lib.pcd_mesh_adjacency(p.faces.data_ptr(), p.offsets.data_ptr(), b, tv, tf, ws.data_ptr(), adj.nbr_start.data_ptr(),
                                      adj.nbr_index.data_ptr(), adj.nbr_counts.data_ptr(), adj.inc_start.data_ptr(),
                                      adj.inc_faces.data_ptr(), adj.vertex_flags.data_ptr(), _lib.stream_ptr()), "mesh_adjacency")
    return adj


def mesh_adjacency(meshes) -> MeshAdjacency:
    """The vertex rings of a list of meshes: per vertex its distinct neighbours in ascending order, each with the number of valid faces
    holding the edge towards and from it, its incident valid faces in ascending order, and the VERTEX_* flags.  A face is valid iff its
    indices are rows of the mesh and pairwise different.  No host synchronisation; pass the result as `adjacency=` to build it once."""
    p, _ = _pack(meshes, "mesh_adjacency")
    return _adjacency(p, None, "mesh_adjacency")


def _check_smooth(iterations, lam, mu) -> Tuple[int, float, float]:
    n = int(iterations)
    if n != iterations or n < 0:
        raise ValueError(f"iterations must be an integer >= 0, got {iterations!r}")
    lam, mu = float(lam), float(mu)
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError(f"lam and mu must be finite, got {lam!r}, {mu!r}")
    if not 0.0 < lam <= 1.0:
        raise ValueError(f"lam must lie in (0, 1], got {lam!r}")
    if not -1.0 < mu <= 0.0:
        raise ValueError(f"mu must lie in (-1, 0] (0: plain Laplacian smoothing), got {mu!r}")
    if mu != 0.0 and abs(mu) < lam:
        raise ValueError(f"a nonzero mu must not be smaller in size than lam (the pair would shrink the mesh), got lam {lam!r}, mu {mu!r}")
    return n, lam, mu


def smooth_meshes(meshes, iterations: int = 10, lam: float = 0.5, mu: float = -0.53, pin_boundary: bool = False,
                  adjacency: Optional[MeshAdjacency] = None) -> List[Mesh]:
    """Taubin smoothing: `iterations` rounds of a `lam` step then a `mu` step of the uniform umbrella operator (x' = x + f (mean of the
    ring - x), all vertices from the old positions); mu = 0 gives plain Laplacian smoothing, one step a round.  Faces are shared with
    the input, vertices are new; `iterations=0` returns the positions bitwise, `pin_boundary` keeps boundary vertices where they are.
    One launch per step over the whole batch; no host synchronisation."""
    n, lam, mu = _check_smooth(iterations, lam, mu)
    (p, meshes) = _pack(meshes, "smooth_meshes")
    adj = _adjacency(p, adjacency, "smooth_meshes")
    lib = _lib.load()
    tv, dev = p.totals[0], p.verts.device
    out = torch.empty(max(tv, 1), 3, dtype=torch.float32, device=dev)
    ws = torch.empty(max(lib.pcd_mesh_smooth_workspace_bytes(tv), 4) // 4, dtype=torch.float32, device=dev)
    _lib.check(lib.pcd_mesh_smooth(p.verts.data_ptr(), p.offsets.data_ptr(), p.batch, tv, adj.nbr_start.data_ptr(),
                                   adj.nbr_index.data_ptr(), adj.vertex_flags.data_ptr(), n, lam, mu, int(bool(pin_boundary)),
                                   ws.data_ptr(), out.data_ptr(), _lib.stream_ptr()), "mesh_smooth")
    return [Mesh(v, m.faces) for v, m in zip(p.split_vertices(out), meshes)]


def vertex_normals(meshes, adjacency: Optional[MeshAdjacency] = None) -> List[torch.Tensor]:
    """Per mesh the (V, 3) area-weighted unit vertex normals; zeros at unreferenced vertices and where the faces cancel."""
    p, _ = _pack(meshes, "vertex_normals")
    adj = _adjacency(p, adjacency, "vertex_normals")
    lib = _lib.load()
    tv = p.totals[0]
    out = torch.empty(max(tv, 1), 3, dtype=torch.float32, device=p.verts.device)
    _lib.check(lib.pcd_mesh_vertex_normals(p.verts.data_ptr(), p.faces.data_ptr(), p.offsets.data_ptr(), p.batch, tv,
                                           adj.inc_start.data_ptr(), adj.inc_faces.data_ptr(), out.data_ptr(), _lib.stream_ptr()),
               "mesh_vertex_normals")
    return p.split_vertices(out)


def _components(p: _Packed, adj: MeshAdjacency):
    lib = _lib.load()
    tv, dev = p.totals[0], p.verts.device
    labels, sizes, counts = _i32(tv, dev), _i32(tv, dev), _i32(p.batch, dev)
    ws = _i32(max(lib.pcd_mesh_components_workspace_bytes(tv), 4) // 4, dev)
    _lib.check(lib.pcd_mesh_components(p.faces.data_ptr(), p.offsets.data_ptr(), p.batch, tv, p.max_vertices, adj.nbr_start.data_ptr(),
                                       adj.nbr_index.data_ptr(), adj.vertex_flags.data_ptr(), ws.data_ptr(), labels.data_ptr(),
                                       counts.data_ptr(), sizes.data_ptr(), _lib.stream_ptr()), "mesh_components")
    return labels, counts, sizes


def connected_components(meshes, adjacency: Optional[MeshAdjacency] = None, return_sizes: bool = False):
    """-> (labels, counts): per mesh the (V,) int32 label of every vertex, the least vertex index of its component (-1 for a vertex in
    no valid face), and the (B,) int32 device tensor of component counts.  With `return_sizes` also, per mesh, the (V,) int32 face count
    of the component each label root names (0 at the other vertices)."""
    p, _ = _pack(meshes, "connected_components")
    labels, counts, sizes = _components(p, _adjacency(p, adjacency, "connected_components"))
    out = (p.split_vertices(labels), counts)
    return out + (p.split_vertices(sizes),) if return_sizes else out


def _compact(p: _Packed, keep: torch.Tensor) -> List[Mesh]:
    lib = _lib.load()
    tv, dev, b = p.totals[0], p.verts.device, p.batch
    ws = _i32(max(lib.pcd_mesh_compact_workspace_bytes(tv), 4) // 4, dev)
    counts = torch.empty(b, 2, dtype=torch.int32, device=dev)
    _lib.check(lib.pcd_mesh_compact_count(p.faces.data_ptr(), p.offsets.data_ptr(), b, keep.data_ptr(), ws.data_ptr(), counts.data_ptr(),
                                          _lib.stream_ptr()), "mesh_compact_count")
    offsets = (torch.cumsum(counts, dim=0, dtype=torch.int64) - counts).contiguous()
    cnt = counts.cpu().tolist()          # the packed outputs are sized on the host: one sync, as in voxel_tensor_to_meshes
    nv, nf = [c[0] for c in cnt], [c[1] for c in cnt]
    verts = torch.empty(max(sum(nv), 1), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(max(sum(nf), 1), 3, dtype=torch.int32, device=dev)
    _lib.check(lib.pcd_mesh_compact_emit(p.verts.data_ptr(), p.faces.data_ptr(), p.offsets.data_ptr(), b, ws.data_ptr(), offsets.data_ptr(),
                                         verts.data_ptr(), faces.data_ptr(), _lib.stream_ptr()), "mesh_compact_emit")
    return [Mesh(v, f) for v, f in zip(torch.split(verts[:sum(nv)], nv), torch.split(faces[:sum(nf)], nf))]


def compact_meshes(meshes, keep: Sequence[torch.Tensor]) -> List[Mesh]:
    """Keep the vertices flagged in `keep` (a list of bool / int (V,) tensors, nonzero = kept) in order, and in order the valid faces
    whose three vertices are all kept, renumbered.  Invalid faces are dropped.  One host synchronisation to size the outputs."""
    meshes, keep = list(meshes), list(keep)
    if len(keep) != len(meshes):
        raise ValueError(f"compact_meshes: {len(meshes)} meshes but {len(keep)} keep tensors")
    for i, (m, k) in enumerate(zip(meshes, keep)):
        if k.dim() != 1 or k.shape[0] != m[0].shape[0] or k.dtype.is_floating_point or k.dtype.is_complex:
            raise ValueError(f"compact_meshes: keep[{i}] must be a bool or integer ({m[0].shape[0]},) tensor")
    p, _ = _pack(meshes, "compact_meshes")
    if any(k.device != p.verts.device for k in keep):
        raise RuntimeError("compact_meshes runs only on an MI355X device (no CPU path): keep must be on the meshes' device")
    flat = torch.cat([(k != 0).to(torch.int32) for k in keep]) if p.totals[0] else _i32(1, p.verts.device)
    return _compact(p, flat.contiguous())


def remove_small_components(meshes, min_faces: Optional[int] = None, keep_largest: bool = False) -> List[Mesh]:
    """Drop connected components: with `keep_largest` all but the one with the most faces (the smaller label on a tie), with `min_faces`
    those with fewer faces.  Exactly one of the two must be given.  Unreferenced vertices and invalid faces go too."""
    if (min_faces is None) == (not keep_largest):
        raise ValueError("remove_small_components: give exactly one of min_faces and keep_largest")
    k = 0
    if min_faces is not None:
        k = int(min_faces)
        if k != min_faces or k < 0:
            raise ValueError(f"min_faces must be an integer >= 0, got {min_faces!r}")
    p, _ = _pack(meshes, "remove_small_components")
    labels, _, sizes = _components(p, _adjacency(p, None, "remove_small_components"))
    keep = _i32(p.totals[0], p.verts.device)
    _lib.check(_lib.load().pcd_mesh_component_keep(p.offsets.data_ptr(), p.batch, labels.data_ptr(), sizes.data_ptr(),
                                                   KEEP_LARGEST if keep_largest else KEEP_MIN_FACES, k, keep.data_ptr(), _lib.stream_ptr()),
               "mesh_component_keep")
    return _compact(p, keep)


SIMPLIFY_RESOLUTION, SIMPLIFY_CELL_SIZE, SIMPLIFY_TARGET_FACES = 0, 1, 2   # include/pcd_hip.h PCD_MESH_SIMPLIFY_*
PLACEMENTS = {"quadric": 0, "mean": 1}
SIMPLIFY_MAX_RESOLUTION, SIMPLIFY_MAX_VERTICES = 1024, 1 << 21


def _per_mesh(value, batch: int, name: str) -> list:
    values = list(value) if isinstance(value, (list, tuple)) or (torch.is_tensor(value) and value.dim() > 0) else [value] * batch
    if len(values) != batch:
        raise ValueError(f"{name} must be a scalar or one value per mesh ({batch}), got {len(values)}")
    return [v.item() if torch.is_tensor(v) else v for v in values]


def _check_simplify(batch: int, resolution, cell_size, target_faces, placement) -> Tuple[int, list, int]:
    """-> (mode, one validated value per mesh, placement code)"""
    given = [(m, v) for m, v in ((SIMPLIFY_RESOLUTION, resolution), (SIMPLIFY_CELL_SIZE, cell_size), (SIMPLIFY_TARGET_FACES, target_faces))
             if v is not None]
    if len(given) != 1:
        raise ValueError("simplify_meshes: give exactly one of resolution, cell_size and target_faces")
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be 'quadric' or 'mean', got {placement!r}")
    mode, value = given[0]
    if mode == SIMPLIFY_CELL_SIZE:
        values = [float(c) for c in _per_mesh(value, batch, "cell_size")]
        for c in values:
            if not (math.isfinite(c) and c > 0.0):
                raise ValueError(f"cell_size must be finite and > 0, got {c!r}")
        return mode, values, PLACEMENTS[placement]
    name = "resolution" if mode == SIMPLIFY_RESOLUTION else "target_faces"
    values = []
    for x in _per_mesh(value, batch, name):
        n = int(x)
        if n != x:
            raise ValueError(f"{name} must be an integer, got {x!r}")
        if mode == SIMPLIFY_RESOLUTION and not 1 <= n <= SIMPLIFY_MAX_RESOLUTION:
            raise ValueError(f"resolution must lie in 1 .. {SIMPLIFY_MAX_RESOLUTION}, got {x!r}")
        if mode == SIMPLIFY_TARGET_FACES and not 0 <= n < 2 ** 31:
            raise ValueError(f"target_faces must be an integer >= 0, got {x!r}")
        values.append(n)
    return mode, values, PLACEMENTS[placement]


def simplify_meshes(meshes, resolution=None, cell_size=None, target_faces=None, placement: str = "quadric", deduplicate: bool = False,
                    return_map: bool = False):
    """Simplification by vertex clustering (DESIGN.md "Mesh simplification"): per mesh a grid of `resolution`^3 cubic cells over the box of
    its referenced vertices (or cells of side `cell_size`, or the resolution a ten-round bisection on the device finds for a budget of
    `target_faces`: the result has at most that many faces); the vertices of a cell become one vertex, at the minimiser of the cell's summed
    face quadrics pulled towards the members' mean (`placement="quadric"`) or at the mean (`"mean"`), and the faces that keep three
    different vertices survive, in order.  Exactly one of the first three must be given, a scalar or one value per mesh.  Unreferenced
    vertices and invalid faces go; a cluster whose faces all collapse keeps its vertex.  A closed mesh (`mesh_measures(...)["closed"]`) stays closed; `deduplicate` keeps only the first of the
    faces with the same oriented vertex triple and may break that.  -> list of Mesh; with `return_map` (meshes, maps, resolutions): per mesh
    the (V,) int32 new index of every input vertex (-1 unreferenced) and the (B,) int32 device tensor of the resolutions used.  Bitwise
    repeatable; one host read to size the result."""
    meshes = list(meshes)
    mode, values, place = _check_simplify(len(meshes), resolution, cell_size, target_faces, placement)
    p, _ = _pack(meshes, "simplify_meshes")
    if p.max_vertices >= SIMPLIFY_MAX_VERTICES:
        raise ValueError(f"simplify_meshes: a mesh has {p.max_vertices} vertices, the limit is {SIMPLIFY_MAX_VERTICES - 1}")
    lib = _lib.load()
    b, (tv, tf), dev = p.batch, p.totals, p.verts.device
    params = torch.tensor(values, dtype=torch.float32 if mode == SIMPLIFY_CELL_SIZE else torch.int32).to(dev)
    nbytes = lib.pcd_mesh_simplify_workspace_bytes(b, tv, tf)
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=dev)
    res, vmap, counts = _i32(b, dev), _i32(tv, dev), torch.empty(b, 2, dtype=torch.int32, device=dev)
    sizes = (b, tv, tf, p.max_vertices)
    _lib.check(lib.pcd_mesh_simplify_count(p.verts.data_ptr(), p.faces.data_ptr(), p.offsets.data_ptr(), *sizes, mode, params.data_ptr(),
                                           int(bool(deduplicate)), ws.data_ptr(), nbytes, res.data_ptr(), vmap.data_ptr(), counts.data_ptr(),
                                           _lib.stream_ptr()), "mesh_simplify_count")
    offsets = (torch.cumsum(counts, dim=0, dtype=torch.int64) - counts).contiguous()
    cnt = counts.cpu().tolist()          # the packed outputs are sized on the host: the one sync, as in _compact
    nv, nf = [c[0] for c in cnt], [c[1] for c in cnt]
    verts = torch.empty(max(sum(nv), 1), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(max(sum(nf), 1), 3, dtype=torch.int32, device=dev)
    _lib.check(lib.pcd_mesh_simplify_emit(p.verts.data_ptr(), p.faces.data_ptr(), p.offsets.data_ptr(), *sizes, place, ws.data_ptr(), nbytes,
                                          offsets.data_ptr(), verts.data_ptr(), faces.data_ptr(), _lib.stream_ptr()), "mesh_simplify_emit")
    out = [Mesh(v, f) for v, f in zip(torch.split(verts[:sum(nv)], nv), torch.split(faces[:sum(nf)], nf))]
    return (out, p.split_vertices(vmap), res[:b]) if return_map else out


def add_simplify_arguments(ap) -> None:
    """The simplification flags of `process_meshes.py` and `generate_mesh_ldm.py` on an argparse parser"""
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--simplify-resolution", type=int, default=None, metavar="R", help="cluster the vertices in an R^3 grid over each mesh's box")
    how.add_argument("--simplify-cell", type=float, default=None, metavar="H", help="cluster the vertices in cubic cells of side H")
    how.add_argument("--target-faces", type=int, default=None, metavar="N", help="the finest grid a bisection finds that leaves at most N faces")
    ap.add_argument("--placement", choices=tuple(PLACEMENTS), default="quadric", help="a cluster's vertex: quadric minimiser or mean")
    ap.add_argument("--deduplicate", action="store_true", help="keep one of the faces that share an oriented vertex triple")


def simplify_keywords(args) -> dict:
    """`process_meshes`' keywords from the flags of `add_simplify_arguments`"""
    return dict(simplify_resolution=args.simplify_resolution, simplify_cell_size=args.simplify_cell, target_faces=args.target_faces,
                placement=args.placement, deduplicate=args.deduplicate)


def process_meshes(meshes, keep_largest: bool = False, min_faces: Optional[int] = None, smooth: int = 0, lam: float = 0.5, mu: float = -0.53,
                   pin_boundary: bool = False, normals: bool = False, simplify_resolution=None, simplify_cell_size=None, target_faces=None,
                   placement: str = "quadric", deduplicate: bool = False, info: Optional[dict] = None):
    """The steps of `process_meshes.py` and `generate_mesh_ldm.py` in their fixed order -- components, then simplification, then smoothing,
    then normals -- each only where asked for.  -> (meshes, list of (V, 3) normals or None).  A dict passed as `info` gets
    `resolutions`, the (B,) int32 device tensor of the grid resolutions used, where simplification ran."""
    _check_smooth(smooth, lam, mu)
    meshes = [Mesh(*m) for m in meshes]
    simplify = any(x is not None for x in (simplify_resolution, simplify_cell_size, target_faces))
    if simplify:
        _check_simplify(len(meshes), simplify_resolution, simplify_cell_size, target_faces, placement)
    if keep_largest or min_faces is not None:
        meshes = remove_small_components(meshes, min_faces=min_faces, keep_largest=keep_largest)
    if simplify:
        meshes, _, resolutions = simplify_meshes(meshes, resolution=simplify_resolution, cell_size=simplify_cell_size,
                                                 target_faces=target_faces, placement=placement, deduplicate=deduplicate, return_map=True)
        if info is not None:
            info["resolutions"] = resolutions
    adj = mesh_adjacency(meshes) if smooth > 0 or normals else None
    if smooth > 0:
        meshes = smooth_meshes(meshes, smooth, lam, mu, pin_boundary=pin_boundary, adjacency=adj)
    return meshes, (vertex_normals(meshes, adjacency=adj) if normals else None)


def mesh_measures(meshes, adjacency: Optional[MeshAdjacency] = None) -> dict:
    """Per mesh, as (B,) device tensors: float64 `area`, signed `volume` and (B, 3) `centroid` (area-weighted, of the surface), and
    int32 `vertices` (referenced), `edges`, `faces` (valid), `boundary_edges`, `irregular_edges`, `components`, `euler` (V - E + F) and
    `closed` (1 iff every directed edge occurs as often as its reverse: the predicate of `utils.mesh_is_closed`)."""
    p, _ = _pack(meshes, "mesh_measures")
    adj = _adjacency(p, adjacency, "mesh_measures")
    labels, _, _ = _components(p, adj)
    real = torch.empty(p.batch, 5, dtype=torch.float64, device=p.verts.device)
    whole = torch.empty(p.batch, 8, dtype=torch.int32, device=p.verts.device)
    _lib.check(_lib.load().pcd_mesh_measures(p.verts.data_ptr(), p.faces.data_ptr(), p.offsets.data_ptr(), p.batch, adj.nbr_start.data_ptr(),
                                             adj.nbr_index.data_ptr(), adj.nbr_counts.data_ptr(), labels.data_ptr(), real.data_ptr(),
                                             whole.data_ptr(), _lib.stream_ptr()), "mesh_measures")
    out = {"area": real[:, 0], "volume": real[:, 1], "centroid": real[:, 2:5]}
    out.update({name: whole[:, i] for i, name in enumerate(MEASURES)})
    return out
