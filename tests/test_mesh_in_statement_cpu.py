"""The float64 statement of the mesh-input definitions (tests/mesh_in_statement.py) against cases worked by hand, its two forms against each
other, the surface-nets round trip on the host, the share of voxels the conditioned random inputs of tests/test_gpu_mesh_in.py leave undecided
(asserted here, so the GPU test cannot hide it), and the argument refusals of the two entry points (no GPU)."""
import numpy as np
import pytest

import mesh_in_statement as S
import mesh_statement as M

R = 8
MARGIN = 1e-4            # voxels whose statement margin is below this are left out of the conditioned comparison ...
MAX_LEFT_OUT = 0.01      # ... and at most this share of a mesh's voxels may be


def box(lo, hi, r=R):
    """bool [z][y][x]: the nodes with lo <= index <= hi on every axis"""
    out = np.zeros((r, r, r), bool)
    out[lo:hi + 1, lo:hi + 1, lo:hi + 1] = True
    return out


def test_a_square_on_a_cube_face_touches_the_cubes_on_both_sides():
    """The unit square z = 2.5, 1.5 <= x, y <= 2.5, as two triangles: it is the face shared by the cubes of the nodes (z, y, x) = (2, 2, 2) and (3, 2, 2),
    and touches their neighbours in x and y along an edge or at a corner.  Ties count: 3 x 3 x 2 nodes."""
    v = np.asarray([(1.5, 1.5, 2.5), (2.5, 1.5, 2.5), (2.5, 2.5, 2.5), (1.5, 2.5, 2.5)])
    f = np.asarray([(0, 1, 2), (0, 2, 3)])
    want = np.zeros((R, R, R), bool)
    want[2:4, 1:4, 1:4] = True
    assert np.array_equal(S.voxelize_surface(v, f, R), want)
    occ, margin = S.voxelize_surface_vec(v, f, R)
    assert np.array_equal(occ, want)
    assert margin[2, 2, 2] == 0.0 and margin[3, 1, 3] == 0.0 and margin[4, 2, 2] > 0.05           # touching: no slack at all; a node further: a clear gap


def test_a_square_covering_one_node_fills_the_column_below_it():
    v = np.asarray([(1.5, 1.5, 2.5), (2.5, 1.5, 2.5), (2.5, 2.5, 2.5), (1.5, 2.5, 2.5)])
    f = np.asarray([(0, 1, 2), (0, 2, 3)])
    w = S.winding(v, f, R)
    want = np.zeros((R, R, R), np.int64)
    want[0:3, 2, 2] = 1                                                    # counter-clockwise seen from +z: n_z > 0; nodes z = 0, 1, 2 lie below 2.5
    assert np.array_equal(w, want)
    assert np.array_equal(S.winding(v, f[:, ::-1], R), -want)              # the other orientation
    assert int(S.voxelize_interior(v, f, R).sum()) == 3


def test_a_triangle_through_node_centres_is_not_above_them():
    """(0, 0, 3), (6, 0, 3), (0, 6, 3): the plane passes through the nodes z = 3.  Interior is strict, so only z = 0, 1, 2 count; the top-left rule
    keeps the edges y = 0 (d_y = 0, d_x > 0) and x = 0 (d_y < 0) and drops x + y = 6 (d_y > 0): the columns x, y >= 0, x + y <= 5, 21 of them."""
    v = np.asarray([(0.0, 0.0, 3.0), (6.0, 0.0, 3.0), (0.0, 6.0, 3.0)])
    f = np.asarray([(0, 1, 2)])
    w = S.winding(v, f, R)
    want = np.zeros((R, R, R), np.int64)
    for y in range(R):
        for x in range(R):
            if x + y <= 5:
                want[0:3, y, x] = 1
    assert np.array_equal(w, want) and int(want.sum()) == 63
    wv, margin = S.winding_vec(v, f, R)
    assert np.array_equal(wv, want)
    assert margin[3, 1, 1] == 0.0 and margin[2, 0, 3] == 0.0 and margin[1, 2, 2] > 0.05           # on the plane; on an edge; well inside
    surface = S.voxelize_surface(v, f, R)
    assert surface[3, 0, 0] and surface[3, 3, 3] and not surface[2, 1, 1] and not surface[4, 1, 1] and surface[3, 4, 3] and not surface[3, 4, 4]


def test_a_closed_cube_fills_the_nodes_strictly_inside_and_marks_its_shell():
    v, f = S.cube(1.5, 4.5)
    assert np.array_equal(S.voxelize_interior(v, f, R), box(2, 4))
    shell = box(1, 5)
    shell[3, 3, 3] = False                                                 # the one cube that reaches no face of the box
    assert np.array_equal(S.voxelize_surface(v, f, R), shell)
    assert np.array_equal(S.voxelize_solid(v, f, R), box(1, 5))
    # on integer coordinates the faces pass through nodes: strictly-above and top-left make every axis half open, [2, 5)
    vi, fi = S.cube(2.0, 5.0)
    assert np.array_equal(S.voxelize_interior(vi, fi, R), box(2, 4))


def test_overlapping_cubes_fill_their_union_and_an_inside_out_cube_fills_too():
    v, f = S.merge(S.cube(1.5, 4.5), S.cube(2.5, 5.5))
    w = S.winding(v, f, R)
    assert np.array_equal(w != 0, box(2, 4) | box(3, 5))
    assert np.array_equal(w == 2, box(3, 4))                               # parity would empty the part they share
    vo, fo = S.cube(1.5, 4.5, inside_out=True)
    wo = S.winding(vo, fo, R)
    assert np.array_equal(wo, -box(2, 4).astype(np.int64)) and np.array_equal(S.voxelize_interior(vo, fo, R), box(2, 4))


def test_degenerate_triangles_are_tested_as_segments_and_points():
    seg = np.asarray([(1.0, 1.0, 1.0), (3.0, 1.0, 1.0), (2.0, 1.0, 1.0)])  # collinear: the segment x = 1 .. 3
    got = S.voxelize_surface(seg, [(0, 1, 2)], R)
    want = np.zeros((R, R, R), bool)
    want[1, 1, 1:4] = True
    assert np.array_equal(got, want)
    pt = np.asarray([(2.5, 2.0, 2.0)] * 3)                                 # a point on the face between two cubes
    got = S.voxelize_surface(pt, [(0, 1, 2)], R)
    want = np.zeros((R, R, R), bool)
    want[2, 2, 2:4] = True
    assert np.array_equal(got, want)
    assert not S.voxelize_interior(seg, [(0, 1, 2)], R).any() and not S.voxelize_interior(pt, [(0, 1, 2)], R).any()
    diag = np.asarray([(0.0, 0.0, 0.0), (2.0, 2.0, 0.0), (2.0, 2.0, 0.0)])  # a diagonal segment passes the corner shared by (0, 1), (1, 0): both touch
    got = S.voxelize_surface(diag, [(0, 1, 2)], R)
    assert got[0, 0, 0] and got[0, 1, 1] and got[0, 2, 2] and got[0, 0, 1] and got[0, 1, 0] and not got[0, 0, 2] and not got[1].any()


def test_the_two_forms_agree_on_lattice_triangles():
    v, f = S.lattice_triangles(40, 0)
    occ, _ = S.voxelize_surface_vec(v, f, R)
    assert np.array_equal(S.voxelize_surface(v, f, R), occ) and 0 < int(occ.sum()) < R ** 3
    w, _ = S.winding_vec(v, f, R)
    assert np.array_equal(S.winding(v, f, R), w) and int((w != 0).sum()) > 0


@pytest.mark.parametrize("name", ["checkerboard", "single_voxel", "random"])
def test_surface_nets_round_trip_on_the_host(name):
    """Every surface-nets quad is pierced once by the grid edge it is dual to and by no other grid line, so the interior of a grid's mesh is the grid."""
    shape = (R, R, R)
    g = {"checkerboard": lambda: M.checkerboard(shape), "single_voxel": lambda: M.single_voxel(shape, (3, 0, 7)),
         "random": lambda: M.lattice((np.random.default_rng(3).random(shape) < 0.4).astype(np.float64))}[name]()
    v, f = M.surface_nets(g, 0.5)
    p = S.index_coords(v, R)
    want = g > 0.5
    if name != "checkerboard":                                             # the plain loops: ~ 1e5 (triangle, column) pairs; the checkerboard has 4e5
        assert np.array_equal(S.voxelize_interior(p, f, R), want)
    assert np.array_equal(S.voxelize_interior_vec(p, f, R)[0], want)


def test_conditioned_inputs_leave_few_voxels_undecided():
    """The inputs of test_gpu_mesh_in.py's conditioned comparison: per mesh, the share of voxels with a margin under 1e-4 stays under 1 %, and the
    mesh occupies voxels."""
    for seed in range(4):
        v, f = S.conditioned_triangles(300, seed)
        t = v[f].astype(np.float64)
        edges = np.linalg.norm(t - np.roll(t, 1, axis=1), axis=2) / (2.0 / 31.0)
        assert v.dtype == np.float32 and edges.min() >= 2.0 - 1e-6 and edges.max() <= 10.0 + 1e-6 and np.abs(v).max() <= 1.0
        occ, margin = S.voxelize_surface_vec(S.index_coords(v, 32), f, 32)
        left_out = float((margin < MARGIN).mean())
        print(f"mesh {seed}: occupied {int(occ.sum())}, left out {left_out:.5f}")
        assert int(occ.sum()) > 0
        assert left_out <= MAX_LEFT_OUT


def test_entry_points_refuse_bad_arguments_without_a_device():
    from shapegen_amd import _lib
    lib = _lib.load()
    p = 64                                                                 # never dereferenced on the host
    ok = dict(vertices=p, faces=p, offsets=p, batch=2, r=32, lo=-1.0, inv_pitch=15.5, mode=2, workspace=p, vox=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pcd_mesh_voxelize(a["vertices"], a["faces"], a["offsets"], a["batch"], a["r"], a["lo"], a["inv_pitch"], a["mode"], a["workspace"],
                                     a["vox"], 0)

    bad = [dict(vertices=None), dict(faces=None), dict(offsets=None), dict(workspace=None), dict(vox=None), dict(batch=0), dict(batch=-3),
           dict(r=1), dict(r=65), dict(r=0), dict(mode=3), dict(mode=-1), dict(lo=float("nan")), dict(lo=float("inf")),
           dict(inv_pitch=float("nan")), dict(inv_pitch=float("inf")), dict(inv_pitch=0.0), dict(inv_pitch=-1.0)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"bad argument" in lib.pcd_last_error()
    assert lib.pcd_mesh_voxelize_workspace_bytes(0, 32) == 0 and lib.pcd_mesh_voxelize_workspace_bytes(1, 1) == 0
    assert lib.pcd_mesh_voxelize_workspace_bytes(1, 65) == 0
    one = lib.pcd_mesh_voxelize_workspace_bytes(1, 64)
    assert one >= 64 ** 3 * 4 + 64 ** 3 // 8 and lib.pcd_mesh_voxelize_workspace_bytes(5, 64) == 5 * one
    assert lib.pcd_mesh_voxelize_workspace_bytes(3, 2) > 0

    def sample(**kw):
        a = dict(dict(vertices=p, faces=p, offsets=p, batch=2, n=16, u=None, workspace=p, points=p, normals=None, index=None), **kw)
        return lib.pcd_mesh_sample_points(a["vertices"], a["faces"], a["offsets"], a["batch"], a["n"], 1, 0, a["u"], a["workspace"], a["points"],
                                          a["normals"], a["index"], 0)

    for kw in (dict(vertices=None), dict(faces=None), dict(offsets=None), dict(workspace=None), dict(points=None), dict(batch=0), dict(n=0),
               dict(batch=65536)):
        assert sample(**kw) == -1, kw
    assert lib.pcd_mesh_sample_workspace_bytes(0, 10) == 0 and lib.pcd_mesh_sample_workspace_bytes(2, 0) == 0
    assert lib.pcd_mesh_sample_workspace_bytes(2, 1000) >= 4000
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcd_hip.h")).read()
    fills = {k: int(v) for k, v in re.findall(r"#define PCD_MESH_FILL_(\w+) (\d+)", header)}
    from shapegen_amd.utils import MESH_FILLS
    assert {k.lower(): v for k, v in fills.items()} == MESH_FILLS
