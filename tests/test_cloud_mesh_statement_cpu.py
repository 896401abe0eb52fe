"""The statement of the cloud-to-mesh definition (tests/cloud_mesh_statement.py) against independent implementations and against the geometric
conditions the method promises, on the CPU: its outside equals scipy.ndimage.label's component of the padding, its depth equals
scipy.ndimage.distance_transform_edt squared, its boxed shell equals the brute force over every pair, and the meshes of the condition cases
are closed with the right Euler characteristic.

Figures of the condition cases on the statement (tests/cloud_mesh_cases.py seeds; scale 1.5, k = 8, bounds +-1.25), for the record -- the
bounds asserted are the issue's, 0.02 for the sphere's radial band and 1 % flipped triangles, which its prototype met with 0.0098 / 0.0100 and
<= 0.01 %: the test prints what these seeds give."""
import numpy as np
import pytest

import cloud_mesh_cases as C
import cloud_mesh_statement as S


@pytest.mark.parametrize("R", [8, 31, 33])
def test_outside_and_depth_equal_scipy(R):
    from scipy import ndimage
    rng = np.random.default_rng(R)
    for density in (0.3, 0.6):
        shell = rng.random((R, R, R)) < density
        outside = S.outside_bfs(shell)
        lab, _ = ndimage.label(np.pad(~shell, 1, constant_values=True))
        padded = lab == lab[0, 0, 0]
        assert np.array_equal(outside, padded[1:-1, 1:-1, 1:-1])
        assert not (outside & shell).any()
        edt = ndimage.distance_transform_edt(~padded)[1:-1, 1:-1, 1:-1]
        d2 = S.depth2(outside)
        assert d2.dtype == np.int32 and np.array_equal(d2, np.rint(edt * edt).astype(np.int32))
        assert np.array_equal(d2 == 0, outside)
        # the packing into row words round-trips
        assert np.array_equal(S.unwords(S.words(shell), R)[0], shell)


def test_named_masks_have_the_topology_they_are_named_for():
    for R in (8, 33):
        masks, st = C.fill_masks(R), C.fill_statements(R)
        assert st["empty"][1] == (0, 0, 0) and st["empty"][0].all()
        assert st["full"][1][0] == R ** 3 and st["full"][1][1] == 0 and not st["full"][0].any()
        inner = (R - 6) ** 3
        assert st["hollow"][1][1] == inner and st["holed"][1][1] == 0 and st["border"][1][1] == (R // 2 - 1) ** 3
        assert st["border"][1][2] > 0 and st["hollow"][1][2] == 0
        free = ~masks["corridor"]
        assert np.array_equal(st["corridor"][0], free) and free.sum() == (R - 1) + (R - 2)
    maze = C.fill_masks(C.MAZE_R)["maze"]
    assert (~maze).sum() == C.MAZE_PATH and np.array_equal(C.fill_statements(C.MAZE_R)["maze"][0], ~maze)
    # the path is one node wide: every free node has at most two free neighbours, and exactly two nodes (the mouth and the end) have one
    free = np.pad(~maze, 1, constant_values=False)
    near = sum(np.roll(free, s, a) for a in range(3) for s in (1, -1))[1:-1, 1:-1, 1:-1][~maze]
    assert near.max() == 2 and (near == 1).sum() == 2


def test_depth_cases():
    for R in (8, 64):
        d = C.depth_statements(R)
        z, y, x = np.meshgrid(*[np.arange(R)] * 3, indexing="ij")
        to_layer = np.minimum.reduce([z + 1, y + 1, x + 1, R - z, R - y, R - x]) ** 2
        assert np.array_equal(d["none"], to_layer)
        assert np.array_equal(d["single"], np.minimum(to_layer, z * z + y * y + x * x))
        assert d["single"][0, 0, 0] == 0 and d["single"].max() == ((R + 1) // 2) ** 2


def test_boxed_shell_equals_the_brute_force():
    for R, (pts, n, r) in ((8, C.shell_clouds()[2]), (33, C.shell_clouds()[7]), (33, C.shell_clouds()[8])):
        h = S.pitch(R)
        a = S.shell(pts[:n].numpy(), R, S.F32(-1.25), h, S.F32(r))
        assert np.array_equal(a, S.shell_full(pts[:n].numpy(), R, S.F32(-1.25), h, S.F32(r))) and a.any()
    pts, R, (lo, hi), r = C.lattice_cloud()
    h = S.pitch(R, lo, hi)
    assert float(h) == 1.0 / 16.0
    a = S.shell(pts.numpy(), R, S.F32(lo), h, S.F32(r))
    assert np.array_equal(a, S.shell_full(pts.numpy(), R, S.F32(lo), h, S.F32(r)))
    # the <= decides: nodes at exactly r from a point, and at no lesser distance from any other, exist
    c = S.nodes(R, lo, h).astype(np.float64)
    grid = np.stack(np.meshgrid(c, c, c, indexing="ij")[::-1], axis=-1).reshape(-1, 3)
    d2 = ((grid[:, None, :] - pts.numpy().astype(np.float64)[None]) ** 2).sum(axis=-1).min(axis=1).reshape(R, R, R)
    assert (d2 == r * r).any() and np.array_equal(a, d2 <= r * r)


def test_radius_clamp_and_field():
    h = S.pitch(64)
    assert S.clamp(0.01, h, 0.0) == S.F32(2.0) * h and S.clamp(0.01, h, -1.0) == S.F32(3.0) * h and S.clamp(0.5, h, 0.5) == S.F32(0.5)
    assert S.clamp(float("nan"), h, 0.5) == S.F32(1.5) * h
    r = S.radius(C.surface("sphere").numpy()[:5], h)
    assert r == S.F32(2.0) * h                                  # 5 points: nobody has 8 neighbours
    s, have = S.spacing(C.surface("sphere").numpy())
    assert have == 2048 and 0.08 < s < 0.13                     # sqrt(8 * 4 pi 0.64 / (2048 pi)) = 0.1 for a uniform sphere
    d2 = np.array([[[0, 1, 4, 5]]], np.int32)
    for inset in (-1.0, 0.0, 0.5):
        v = S.field(d2, h, S.clamp(0.01, h, inset), inset)
        assert v.dtype == np.float32 and v[0, 0, 0] == 0.0
        # with the clamp, a node one pitch deep is never inside (v <= 1) and one at the threshold distance of two pitches sits at it
        assert v[0, 0, 1] < 1.0 and abs(float(v[0, 0, 2]) - 1.0) < 1e-6 and v[0, 0, 3] > 1.0


@pytest.mark.parametrize("name,R,inset", C.CONDITIONS)
def test_conditions_hold_for_the_statement(name, R, inset):
    pts = C.surface(name).numpy()
    st = S.cloud_to_mesh(pts, R, None, 1.5, inset)
    fig = C.check_conditions(name, R, inset, st["vertices"], st["projected"], st["faces"], st["info"])
    print(f"{name} R {R} inset {inset}: radius {float(st['radius']):.4f} {fig}")
    if st["vertices"].shape[0]:
        assert np.isnan(st["gap"]).sum() == 0 and (st["gap"] < 1e-6).sum() == 0       # no vertex would be left out of the projection comparison


def test_tiny_clouds_give_empty_meshes():
    for pts in (np.zeros((0, 3), np.float32), C.surface("sphere").numpy()[:3]):
        st = S.cloud_to_mesh(pts, 32)
        assert st["vertices"].shape == (0, 3) and st["faces"].shape == (0, 3) and st["info"][1] == 0
