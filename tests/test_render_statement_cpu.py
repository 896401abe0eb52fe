"""The float64 statement of the renderer (tests/render_statement.py) against cases worked by hand, `orbit_view` against its definition, and the
share of pixels the general-position inputs of tests/test_gpu_render.py leave out of the comparison (asserted here, so the GPU test cannot hide
it).  No GPU."""
import numpy as np
import pytest

import render_statement as S

MARGIN = 1e-3            # pixels whose coverage margin or depth gap is below this many pixels are left out of the general-position comparison ...
MAX_LEFT_OUT = 0.03      # ... and at most this share of the pixels the statement covers may be


def px_view(height, width):
    """world = pixels, the origin at the image's top-left corner"""
    v = S.front_view(1.0, height, width)
    v[0, 3] = v[1, 3] = 0.0
    return v


def test_a_disc_of_radius_two_and_a_half_on_a_pixel_centre_covers_21_pixels():
    out = S.render_points(np.asarray([(4.5, 4.5, 1.0)]), px_view(9, 9), 9, 9, 2.5)
    want = np.zeros((9, 9), bool)
    want[2:7, 3:6] = want[3:6, 2:7] = True                                 # the 5 x 5 square without its corners: d2 = 8 > 6.25; (2, 1): d2 = 5
    assert int(want.sum()) == 21 and np.array_equal(out["ids"] >= 0, want)
    assert np.array_equal(out["depth"][want], np.ones(21)) and np.isinf(out["depth"][~want]).all()
    assert abs(out["cover_margin"][4, 4] - 2.5) < 1e-12 and abs(out["cover_margin"][4, 6] - 0.5) < 1e-12
    # the pole of the impostor faces the eye: n = (0, 0, -1), L = -l_z
    shade = 0.3 + 0.7 * -S.DEFAULT_LIGHT[2]
    assert np.array_equal(out["rgb"][4, 4], np.floor(255.0 * np.float32(S.DEFAULT_COLOR).astype(np.float64) * shade + 0.5).astype(np.uint8))
    assert np.array_equal(out["rgb"][0, 0], (255, 255, 255))
    # r = 0.5 covers the one pixel whose centre it sits on; on a pixel corner it covers none (d2 = 1/2 > 1/4)
    assert int((S.render_points(np.asarray([(4.5, 4.5, 1.0)]), px_view(9, 9), 9, 9, 0.5)["ids"] >= 0).sum()) == 1
    assert int((S.render_points(np.asarray([(4.0, 4.0, 1.0)]), px_view(9, 9), 9, 9, 0.5)["ids"] >= 0).sum()) == 0
    # dx = 2, dy = 1.5: d2 = 6.25 = r^2 exactly, covered
    assert S.render_points(np.asarray([(3.5, 4.0, 1.0)]), px_view(9, 9), 9, 9, 2.5)["ids"][5, 5] == 0


def test_top_left_ties_on_a_right_triangle_and_its_other_half():
    """Legs through the pixel centres of row 1 and column 1, the hypotenuse through the centres with i + j = 6: the top and left edges own their
    pixels, the hypotenuse belongs to the half whose inward normal points right; the two halves tile the 4 x 4 square exactly once."""
    v = np.asarray([(1.5, 1.5, 1.0), (5.5, 1.5, 1.0), (1.5, 5.5, 1.0), (5.5, 5.5, 1.0)])
    i, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    upper = (i >= 1) & (j >= 1) & (i + j < 6)
    lower = (i <= 4) & (j <= 4) & (i + j >= 6)
    assert int(upper.sum()) == 10 and int(lower.sum()) == 6
    for order in ((0, 1, 2), (1, 2, 0), (2, 1, 0)):                          # either winding, any first vertex
        assert np.array_equal(S.render_mesh(v, [order], px_view(8, 8), 8, 8)["ids"] >= 0, upper)
    for order in ((1, 3, 2), (2, 3, 1)):
        assert np.array_equal(S.render_mesh(v, [order], px_view(8, 8), 8, 8)["ids"] >= 0, lower)
    both = S.render_mesh(v, [(0, 1, 2), (1, 3, 2)], px_view(8, 8), 8, 8)
    assert np.array_equal(both["ids"], np.where(upper, 0, np.where(lower, 1, -1)))
    assert both["cover_margin"][1, 1] == 0.0 and both["cover_margin"][3, 3] == 0.0 and both["cover_margin"][2, 2] == 1.0


def test_equal_depth_goes_to_the_lower_index_whatever_the_order():
    v = np.asarray([(0.5, 0.5, 2.0), (6.5, 0.5, 2.0), (0.5, 6.5, 2.0), (7.0, 7.0, 2.0)])
    a = S.render_mesh(v, [(0, 1, 2), (1, 3, 2), (0, 1, 2)], px_view(8, 8), 8, 8)
    assert set(np.unique(a["ids"]).tolist()) == {-1, 0, 1} and (a["depth"][a["ids"] >= 0] == 2.0).all()
    assert (a["depth_gap"][a["ids"] == 0] == 0.0).all() and np.isinf(a["depth_gap"][a["ids"] == 1]).all()
    b = S.render_mesh(v, [(1, 3, 2), (0, 1, 2), (0, 1, 2)], px_view(8, 8), 8, 8)
    assert np.array_equal(b["ids"] == 1, a["ids"] == 0) and not (b["ids"] == 2).any()
    p = S.render_points(np.asarray([(3.5, 3.5, 1.0), (4.5, 3.5, 1.0), (3.5, 3.5, 1.0), (4.0, 4.0, 0.5)]), px_view(8, 8), 8, 8, 1.5)
    assert not (p["ids"] == 2).any() and p["ids"][3, 2] == 0 and p["ids"][3, 5] == 1 and p["ids"][3, 3] == 3
    # a nearer primitive wins whatever its index; -0 and +0 are one depth
    z = S.render_points(np.asarray([(3.5, 3.5, 0.0), (3.5, 3.5, -0.0)]), px_view(8, 8), 8, 8, 1.5)
    assert not (z["ids"] == 1).any()


def test_what_draws_nothing():
    nan = float("nan")
    v = np.asarray([(1.0, 1.0, 1.0), (3.0, 3.0, 1.0), (5.0, 5.0, 2.0), (6.0, 1.0, 1.0), (nan, 2.0, 1.0)])
    for face in ((0, 1, 2), (0, 1, 1), (0, 3, 5), (0, 3, -1), (0, 3, 4)):   # collinear, repeated vertex, index past the rows, negative, NaN
        assert (S.render_mesh(v, [face], px_view(8, 8), 8, 8)["ids"] == -1).all(), face
    assert (S.render_points(np.asarray([(nan, 1.0, 1.0), (1.0, 1.0, float("inf")), (30.0, 1.0, 1.0)]), px_view(8, 8), 8, 8, 2.0)["ids"] == -1).all()


def test_the_fp32_form_decides_the_lattice_as_float64_does():
    view = S.front_view(8.0, 48, 64)
    v, f = S.lattice_mesh()
    a, b = S.render_mesh(v, f, view, 48, 64), S.render_mesh(v, f, view, 48, 64, dtype=np.float32)
    assert np.array_equal(a["ids"], b["ids"]) and b["depth"].dtype == np.float32
    assert sorted(set(np.unique(a["ids"]).tolist())) == [-1, 0, 1, 2, 6, 7, 8]
    assert a["ids"][30, 14] == 6 and a["cover_margin"][30, 14] > 1.0                        # inside both coplanar triangles: 6 wins
    for r in (2.5, 0.5):
        a, b = S.render_points(S.lattice_points(), view, 48, 64, r), S.render_points(S.lattice_points(), view, 48, 64, r, dtype=np.float32)
        assert np.array_equal(a["ids"], b["ids"]) and not (a["ids"] == 9).any() and not (a["ids"] >= 7).any()
    assert int((a["ids"] >= 0).sum()) == 6            # r = 1/2: a disc on a pixel centre owns that pixel, the one half way between two both (d2 = r^2)


def test_orbit_view_is_an_orthonormal_frame_scaled_to_the_image():
    from shapegen_amd import utils
    for azim, elev, h, w, half, center in ((-60, 30, 48, 64, 1.0, (0, 0, 0)), (35, 20, 136, 160, 1.5, (0.2, -0.1, 0.3)), (0, 90, 32, 32, 1.0, (0, 0, 0))):
        view = utils.orbit_view(azim, elev, h, w, half, center)
        assert view.dtype.is_floating_point and view.dtype.itemsize == 4 and tuple(view.shape) == (3, 4)
        m, t = view.numpy().astype(np.float64)[:, :3], view.numpy().astype(np.float64)[:, 3]
        s = min(h, w) / (2.0 * half)
        assert np.allclose(m @ m.T, s * s * np.eye(3), atol=1e-4 * s * s)
        assert np.allclose(m @ np.asarray(center) + t, (w / 2.0, h / 2.0, 0.0), atol=1e-4)
        assert np.allclose(np.cross(m[0], m[1]), s * m[2], atol=1e-4 * s * s)               # x right, y down, z away: right-handed
        a, e = np.deg2rad(azim), np.deg2rad(elev)
        assert np.allclose(-m[2] / s, (np.cos(a) * np.cos(e), np.sin(a) * np.cos(e), np.sin(e)), atol=1e-6)   # the eye sits towards (azim, elev)
        assert m[1] @ (0.0, 0.0, 1.0) <= 1e-6                                               # world z is up: it projects to -y
    turn = utils.orbit_views(4, 30.0, 48, 64)
    assert tuple(turn.shape) == (4, 3, 4) and np.array_equal(turn[0].numpy(), utils.orbit_view(-60.0, 30.0, 48, 64).numpy())
    assert np.allclose(turn[2].numpy()[0, :3], -turn[0].numpy()[0, :3], atol=1e-4)            # half a turn on: right is reversed
    with pytest.raises(ValueError):
        utils.orbit_views(0, 30.0, 48, 64)
    with pytest.raises(ValueError):
        utils.orbit_view(0.0, 0.0, 48, 64, half_extent=0.0)


def _views(h, w):
    from shapegen_amd import utils
    shared = np.stack([utils.orbit_view(a, e, h, w).numpy() for a, e in S.VIEW_ANGLES])
    own = np.stack([np.stack([utils.orbit_view(a + 25.0 * b, e, h, w).numpy() for a, e in S.VIEW_ANGLES]) for b in range(3)])
    return shared, own


def test_the_general_position_inputs_leave_out_at_most_three_percent():
    """For every input the GPU test compares against the statement: the share of covered pixels within 1e-3 px of a coverage boundary or of a
    depth tie is at most 3 %, and something is covered at all."""
    worst = 0.0
    for name, case in S.general_cases().items():
        shared, _ = _views(case[2], case[3])
        out = S.render_case(case, shared[0])
        keep, share = S.comparable(out, MARGIN)
        covered = int((out["ids"] >= 0).sum())
        print(f"{name}: covered {covered} of {out['ids'].size}, left out {share:.4%}")
        assert covered > 0.1 * out["ids"].size and share <= MAX_LEFT_OUT, (name, covered, share)
        worst = max(worst, share)
    meshes, clouds, radius = S.ragged_batch()
    shared, own = _views(48, 64)
    for b in (0, 2):
        for views in (shared, own[b]):
            for k in range(3):
                for out in (S.render_mesh(meshes[b][0], meshes[b][1], views[k], 48, 64), S.render_points(clouds[b], views[k], 48, 64, radius)):
                    keep, share = S.comparable(out, MARGIN)
                    assert (out["ids"] >= 0).any() and share <= MAX_LEFT_OUT, (b, k, share)
                    worst = max(worst, share)
    print(f"worst share left out: {worst:.4%}")
