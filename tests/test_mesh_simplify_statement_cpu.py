"""The numpy statement of DESIGN.md "Mesh simplification" (tests/mesh_simplify_statement.py) against what must hold whatever the numbers
are: closed meshes stay closed, a grid with one vertex per cell is compaction, the bisection keeps its promise, quadric placement keeps
the volume better than the cell mean, and `deduplicate` removes exactly the repeated faces."""
import functools

import numpy as np
import pytest

import mesh_ops_statement as S
import mesh_simplify_cases as C
import mesh_simplify_statement as Q

RESOLUTIONS = (1, 2, 3, 4, 8, 16, 32)


@functools.lru_cache(maxsize=None)
def simplified(name, r, placement="quadric", deduplicate=False):
    return Q.simplify(*C.case(name), resolution=r, placement=placement, deduplicate=deduplicate)


@pytest.mark.parametrize("name", C.CLOSED)
def test_closed_meshes_stay_closed(name):
    assert S.measures(*C.case(name))["closed"] == 1
    for r in RESOLUTIONS:
        out = simplified(name, r)
        m = S.measures(out["vertices"], out["faces"])
        assert m["closed"] == 1, (name, r)
        assert out["faces"].min(initial=0) >= 0 and out["faces"].max(initial=-1) < out["vertices"].shape[0]
    assert simplified(name, 1)["faces"].shape[0] == 0 and simplified(name, 1)["vertices"].shape[0] == 1


def test_the_plate_collapses_and_the_flat_patch_falls_back_to_the_mean():
    v, f = C.case("thin_plate")
    assert S.measures(v, f)["euler"] == 2
    out = simplified("thin_plate", 8)                                        # both sheets in one layer of 8 x 8 cells (the last row clamps)
    assert out["vertices"].shape[0] == 64 and S.measures(out["vertices"], out["faces"])["closed"] == 1
    flat = simplified("flat_patch", 2)
    assert np.array_equal(flat["vertices"][:, 2], np.zeros(flat["vertices"].shape[0], np.float32))
    assert np.isfinite(flat["vertices"]).all()


@pytest.mark.parametrize("name", ["tetrahedron", "octahedron", "cube", "mixed", "bad_indices", "grid_patch", "icosphere_642",
                                  "non_finite_unreferenced"])
def test_one_vertex_per_cell_is_compaction(name):
    v, f = C.case(name)
    referenced = Q.box(v, f)[2]
    r = next((r for r in (2, 3, 4, 8, 16, 32, 64, 128, 256, 512, 1024) if Q.clusters(v, f, resolution=r)["roots"].size == referenced.sum()), None)
    assert r is not None, name
    wv, wf = S.compact(v, f, referenced)
    mean = Q.simplify(v, f, resolution=r, placement="mean")
    assert np.array_equal(mean["faces"], wf) and np.array_equal(mean["vertices"].view(np.uint32), wv.view(np.uint32))
    assert np.array_equal(mean["map"][referenced], np.arange(referenced.sum())) and np.all(mean["map"][~referenced] == -1)
    quad = Q.simplify(v, f, resolution=r, placement="quadric")
    assert np.array_equal(quad["faces"], wf)
    # A lone vertex lies on every plane of its quadric and is its own mean, so A' x = b' in exact arithmetic.  In fp64 the residual
    # res = A' x - b' is not 0, and the least eigenvalue of A' is at least the regulariser reg, so the exact solution of the rounded
    # system is within |res| / reg of x; Cramer's rule adds its own rounding, at most cond(A') <= 1003 times a few dozen fp64 roundings
    # (1e5 eps covers it), and the result is rounded to fp32 once (one spacing).
    info = quad["info"]
    x = wv.astype(np.float64)
    res = np.einsum("kij,kj->ki", info["A"], x) - info["b"]
    reg = 1e-3 * (np.trace(info["A"], axis1=1, axis2=2) / 1.003)
    bound = (np.linalg.norm(res, axis=1) / reg)[:, None] + 1e5 * 2.0 ** -53 * np.maximum(1.0, np.abs(x).max(axis=1))[:, None] + \
        np.spacing(np.abs(wv)).astype(np.float64)
    err = np.abs(quad["vertices"].astype(np.float64) - x)
    print(name, r, float(err.max()), float(bound.min()))
    assert np.all(err <= bound), name


TARGETS = (("icosphere_10242", 2000), ("icosphere_10242", 500), ("icosphere_642", 300), ("icosphere_642", 100), ("nets_sphere", 400),
           ("nets_sphere", 200), ("cube", 12), ("cube", 11), ("thin_plate", 150), ("tetrahedron", 0))


@pytest.mark.parametrize("name,target", TARGETS)
def test_the_bisection_keeps_its_promise(name, target):
    v, f = C.case(name)
    out = Q.simplify(v, f, target_faces=target)
    r = out["resolution"]
    print(name, target, r, out["faces"].shape[0])
    assert out["faces"].shape[0] <= target
    assert r == Q.MAX_R or Q.surviving(v, f, r + 1) > target
    assert out["faces"].shape[0] == simplified(name, r)["faces"].shape[0] if r <= 32 else True


@pytest.mark.parametrize("name", ["icosphere_642", "icosphere_10242", "nets_sphere"])
def test_quadric_placement_keeps_the_volume_better_than_the_mean(name):
    want = S.measures(*C.case(name))["volume"]
    for r in (4, 8, 16):
        quad, mean = simplified(name, r), simplified(name, r, "mean")
        vq, vm = S.measures(quad["vertices"], quad["faces"])["volume"], S.measures(mean["vertices"], mean["faces"])["volume"]
        print(name, r, want, vq, vm)
        assert abs(vq - want) < abs(vm - want), (name, r)


def test_deduplicate_removes_exactly_the_repeated_faces():
    cube_v, cube_f = C.case("cube")
    plain, dedup = simplified("doubled_cube", 2), simplified("doubled_cube", 2, "quadric", True)
    assert plain["faces"].shape[0] == 14 and np.array_equal(plain["faces"], C.case("doubled_cube")[1])
    assert np.array_equal(dedup["faces"], cube_f) and np.array_equal(dedup["map"], np.arange(8))
    assert np.array_equal(dedup["vertices"], plain["vertices"])
    rotated = (cube_v, np.concatenate([cube_f, cube_f[:1, [1, 2, 0]], cube_f[1:2, [0, 2, 1]]]))     # a rotation repeats, a reflection does not
    out = Q.simplify(*rotated, resolution=2, deduplicate=True)
    assert np.array_equal(out["faces"], np.concatenate([cube_f, cube_f[1:2, [0, 2, 1]]]))
