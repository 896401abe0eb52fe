"""The renderer on the GPU (csrc/render.hip through `utils.render_point_clouds`, `render_meshes`, `render_voxels`) against the float64 statement
(tests/render_statement.py): the exact lattice, watertightness, general position, depth and colour, repeatability and the Python surface.

Exact lattice: front view with 8 px per unit at 48 x 64, coordinates multiples of 1/16, so projected coordinates are multiples of 1/2 below 64 and
every product of a coverage predicate fits 24 bits: fp32 decides each tie as float64 does and `ids` are equal pixel for pixel, nothing left out.

Watertightness (azim 35, elev 20), no statement involved.  A fan of 8 triangles that faces the eye: rendered one at a time their masks are
pairwise disjoint and their union is the mask of the whole fan.  A closed surface-nets mesh of a 5^3 blob: front and back sheets overlap on the
screen, so "disjoint" takes the form it has for a closed oriented surface -- at every pixel as many front-facing as back-facing triangles cover
it (no pixel lost along a shared edge, none claimed twice), and the union is the mask of the whole mesh.

General position: pixels whose statement margins (distance to a coverage boundary, gap to the second-nearest depth) are below 1e-3 px are left out;
the bound for fp32 projection plus edge evaluation at 512-px extents is about 1.2e-4 px.  At most 3 % of the covered pixels may be left out (the
shares are asserted on the CPU, in test_render_statement_cpu.py; the worst is 1.1 %).  Elsewhere `ids` are equal.

Depth and colour, where `ids` agree: the depth tolerance is 4 x the worst deviation of the statement run in float32 on the CPU from the float64
one on the same inputs (the factor allows another legitimate order of evaluation).  Recorded: the fp32 statement deviates from float64 by at
most 1.7e-6 px (pts300), 7.9e-6 px (pts2048), 9.6e-5 px (tri40) and 9.6e-5 px (tri300), so the tolerances are 6.8e-6, 3.1e-5, 3.8e-4 and 3.9e-4 px;
the device's own deviation from float64, recorded on an MI355X, is 1.7e-6, 7.9e-6, 9.6e-5 and 9.6e-5 px -- the fp32 statement's to the digit,
as the device evaluates the same fp32 operations in the same order (each test prints both figures).  rgb may differ by one level in at most 1 %
of the pixels (recorded: none for the triangles, 0.02 % for pts2048).

The statements run once per module and are left unchanged."""
import numpy as np
import pytest
import torch

import render_statement as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MARGIN = 1e-3
MAX_LEFT_OUT = 0.03
AZIM, ELEV = 35.0, 20.0


def dev_mesh(mesh):
    from shapegen_amd.utils import Mesh
    v, f = mesh
    return Mesh(torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda())


def dev_cloud(points):
    return torch.from_numpy(np.ascontiguousarray(points, np.float32)).cuda()


def views_of(h, w):
    from shapegen_amd import utils
    shared = torch.stack([utils.orbit_view(a, e, h, w) for a, e in S.VIEW_ANGLES])
    own = torch.stack([torch.stack([utils.orbit_view(a + 25.0 * b, e, h, w) for a, e in S.VIEW_ANGLES]) for b in range(3)])
    return shared, own


def gpu_meshes(meshes, views, h, w, **kw):
    from shapegen_amd.utils import render_meshes
    rgb, ids, depth = render_meshes([dev_mesh(m) for m in meshes], views, h, w, return_buffers=True, **kw)
    v = 1 if torch.as_tensor(views).dim() == 2 else torch.as_tensor(views).shape[-3]
    assert rgb.dtype == torch.uint8 and ids.dtype == torch.int32 and depth.dtype == torch.float32 and rgb.is_cuda
    assert tuple(rgb.shape) == (len(meshes), v, h, w, 3) and tuple(ids.shape) == tuple(depth.shape) == (len(meshes), v, h, w)
    return dict(rgb=rgb.cpu().numpy(), ids=ids.cpu().numpy(), depth=depth.cpu().numpy())


def gpu_points(clouds, views, h, w, radius, **kw):
    from shapegen_amd.utils import render_point_clouds
    rgb, ids, depth = render_point_clouds([dev_cloud(c) for c in clouds], views, h, w, radius, return_buffers=True, **kw)
    assert rgb.dtype == torch.uint8 and ids.dtype == torch.int32 and depth.dtype == torch.float32 and rgb.is_cuda
    return dict(rgb=rgb.cpu().numpy(), ids=ids.cpu().numpy(), depth=depth.cpu().numpy())


def gpu_case(case, view):
    kind, data, h, w, radius = case
    out = gpu_meshes([data], view, h, w) if kind == "mesh" else gpu_points([data], view, h, w, radius)
    return {k: a[0, 0] for k, a in out.items()}


def check_background(got):
    bg = got["ids"] < 0
    assert np.isinf(got["depth"][bg]).all() and (got["depth"][bg] > 0).all() and (got["rgb"][bg] == 255).all()
    assert np.isfinite(got["depth"][~bg]).all()


# ------------------------------------------------------------------ 1. the exact lattice
def test_exact_lattice_mesh():
    view = S.front_view(8.0, 48, 64)
    v, f = S.lattice_mesh()
    assert np.array_equal(np.round(v[np.isfinite(v)] * 16.0), v[np.isfinite(v)] * 16.0)
    want = S.render_mesh(v, f, view, 48, 64)
    got = {k: a[0, 0] for k, a in gpu_meshes([(v, f)], torch.from_numpy(view), 48, 64).items()}
    assert sorted(set(np.unique(want["ids"]).tolist())) == [-1, 0, 1, 2, 6, 7, 8]       # zero area, bad index and NaN draw nothing; 6 hides part of 7
    assert (want["cover_margin"] == 0.0).sum() >= 40                                     # edges through pixel centres: the ties are there
    assert np.array_equal(got["ids"], want["ids"])
    check_background(got)
    flat = np.isin(want["ids"], (0, 6, 7))                                               # constant depth: exact
    assert np.array_equal(got["depth"][flat], want["depth"][flat].astype(np.float32))
    drawn = want["ids"] >= 0
    assert np.abs(got["depth"][drawn] - want["depth"][drawn]).max() <= 1e-5
    assert np.abs(got["rgb"].astype(int) - want["rgb"].astype(int)).max() <= 1


@pytest.mark.parametrize("radius", [2.5, 0.5])
def test_exact_lattice_points(radius):
    view = S.front_view(8.0, 48, 64)
    p = S.lattice_points()
    want = S.render_points(p, view, 48, 64, radius)
    got = {k: a[0, 0] for k, a in gpu_points([p], torch.from_numpy(view), 48, 64, radius).items()}
    assert np.array_equal(got["ids"], want["ids"]) and (want["ids"] >= 0).any() and not (want["ids"] >= 7).any()
    check_background(got)
    assert np.array_equal(got["depth"], want["depth"].astype(np.float32))                # depths are lattice values: exact
    assert np.abs(got["rgb"].astype(int) - want["rgb"].astype(int)).max() <= 1


# ------------------------------------------------------------------ 2. watertightness
def one_at_a_time(mesh, view, h, w):
    """masks [F][H][W] of the triangles rendered alone (one shape per triangle, one launch), and the mask of the whole mesh"""
    v, f = mesh
    alone = gpu_meshes([(v, f[k:k + 1]) for k in range(f.shape[0])], view, h, w)["ids"][:, 0]
    assert set(np.unique(alone).tolist()) <= {-1, 0}
    whole = gpu_meshes([mesh], view, h, w)["ids"][0, 0]
    return alone >= 0, whole >= 0


def test_fan_is_watertight():
    from shapegen_amd.utils import orbit_view
    view = orbit_view(AZIM, ELEV, 48, 64)
    masks, whole = one_at_a_time(S.fan(AZIM, ELEV), view, 48, 64)
    assert masks.shape[0] == 8 and all(m.sum() > 20 for m in masks)
    assert masks.sum(axis=0).max() == 1, "two triangles of the fan claim one pixel"
    assert np.array_equal(masks.any(axis=0), whole), "a pixel of the fan is lost along a shared edge"
    filled = whole[1:-1, 1:-1] | ~(whole[:-2, 1:-1] & whole[2:, 1:-1] & whole[1:-1, :-2] & whole[1:-1, 2:])
    assert filled.all(), "a hole one pixel wide inside the fan"


def test_closed_surface_nets_mesh_is_watertight():
    from shapegen_amd.utils import orbit_view, voxel_tensor_to_meshes
    grid = torch.zeros(1, 1, 5, 5, 5)
    grid[0, 0, 1:4, 1:4, 1:4] = 1.0
    grid[0, 0, 2, 2, 0] = grid[0, 0, 2, 2, 4] = grid[0, 0, 0, 2, 2] = grid[0, 0, 2, 4, 1:4] = 1.0       # bumps: not convex
    mesh = voxel_tensor_to_meshes(grid.cuda(), 0.5)[0]
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    assert f.shape[0] > 100
    view = orbit_view(AZIM, ELEV, 48, 64, half_extent=1.7)
    masks, whole = one_at_a_time((v, f), view, 48, 64)
    q = S.project(view.numpy(), v)[f]
    nz = (q[:, 1, 0] - q[:, 0, 0]) * (q[:, 2, 1] - q[:, 0, 1]) - (q[:, 1, 1] - q[:, 0, 1]) * (q[:, 2, 0] - q[:, 0, 0])
    assert (np.abs(nz) > 1e-3).all()                                                     # no triangle is edge-on in this view
    front, back = masks[nz < 0].sum(axis=0), masks[nz > 0].sum(axis=0)
    assert front.max() >= 2                                                              # the bumps hide part of the body: sheets do overlap
    assert np.array_equal(front, back), "a ray enters the closed surface more or less often than it leaves it"
    assert np.array_equal(masks.any(axis=0), whole) and whole.sum() > 500


# ------------------------------------------------------------------ 3., 4. general position, depth and colour
@pytest.fixture(scope="module")
def general_reference():
    out = {}
    for name, case in S.general_cases().items():
        view = views_of(case[2], case[3])[0][0]
        out[name] = (case, view, S.render_case(case, view.numpy()), S.render_case(case, view.numpy(), dtype=np.float32))
    return out




def compare(got, want, want32, what):
    keep, share = S.comparable(want, MARGIN)
    assert share <= MAX_LEFT_OUT, (what, share)
    wrong = keep & (got["ids"] != want["ids"])
    assert not wrong.any(), (what, int(wrong.sum()), np.argwhere(wrong)[:5].tolist())
    check_background(got)
    same = keep & (want["ids"] >= 0) & (want32["ids"] == want["ids"])
    assert same.any(), (what, "no comparable covered pixel: the depth and colour checks would not run")
    ref = want["depth"][same]
    tol = 4.0 * float(np.abs(want32["depth"][same].astype(np.float64) - ref).max())
    dev = float(np.abs(got["depth"][same].astype(np.float64) - ref).max())
    print(f"{what}: left out {share:.3%}; depth: 4 x fp32 statement {tol:.3e} px, device {dev:.3e} px")
    assert dev <= tol, (what, dev, tol)
    level = np.abs(got["rgb"].astype(int) - want["rgb"].astype(int)).max(axis=-1)[same]
    print(f"{what}: rgb differs by one level in {np.mean(level > 0):.3%} of the pixels")
    assert level.max() <= 1 and np.mean(level > 0) <= 0.01, (what, int(level.max()), float(np.mean(level > 0)))
    return share


@pytest.mark.parametrize("name", ["tri40", "tri300", "pts300", "pts2048"])
def test_general_position_against_the_statement(general_reference, name):
    case, view, want, want32 = general_reference[name]
    assert (want["ids"] >= 0).sum() > 0.1 * want["ids"].size
    compare(gpu_case(case, view), want, want32, name)


def test_a_mesh_of_1025_triangles_against_the_statement():
    """One more triangle than a chunk of 1024: the last chunk holds triangle 1024 alone, and the statement sees it (the seed was chosen for that
    from the statement alone).  Margins and tolerances as for the other general-position cases."""
    case = ("mesh", S.random_triangles(1025, 29, 0.12), 48, 64, None)
    view = views_of(48, 64)[0][0]
    want, want32 = S.render_case(case, view.numpy()), S.render_case(case, view.numpy(), dtype=np.float32)
    assert (S.comparable(want, MARGIN)[0] & (want["ids"] == 1024)).sum() >= 5
    compare(gpu_case(case, view), want, want32, "tri1025")


@pytest.mark.parametrize("own_views", [False, True])
def test_ragged_batch_and_several_views(own_views):
    meshes, clouds, radius = S.ragged_batch()
    shared, own = views_of(48, 64)
    views = own if own_views else shared
    gm, gp = gpu_meshes(meshes, views, 48, 64), gpu_points(clouds, views, 48, 64, radius)
    assert gm["ids"].shape == gp["ids"].shape == (3, 3, 48, 64)
    for got in (gm, gp):                                                                  # the empty shape: background
        assert (got["ids"][1] == -1).all() and np.isinf(got["depth"][1]).all() and (got["rgb"][1] == 255).all()
    for b in (0, 2):
        for k in range(3):
            view = (own[b, k] if own_views else shared[k]).numpy()
            want = S.render_mesh(meshes[b][0], meshes[b][1], view, 48, 64), S.render_points(clouds[b], view, 48, 64, radius)
            want32 = (S.render_mesh(meshes[b][0], meshes[b][1], view, 48, 64, dtype=np.float32),
                      S.render_points(clouds[b], view, 48, 64, radius, dtype=np.float32))
            for got, w, w32, kind in ((gm, want[0], want32[0], "mesh"), (gp, want[1], want32[1], "points")):
                compare({key: a[b, k] for key, a in got.items()}, w, w32, f"ragged {kind} b{b} v{k} own={own_views}")


def test_style_and_a_width_that_is_no_multiple_of_four():
    """colour per shape, light, ambient, background; 30 x 37 takes the pixel-by-pixel stores"""
    from shapegen_amd.utils import orbit_view
    view = orbit_view(AZIM, ELEV, 30, 37)
    mesh, cloud = S.random_triangles(12, 31), S.random_points(60, 32)
    style = dict(light=(0.3, -0.5, -0.8), ambient=0.15, background=(0.1, 0.2, 0.3))
    colors = [(0.9, 0.4, 0.1), (0.2, 0.8, 0.6)]
    light = np.asarray(style["light"]) / np.linalg.norm(style["light"])
    gm = gpu_meshes([mesh, mesh], view, 30, 37, color=colors, **style)
    gp = gpu_points([cloud, cloud], view, 30, 37, 2.0, color=colors, **style)
    for b in range(2):
        kw = dict(color=colors[b], light=light, ambient=0.15, background=style["background"])
        for got, want in ((gm, S.render_mesh(mesh[0], mesh[1], view.numpy(), 30, 37, **kw)), (gp, S.render_points(cloud, view.numpy(), 30, 37, 2.0, **kw))):
            keep, _ = S.comparable(want, MARGIN)
            assert np.array_equal(got["ids"][b, 0][keep], want["ids"][keep]) and (want["ids"] >= 0).any()
            assert (got["rgb"][b, 0][got["ids"][b, 0] < 0] == want["rgb"][want["ids"] < 0][0]).all()
            same = keep & (want["ids"] >= 0)
            level = np.abs(got["rgb"][b, 0].astype(int) - want["rgb"].astype(int)).max(axis=-1)[same]
            assert level.max() <= 1 and np.mean(level > 0) <= 0.01
    assert not np.array_equal(gm["rgb"][0], gm["rgb"][1]) and np.array_equal(gm["ids"][0], gm["ids"][1])


# ------------------------------------------------------------------ 5. repeatability and independence
def test_repeatable_independent_of_the_batch_and_of_the_tile_shape():
    from shapegen_amd import _lib
    lib = _lib.load()
    cases = S.general_cases()
    meshes, clouds, radius = S.ragged_batch()
    shared, own = views_of(136, 160)
    meshes = meshes + [cases["tri300"][1]]
    clouds = clouds + [cases["pts2048"][1]]
    own = torch.cat([own, own[:1]])

    def run():
        return gpu_meshes(meshes, own, 136, 160), gpu_points(clouds, own, 136, 160, radius)

    first = run()
    again = run()
    try:
        assert lib.pcd_render_config(0) == 0
        flat = run()
        assert lib.pcd_render_config(1) == 0
        tall = run()
    finally:
        assert lib.pcd_render_config(2) == 0                             # the default: the tile follows the size of the launch
    assert lib.pcd_render_config(3) == -1 and lib.pcd_render_config(-1) == -1
    for a, b, c, d in zip(first, again, flat, tall):
        for key in ("ids", "depth", "rgb"):
            assert np.array_equal(a[key], b[key]), f"two calls differ in {key}"
            assert np.array_equal(a[key], c[key]), f"the 128 x 64 tile differs from the default in {key}"
            assert np.array_equal(c[key], d[key]), f"the 128 x 128 tile differs from the 128 x 64 tile in {key}"
        assert (a["ids"][3] >= 0).sum() > 1000
    for b in (0, 3):
        alone = gpu_meshes([meshes[b]], own[b], 136, 160), gpu_points([clouds[b]], own[b], 136, 160, radius)
        for a, one in zip(first, alone):
            for key in ("ids", "depth", "rgb"):
                assert np.array_equal(a[key][b], one[key][0]), f"shape {b} alone differs from its images in the batch in {key}"


# ------------------------------------------------------------------ 6. the Python surface
def test_render_voxels_is_render_meshes_of_the_surface_nets_meshes():
    from shapegen_amd import utils
    g = torch.Generator().manual_seed(5)
    grid = (torch.rand(2, 1, 8, 8, 8, generator=g) > 0.6).float().cuda()
    views = utils.orbit_views(2, 30.0, 40, 48, half_extent=1.4)
    a = utils.render_voxels(grid, views, 0.5, height=40, width=48, color=(0.8, 0.3, 0.3))
    b = utils.render_meshes(utils.voxel_tensor_to_meshes(grid, 0.5), views, 40, 48, color=(0.8, 0.3, 0.3))
    assert tuple(a.shape) == (2, 2, 40, 48, 3) and torch.equal(a, b) and bool((a != 255).any())


def test_null_outputs_are_skipped():
    from shapegen_amd import _lib, utils
    lib = _lib.load()
    cloud = dev_cloud(S.random_points(100, 41))
    view = utils.orbit_view(AZIM, ELEV, 32, 40).cuda().contiguous()
    offsets = torch.tensor([0, 100], dtype=torch.int64).cuda()
    style = _lib.RenderStyle(None, (_lib.f32 * 3)(*S.DEFAULT_LIGHT), 0.3, (_lib.f32 * 3)(1.0, 1.0, 1.0))
    full = [torch.full((32, 40), -7, dtype=torch.int32).cuda(), torch.full((32, 40), -7.0).cuda(), torch.full((32, 40, 3), 7, dtype=torch.uint8).cuda()]

    def call(ids, depth, rgb):
        _lib.check(lib.pcd_render_points(cloud.data_ptr(), offsets.data_ptr(), 1, view.data_ptr(), 1, 1, 32, 40, 2.0, style, _lib.ptr(ids),
                                         _lib.ptr(depth), _lib.ptr(rgb), _lib.stream_ptr()), "render_points")
        torch.cuda.synchronize()

    call(*full)
    assert bool((full[0] >= 0).any()) and not bool((full[1] == -7.0).any())
    for skip in range(3):
        bufs = [torch.full_like(t, 9) for t in full]
        call(*[None if k == skip else t for k, t in enumerate(bufs)])
        for k in range(3):
            assert torch.equal(bufs[k], torch.full_like(full[k], 9) if k == skip else full[k]), (skip, k)
    call(None, None, None)
    # the default colour of a null `colors` is the Python default
    assert torch.equal(full[2], utils.render_point_clouds([cloud], view, 32, 40, 2.0)[0, 0])


def test_image_grid_and_the_refusals():
    from shapegen_amd import utils
    cloud = dev_cloud(S.random_points(50, 42))
    views = utils.orbit_views(5, 20.0, 16, 24)
    im = utils.render_point_clouds([cloud, cloud], views, 16, 24)
    assert tuple(im.shape) == (2, 5, 16, 24, 3)
    sheet = utils.image_grid(im, 4)
    assert tuple(sheet.shape) == (3 * 16, 4 * 24, 3) and sheet.is_cuda and sheet.dtype == torch.uint8
    assert torch.equal(sheet[16:32, 24:48], im[1, 0]) and torch.equal(sheet[32:48, 0:24], im[1, 3]) and bool((sheet[32:, 48:] == 255).all())
    padded = utils.image_grid(im[0], 2, pad=3, background=(0.0, 0.0, 0.0))
    assert tuple(padded.shape) == (3 * 16 + 2 * 3, 2 * 24 + 3, 3) and bool((padded[16:19] == 0).all()) and torch.equal(padded[19:35, 27:51], im[0, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.render_point_clouds([cloud.cpu()], views, 16, 24)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.render_meshes([dev_mesh(S.random_triangles(2, 1))._replace(vertices=torch.zeros(6, 3))], views, 16, 24)
    for bad in (dict(height=0), dict(width=2049), dict(radius=0.0), dict(radius=65.0), dict(ambient=1.5), dict(color=(2.0, 0.0, 0.0)),
                dict(light=(0.0, 0.0, 0.0)), dict(background=(0.5, 0.5)), dict(views=torch.zeros(3, 3)), dict(views=torch.zeros(3, 5, 3, 4))):
        kw = dict(views=views, height=16, width=24)
        kw.update(bad)
        with pytest.raises(ValueError):
            utils.render_point_clouds([cloud, cloud], **kw)
    with pytest.raises(ValueError):
        utils.image_grid(im.float(), 2)
