"""The host side of the renderer: the PNG writer (decoded here with zlib alone), the contact sheet, and the refusals of the entry points and of
the Python functions that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_statement as S


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (3, 5), (48, 64)])
def test_save_png_round_trip(tmp_path, size):
    from shapegen_amd.utils import save_png
    h, w = size
    image = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    for k, src in enumerate((image, torch.from_numpy(image))):
        path = tmp_path / "deep" / f"{k}.png"                            # the directory is made
        save_png(str(path), src)
        data = path.read_bytes()
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[-8:-4] == b"IEND"
        back = S.decode_png(data)                                        # checks every chunk's CRC, the header fields and the filter bytes
        assert back.shape == (h, w, 3) and np.array_equal(back, image)


def test_save_png_refuses_what_it_does_not_write(tmp_path):
    from shapegen_amd.utils import save_png
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            save_png(str(tmp_path / "x.png"), bad)
    assert not (tmp_path / "x.png").exists()


def test_image_grid_on_the_host():
    from shapegen_amd.utils import image_grid
    im = torch.arange(5 * 2 * 3 * 3, dtype=torch.uint8).reshape(5, 2, 3, 3)
    sheet = image_grid(im, 3)
    assert tuple(sheet.shape) == (4, 9, 3) and torch.equal(sheet[0:2, 3:6], im[1]) and torch.equal(sheet[2:4, 3:6], im[4])
    assert bool((sheet[2:4, 6:9] == 255).all())
    assert tuple(image_grid(im, 5, pad=1).shape) == (2, 5 * 3 + 4, 3) and tuple(image_grid(im[0], 1).shape) == (2, 3, 3)
    for bad in (dict(images=im.float(), cols=2), dict(images=im, cols=0), dict(images=im[..., :2], cols=2), dict(images=im[:0], cols=2)):
        with pytest.raises(ValueError):
            image_grid(**bad)


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    from shapegen_amd import _lib
    lib = _lib.load()
    style = _lib.RenderStyle(None, (_lib.f32 * 3)(0.0, 0.0, -1.0), 0.3, (_lib.f32 * 3)(1.0, 1.0, 1.0))
    p = 64                                                               # never dereferenced on the host

    def points(points=p, offsets=p, batch=2, views=p, view_sets=1, n_views=1, height=32, width=32, radius=1.5, style=style):
        return lib.pcd_render_points(points, offsets, batch, views, view_sets, n_views, height, width, radius, style, p, p, p, None)

    def meshes(vertices=p, faces=p, offsets=p, batch=2, views=p, view_sets=2, n_views=1, height=32, width=32, style=style):
        return lib.pcd_render_meshes(vertices, faces, offsets, batch, views, view_sets, n_views, height, width, style, p, p, p, None)

    bad = [dict(height=0), dict(height=2049), dict(width=0), dict(width=2049), dict(n_views=0), dict(view_sets=0), dict(view_sets=3), dict(batch=0),
           dict(points=None), dict(offsets=None), dict(views=None), dict(style=None), dict(radius=0.0), dict(radius=-1.0), dict(radius=64.5),
           dict(radius=float("nan"))]
    for kw in bad:
        assert points(**kw) == -1 and b"bad argument" in lib.pcd_last_error(), kw
    for kw in bad:
        if "radius" in kw:
            continue
        kw = {("vertices" if k == "points" else k): v for k, v in kw.items()}
        assert meshes(**kw) == -1 and b"bad argument" in lib.pcd_last_error(), kw
    assert meshes(faces=None) == -1
    dim = _lib.RenderStyle(None, (_lib.f32 * 3)(0.0, 0.0, -1.0), 1.5, (_lib.f32 * 3)(1.0, 1.0, 1.0))
    assert points(style=dim) == -1
    assert lib.pcd_render_config(0) == 0 and lib.pcd_render_config(2) == 0 and lib.pcd_render_config(3) == -1 and lib.pcd_render_config(-1) == -1
    assert C.sizeof(_lib.RenderStyle) == 40                              # pointer, 3 + 1 + 3 floats, padded to the pointer's alignment


def test_python_refusals_without_a_device():
    from shapegen_amd import utils
    cloud = torch.zeros(10, 3)
    views = utils.orbit_views(2, 30.0, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.render_point_clouds([cloud], views, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.render_point_clouds(torch.zeros(2, 10, 3), views, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.render_meshes([(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))], views, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.render_voxels(torch.zeros(1, 1, 4, 4, 4), views)
    for bad in ([], torch.zeros(10, 3), [torch.zeros(10, 2)]):
        with pytest.raises(ValueError):
            utils.render_point_clouds(bad, views, 16, 16)
    with pytest.raises(ValueError):
        utils.render_meshes([], views, 16, 16)
    assert tuple(utils.axis_views(16, 24).shape) == (3, 3, 4)
