"""`geometry.cloud_to_meshes` and its stage wrappers on a machine without a GPU: they exist, refuse CPU tensors with the usual RuntimeError,
refuse every bad argument with a ValueError raised on the host, and the C entry points report PCD_ERR_ARG before any device work."""
import pytest
import torch


def _cloud():
    return torch.rand(2, 64, 3, generator=torch.Generator().manual_seed(0)) * 2 - 1


def test_cloud_to_meshes_refuses_cpu_tensors():
    from shapegen_amd import geometry
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.cloud_to_meshes(_cloud())
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.cloud_to_meshes([_cloud()[0]], resolution=16, radius=0.2, project=False, return_info=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.cloud_shell_grid(_cloud(), resolution=8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.cloud_radius(_cloud())
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.grid_outside(torch.zeros(1, 8, 8, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.grid_depth_field(torch.zeros(1, 8, 8, dtype=torch.int64), torch.ones(1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.project_to_cloud(_cloud(), _cloud())


@pytest.mark.parametrize("kwargs", [
    dict(resolution=7), dict(resolution=65), dict(resolution=32.0), dict(resolution=True),
    dict(bounds=(1.0, 1.0)), dict(bounds=(1.0, -1.0)), dict(bounds=(-1.0, float("inf"))), dict(bounds=(float("nan"), 1.0)), dict(bounds=1.0),
    dict(bounds=(-1.0, 0.0, 1.0)),
    dict(inset=1.5), dict(inset=-1.01), dict(inset=float("nan")), dict(inset="0"),
    dict(radius=0.0), dict(radius=-0.1), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius="0.1"),
    dict(radius=1.2500001), dict(radius=0.6, bounds=(-0.5, 0.5)),              # above (hi - lo) / 2: the shell costs N (r / h)^3
    dict(radius=torch.ones(2, 1)),
    dict(radius_scale=0.0), dict(radius_scale=-1.5), dict(radius_scale=float("inf")), dict(radius_scale=None),
    dict(k=0), dict(k=33), dict(k=8.0),
])
def test_cloud_to_meshes_refuses_bad_arguments_on_the_host(kwargs):
    """Before the clouds are looked at: a CPU tensor gets this far, and the library is not loaded."""
    from shapegen_amd import _lib, geometry
    loaded = _lib.load
    _lib.load = lambda: pytest.fail("the library was loaded before the arguments were checked")
    try:
        with pytest.raises(ValueError):
            geometry.cloud_to_meshes(_cloud(), **kwargs)
    finally:
        _lib.load = loaded


def test_stage_wrappers_refuse_bad_arguments():
    from shapegen_amd import geometry
    with pytest.raises(ValueError):
        geometry.cloud_to_meshes(torch.zeros(4, 3))                           # not (P, N, 3)
    with pytest.raises(ValueError):
        geometry.grid_outside(torch.zeros(1, 8, 8, dtype=torch.int32))
    with pytest.raises(ValueError):
        geometry.grid_outside(torch.zeros(1, 8, 9, dtype=torch.int64))
    with pytest.raises(ValueError):
        geometry.grid_outside(torch.zeros(1, 65, 65, dtype=torch.int64))
    with pytest.raises(ValueError):
        geometry.grid_depth_field(torch.zeros(2, 8, 8, dtype=torch.int64), torch.ones(3))
    with pytest.raises(ValueError):
        geometry.cloud_shell_grid(_cloud(), resolution=4)
    with pytest.raises(ValueError):
        geometry.project_to_cloud(_cloud(), _cloud(), k=0)


def test_entry_points_check_their_arguments_without_a_gpu():
    """PCD_ERR_ARG before any device work: pointers are never dereferenced on the host (64 stands for a valid one)."""
    from shapegen_amd import _lib
    lib = _lib.load()
    p, inf, nan = 64, float("inf"), float("nan")
    h = 2.5 / 63
    sp = lambda **kw: lib.pcd_cloud_spacing(*[{**dict(d2=p, counts=p, n=16, P=2, k=8, rin=None, scale=1.5, h=h, inset=0.0, out=p, s=None), **kw}[a]
                                              for a in ("d2", "counts", "n", "P", "k", "rin", "scale", "h", "inset", "out", "s")])
    for kw in (dict(out=None), dict(d2=None), dict(rin=p), dict(counts=None), dict(n=0), dict(P=0), dict(P=65536), dict(k=0), dict(k=33),
               dict(scale=0.0), dict(scale=nan), dict(h=0.0), dict(h=-h), dict(h=inf), dict(h=nan), dict(inset=1.5), dict(inset=-1.5),
               dict(inset=nan)):
        assert sp(**kw) == -1 and b"bad argument" in lib.pcd_last_error(), kw
    sf = lambda **kw: lib.pcd_cloud_shell_fill(*[{**dict(pts=p, counts=p, n=16, P=2, R=32, lo=-1.25, h=h, radii=p, shell=p, outside=p, info=p,
                                                         sweeps=None, s=None), **kw}[a]
                                                 for a in ("pts", "counts", "n", "P", "R", "lo", "h", "radii", "shell", "outside", "info", "sweeps", "s")])
    for kw in (dict(pts=None), dict(counts=None), dict(radii=None), dict(shell=None), dict(outside=None), dict(info=None), dict(n=0), dict(P=0),
               dict(P=65536), dict(R=7), dict(R=65), dict(lo=nan), dict(lo=inf), dict(h=0.0), dict(h=nan), dict(h=inf)):
        assert sf(**kw) == -1 and b"bad argument" in lib.pcd_last_error(), kw
    for args in ((None, 1, 8, p + 64, p, None, None), (p, 1, 8, None, p, None, None), (p, 1, 8, p + 64, None, None, None),
                 (p, 0, 8, p + 64, p, None, None), (p, 65536, 8, p + 64, p, None, None), (p, 1, 7, p + 64, p, None, None),
                 (p, 1, 65, p + 64, p, None, None), (p, 1, 8, p, p, None, None)):                 # the last: outside == shell
        assert lib.pcd_grid_fill_outside(*args) == -1, args
    for args in ((None, 1, 8, h, p, 0.0, None, p, None), (p, 1, 8, h, None, 0.0, None, p, None), (p, 1, 8, h, p, 0.0, None, None, None),
                 (p, 0, 8, h, p, 0.0, None, p, None), (p, 1, 66, h, p, 0.0, None, p, None), (p, 1, 8, 0.0, p, 0.0, None, p, None),
                 (p, 1, 8, nan, p, 0.0, None, p, None), (p, 1, 8, h, p, 1.25, None, p, None), (p, 1, 8, h, p, 0.0, p, p, None)):
        assert lib.pcd_grid_depth_field(*args) == -1, args
    for args in ((None, p, 4, p, p, 16, 1, p, 8, 1.0, 0.0, p, None), (p, None, 4, p, p, 16, 1, p, 8, 1.0, 0.0, p, None),
                 (p, p, 4, p, p, 16, 1, p, 8, 1.0, 0.0, None, None), (p, p, 0, p, p, 16, 1, p, 8, 1.0, 0.0, p, None),
                 (p, p, 4, p, p, 16, 0, p, 8, 1.0, 0.0, p, None), (p, p, 4, None, p, 16, 1, p, 8, 1.0, 0.0, p, None),
                 (p, p, 4, p, p, 0, 1, p, 8, 1.0, 0.0, p, None), (p, p, 4, p, p, 16, 1, p, 33, 1.0, 0.0, p, None),
                 (p, p, 4, None, None, 0, 1, None, 0, nan, 0.0, p, None), (p, p, 4, None, None, 0, 1, None, 0, 1.0, inf, p, None)):
        assert lib.pcd_project_to_cloud(*args) == -1, args
