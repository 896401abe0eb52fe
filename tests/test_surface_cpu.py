"""The boundary of the surface metrics without a GPU: the symbols are declared, exported and bound, the ABI version did not move, argument
errors come back before any device work, the column names, and CPU tensors raise."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"pcd_nearest_workspace_bytes": 3, "pcd_nearest_neighbors": 12, "pcd_surface_metrics_workspace_bytes": 3, "pcd_surface_metrics": 19,
       "pcd_voxel_iou": 7}


def _header():
    return open(os.path.join(ROOT, "include", "pcd_hip.h")).read()


def test_symbols_are_declared_exported_and_bound():
    from shapegen_amd import _lib
    _lib.build()
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, argc in NEW.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert proto, f"{name} is not declared in include/pcd_hip.h"
        assert len(proto.group(1).split(",")) == argc, name
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(_lib._SIGS[name][1]) == argc, name
    assert lib.pcd_abi_version() == _lib.ABI_VERSION == 2
    assert re.search(r"#define\s+PCD_ABI_VERSION\s+2\b", _header())


def test_row_constants_mirror_the_header():
    from shapegen_amd import _lib
    enum = re.search(r"enum\s*\{\s*(PCD_SURF_ROW_ACC[^}]*)\}", _header()).group(1)
    names = [n.split("=")[0].strip()[len("PCD_SURF_ROW_"):] for n in enum.split(",")]
    assert names[-1] == "BASE" and tuple(names[:-1]) == _lib.PCD_SURF_ROW
    assert _lib.PCD_SURF_ROW_BASE == 10 == len(_lib.PCD_SURF_ROW)
    assert int(re.search(r"#define\s+PCD_SURF_MAX_THRESHOLDS\s+(\d+)", _header()).group(1)) == _lib.PCD_SURF_MAX_THRESHOLDS == 8


def test_argument_errors_without_gpu():
    from shapegen_amd import _lib
    lib = _lib.load()
    p = 64                                                                    # never dereferenced on the host
    taus = (C.c_float * 8)(0.02, 0.04, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6)
    big = 1 << 30
    assert lib.pcd_nearest_workspace_bytes(3, 100, 50) >= 3 * 100 * 8
    assert lib.pcd_nearest_workspace_bytes(0, 100, 50) == 0 and lib.pcd_nearest_workspace_bytes(3, 0, 50) == 0
    assert lib.pcd_surface_metrics_workspace_bytes(3, 100, 50) >= 2 * 3 * 100 * 8
    assert lib.pcd_surface_metrics_workspace_bytes(3, 50, 100) == lib.pcd_surface_metrics_workspace_bytes(3, 100, 50)
    assert lib.pcd_surface_metrics_workspace_bytes(0, 100, 50) == 0 and lib.pcd_surface_metrics_workspace_bytes(32768, 4, 4) == 0

    def nearest(q=p, nq=p, nq_max=100, t=p, nt=p, nt_max=50, pairs=3, d2=p, index=p, ws=p, ws_bytes=big):
        return lib.pcd_nearest_neighbors(q, nq, nq_max, t, nt, nt_max, pairs, d2, index, ws, ws_bytes, None)

    need = lib.pcd_nearest_workspace_bytes(3, 100, 50)
    for kw in (dict(q=None), dict(nq=None), dict(t=None), dict(nt=None), dict(d2=None), dict(index=None), dict(ws=None), dict(pairs=0),
               dict(pairs=-1), dict(pairs=65536), dict(nq_max=0), dict(nt_max=0), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert nearest(**kw) == -1, kw
        assert b"bad argument" in lib.pcd_last_error()

    def surface(a=p, na=p, b=p, nb=p, pairs=3, thresholds=taus, k=3, rows=p, ws=p, ws_bytes=big, na_max=100, nb_max=50):
        return lib.pcd_surface_metrics(a, None, na, na_max, b, None, nb, nb_max, pairs, thresholds, k, rows, None, None, None, None, ws,
                                       ws_bytes, None)

    need = lib.pcd_surface_metrics_workspace_bytes(3, 100, 50)
    bad = [dict(a=None), dict(na=None), dict(b=None), dict(nb=None), dict(rows=None), dict(ws=None), dict(pairs=0), dict(pairs=-5),
           dict(pairs=32768),                                                # 2 * pairs = 65536 is past the grid limit
           dict(k=-1), dict(k=9), dict(k=3, thresholds=None), dict(na_max=0), dict(nb_max=0), dict(ws_bytes=need - 1)]
    for value in (-0.01, float("nan"), float("inf"), -float("inf")):
        bad.append(dict(thresholds=(C.c_float * 3)(0.02, value, 0.1)))
    for kw in bad:
        assert surface(**kw) == -1, kw
        assert b"bad argument" in lib.pcd_last_error()

    for args in ((None, p, 2, 8, 0.5, p), (p, None, 2, 8, 0.5, p), (p, p, 2, 8, 0.5, None), (p, p, 0, 8, 0.5, p), (p, p, 2, 0, 0.5, p),
                 (p, p, 2, 8, float("nan"), p)):
        assert lib.pcd_voxel_iou(*args, None) == -1, args


def test_surface_columns():
    from shapegen_amd import metrics as M
    base = ["ACC", "COMP", "CHAMFER_L1", "ACC2", "COMP2", "CHAMFER_L2", "HAUSDORFF", "NC_A", "NC_B", "NC"]
    assert M.DEFAULT_THRESHOLDS == (0.02, 0.04, 0.1)
    assert M.surface_columns() == base + ["PRECISION@0.02", "RECALL@0.02", "FSCORE@0.02", "PRECISION@0.04", "RECALL@0.04", "FSCORE@0.04",
                                          "PRECISION@0.1", "RECALL@0.1", "FSCORE@0.1"]
    assert M.surface_columns(()) == base and M.surface_columns((0.25,))[10:] == ["PRECISION@0.25", "RECALL@0.25", "FSCORE@0.25"]
    assert M.mesh_columns((0.5,)) == M.surface_columns((0.5,)) + ["IOU"]
    assert len(M.surface_columns(range(8))) == 10 + 3 * 8


def test_cpu_tensors_raise():
    from shapegen_amd import metrics as M
    from shapegen_amd.utils import Mesh
    x = torch.zeros(2, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.nearest_neighbors(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.nearest_neighbors([x[0]], [x[1]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.surface_metrics(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.voxel_iou(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4))
    tri = Mesh(torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.mesh_metrics([tri], [tri])
    with pytest.raises(ValueError):
        M.surface_metrics(x, x, thresholds=(-0.1,))
    with pytest.raises(ValueError):
        M.surface_metrics(x, x, thresholds=tuple(range(9)))
