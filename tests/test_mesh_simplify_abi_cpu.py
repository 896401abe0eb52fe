"""The boundary of mesh simplification without a device: the symbols are declared, exported and prototyped, the constants of
`mesh_ops` are the header's, and the entry points refuse bad arguments before any device work."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pcd_mesh_simplify_workspace_bytes", "pcd_mesh_simplify_count", "pcd_mesh_simplify_emit")


def header():
    return open(os.path.join(ROOT, "include", "pcd_hip.h")).read()


def test_symbols_are_declared_exported_and_prototyped():
    from shapegen_amd import _lib, mesh_ops
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in _lib._SIGS, name
    define = dict(re.findall(r"^#define (PCD_MESH_SIMPLIFY_\w+) (.+)$", header(), re.M))
    value = lambda k: eval(define["PCD_MESH_SIMPLIFY_" + k])
    assert (value("RESOLUTION"), value("CELL_SIZE"), value("TARGET_FACES")) == \
        (mesh_ops.SIMPLIFY_RESOLUTION, mesh_ops.SIMPLIFY_CELL_SIZE, mesh_ops.SIMPLIFY_TARGET_FACES)
    assert mesh_ops.PLACEMENTS == {"quadric": value("QUADRIC"), "mean": value("MEAN")}
    assert value("MAX_RESOLUTION") == mesh_ops.SIMPLIFY_MAX_RESOLUTION == 1024
    assert value("MAX_VERTICES") == mesh_ops.SIMPLIFY_MAX_VERTICES == 1 << 21


def test_arg_validation_without_gpu():
    from shapegen_amd import _lib
    lib = _lib.load()
    size = lib.pcd_mesh_simplify_workspace_bytes
    assert size(0, 10, 10) == 0 and size(1, -1, 10) == 0 and size(70000, 10, 10) == 0 and size(1, 10, 1 << 40) == 0
    assert 0 < size(1, 0, 0) <= size(1, 100, 200) < size(2, 1000, 2000) and size(3, 100, 200) % 256 == 0
    p, n = 64, size(2, 100, 200)                                            # pointers are compared with NULL and never read on the host
    good = dict(v=p, f=p, o=p, batch=2, tv=100, tf=200, mv=60, mode=0, params=p, dd=0, ws=p, n=n, res=p, map=p, counts=p)

    def count(**kw):
        a = dict(good, **kw)
        return lib.pcd_mesh_simplify_count(a["v"], a["f"], a["o"], a["batch"], a["tv"], a["tf"], a["mv"], a["mode"], a["params"], a["dd"],
                                           a["ws"], a["n"], a["res"], a["map"], a["counts"], None)

    def emit(**kw):
        a = dict(dict(good, mode=0, out_o=p, out_v=p, out_f=p), **kw)
        return lib.pcd_mesh_simplify_emit(a["v"], a["f"], a["o"], a["batch"], a["tv"], a["tf"], a["mv"], a["mode"], a["ws"], a["n"],
                                          a["out_o"], a["out_v"], a["out_f"], None)
    for key in ("v", "f", "o", "params", "ws", "res", "map", "counts"):
        assert count(**{key: None}) == -1, key
    assert b"bad argument" in lib.pcd_last_error()
    for kw in (dict(mode=3), dict(mode=-1), dict(dd=2), dict(batch=0), dict(batch=65536), dict(tv=-1), dict(tf=-1), dict(mv=101), dict(mv=-1),
               dict(tv=1 << 22, mv=1 << 21, n=1 << 40)):
        assert count(**kw) == -1, kw
    assert count(n=n - 1) == -3 and count(n=0) == -3
    for key in ("v", "f", "o", "ws", "out_o", "out_v", "out_f"):
        assert emit(**{key: None}) == -1, key
    for kw in (dict(mode=2), dict(mode=-1), dict(batch=0), dict(mv=101), dict(tv=1 << 22, mv=1 << 21, n=1 << 40)):
        assert emit(**kw) == -1, kw
    assert emit(n=n - 1) == -3
