"""Every public packer of the register-resident chains (csrc/widechain.hip, wideffn.hip, sab_tail.hip) against the numpy statement of its buffer
(tests/stage_image_statement.py), byte for byte, with `*_packed_bytes` against the statement's size.  No chain kernel is launched.

Each buffer is allocated 4 KiB larger than the reported size and packed twice, over a fill of 0xA5 and over its complement 0x5A: the slack must keep
the fill (no overrun), and the inside must equal the statement both times (a byte the packer left alone would hold the fill, and cannot equal the
statement under both fills)."""
import ctypes as C

import numpy as np
import pytest
import torch

import stage_image_statement as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SLACK = 4096
ENDS_SHAPES = {0: [(128, 128), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256)],      # (C, K) of E23's layers
               1: [(256, 512), (256, 256), (128, 256), (128, 256)]}                              # ... of D21's
ENDS_NARROW = {0: 2, 1: 3}


def _lib_():
    from shapegen_amd import _lib
    return _lib, _lib.load()


def _w(g, c, k):
    return (torch.randn(c, k, generator=g) / k ** 0.5).half().numpy()


def _v(g, n):
    return torch.randn(n, generator=g).float().numpy()


def _check(parts, weights, params, nbytes, pack):
    """pack(device pointers of weights, of params, destination pointer) -> return code"""
    _lib, _ = _lib_()
    want = S.assemble(parts, weights, params)
    assert nbytes == S.size(parts) == want.size
    keys = weights.keys() if isinstance(weights, dict) else range(len(weights))
    dw = {k: torch.from_numpy(np.ascontiguousarray(weights[k])).cuda() for k in keys}
    keys = params.keys() if isinstance(params, dict) else range(len(params))
    dp = {k: torch.from_numpy(np.ascontiguousarray(params[k])).cuda() for k in keys}
    for fill in (0xA5, 0x5A):
        buf = torch.full((nbytes + SLACK,), fill, dtype=torch.uint8, device="cuda")
        _lib.check(pack({k: t.data_ptr() for k, t in dw.items()}, {k: t.data_ptr() for k, t in dp.items()}, buf.data_ptr()))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[nbytes:] == fill).all(), "the packer wrote past its reported size"
        bad = np.flatnonzero(got[:nbytes] != want)
        assert bad.size == 0, (fill, bad.size, int(bad[0]), int(bad[-1]))


def _ptrs(d, n):
    return (C.c_void_p * n)(*[d[i] for i in range(n)])


@pytest.mark.parametrize("chain", [0, 1])
def test_pw_wide_pack(chain):
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(4100 + chain)
    shapes = [(256, 256), (256, 256), (512, 256)] if chain == 0 else [(256, 512), (256, 256), (128, 256)]
    ws, bs = [_w(g, *s) for s in shapes], [_v(g, s[0]) for s in shapes]
    _check(S.pw_wide(chain), ws, bs, int(lib.pcd_pw_wide_packed_bytes(chain)),
           lambda w, b, dst: lib.pcd_pw_wide_pack(chain, _ptrs(w, 3), _ptrs(b, 3), dst, _lib.stream_ptr()))


@pytest.mark.parametrize("hilo", [0, 1])
@pytest.mark.parametrize("chain", [0, 1])
def test_pw_wide_ends_pack(chain, hilo):
    from shapegen_amd import packing
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(4200 + 10 * chain + hilo)
    shapes = ENDS_SHAPES[chain]
    ws = [_w(g, *s) for s in shapes]
    if hilo:
        c, k = shapes[ENDS_NARROW[chain]]
        ws[ENDS_NARROW[chain]] = packing.split_hilo((torch.randn(c, k, generator=g, dtype=torch.float64) / k ** 0.5).numpy())
        assert ws[ENDS_NARROW[chain]].shape == (c, 2 * k) and ws[ENDS_NARROW[chain]].dtype == np.float16
    bs = [_v(g, s[0]) for s in shapes]
    n = len(shapes)
    _check(S.pw_wide_ends(chain, hilo), ws, bs, int(lib.pcd_pw_wide_ends_packed_bytes(chain, hilo)),
           lambda w, b, dst: lib.pcd_pw_wide_ends_pack(chain, hilo, _ptrs(w, n), _ptrs(b, n), dst, _lib.stream_ptr()))


@pytest.mark.parametrize("passes", [1, 2, 3, 4])
def test_ln_linear_pack(passes):
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(4300 + passes)
    ws = {"w": _w(g, 256 * passes, 256)}
    ps = {"b": _v(g, 256 * passes), "ln_g": _v(g, 256), "ln_b": _v(g, 256)}
    _check(S.ln_linear(passes), ws, ps, int(lib.pcd_pw_wide_ln_linear_packed_bytes(passes)),
           lambda w, p, dst: lib.pcd_pw_wide_ln_linear_pack(w["w"], p["b"], passes, p["ln_g"], p["ln_b"], dst, _lib.stream_ptr()))


def test_wide_ffn_pack():
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(4400)
    ws = {"w1": _w(g, 1024, 256), "w2": _w(g, 256, 1024)}
    ps = {"b1": _v(g, 1024), "b2": _v(g, 256), "ln_g": _v(g, 256), "ln_b": _v(g, 256)}
    _check(S.wide_ffn(), ws, ps, int(lib.pcd_wide_ffn_packed_bytes()),
           lambda w, p, dst: lib.pcd_wide_ffn_pack(w["w1"], p["b1"], w["w2"], p["b2"], p["ln_g"], p["ln_b"], dst, _lib.stream_ptr()))


@pytest.mark.parametrize("c", [64, 128])
def test_sab_tail_pack(c):
    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(4500 + c)
    ws = {"w_in": _w(g, 3 * c, c), "w_out": _w(g, c, c), "w_ff1": _w(g, 4 * c, c), "w_ff2": _w(g, c, 4 * c)}
    ps = {"b_in": _v(g, 3 * c), "b_out": _v(g, c), "ln1_g": _v(g, c), "ln1_b": _v(g, c), "ln2_g": _v(g, c), "ln2_b": _v(g, c),
          "b_ff1": _v(g, 4 * c), "b_ff2": _v(g, c)}

    def pack(w, p, dst):
        d = _lib.SabDesc()
        d.dim = c
        for k, ptr in {**w, **p}.items():
            setattr(d, k, ptr)
        return lib.pcd_sab_tail_pack(C.byref(d), dst, _lib.stream_ptr())
    _check(S.sab_tail(c), ws, ps, int(lib.pcd_sab_tail_packed_bytes(c)), pack)
