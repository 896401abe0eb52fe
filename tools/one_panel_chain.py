"""Dev tool for profilers: E4, D3T or D43 (csrc/panelchain.hip) as the chain ("chain") or as the launches it replaces ("layers": per-layer launches
for E4 and D3T; lin 15 + lin 16 per layer + D3T for D43), M = 64 x 2048.
    python tools/one_panel_chain.py {chain|layers} {0|1|2} [reps]        (0 = E4, 1 = D3T, 2 = D43)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import torch, shapegen_amd
from shapegen_amd import _lib
torch.set_grad_enabled(False)
lib = _lib.load()
what, chain, reps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 10
M = 64 * 2048
g = torch.Generator().manual_seed(0)
shapes = {0: [(512, 512), (512, 512), (1024, 512)], 1: [(512, 512), (256, 512)], 2: [(512, 1024), (512, 1024), (512, 512), (256, 512)]}[chain]
ws = [(torch.randn(s, generator=g) * (2.0 / s[1]) ** 0.5).half().cuda() for s in shapes]
bs = [(torch.randn(s[0], generator=g) * 0.1).cuda() for s in shapes]
frags = []
for w in ws:
    f = torch.empty_like(w)
    _lib.check(lib.pcd_gemm_pack_wfrag(w.data_ptr(), w.shape[1], w.shape[1], w.shape[0], f.data_ptr(), _lib.stream_ptr()))
    frags.append(f)
bufs = [torch.randn(M, shapes[0][1], generator=g).half().cuda()] + [torch.empty(M, s[0], dtype=torch.float16, device="cuda") for s in shapes]
x3 = torch.randn(M, 512, generator=g).half().cuda() if chain == 2 else None
ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
fp, bp = ptrs(frags), ptrs(bs)


def layer(i):
    d = _lib.GemmDesc()
    d.a1, d.lda1, d.k1 = bufs[i].data_ptr(), bufs[i].shape[1], bufs[i].shape[1]
    if chain == 2 and i == 1:
        d.a2, d.lda2, d.k2 = x3.data_ptr(), 512, 512
    d.w, d.ldw, d.bias, d.relu, d.m, d.c = ws[i].data_ptr(), ws[i].shape[1], bs[i].data_ptr(), 1, M, ws[i].shape[0]
    _lib.check(lib.pcd_gemm_f16_wfrag(C.byref(d), frags[i].data_ptr(), bufs[i + 1].data_ptr(), ws[i].shape[0], _lib.stream_ptr()))


for _ in range(reps):
    if what == "chain" and chain == 2:
        _lib.check(lib.pcd_panel_chain_dec(bufs[0].data_ptr(), x3.data_ptr(), M, fp, bp, 0, bufs[-1].data_ptr(), 256, 256, _lib.stream_ptr()))
    elif what == "chain":
        _lib.check(lib.pcd_panel_chain(chain, bufs[0].data_ptr(), M, fp, bp, 0, bufs[-1].data_ptr(), shapes[-1][0], 256, _lib.stream_ptr()))
    elif chain == 2:
        layer(0); layer(1)
        _lib.check(lib.pcd_panel_chain(1, bufs[2].data_ptr(), M, ptrs(frags[2:]), ptrs(bs[2:]), 0, bufs[-1].data_ptr(), 256, 256, _lib.stream_ptr()))
    else:
        for i in range(len(shapes)): layer(i)
torch.cuda.synchronize()
