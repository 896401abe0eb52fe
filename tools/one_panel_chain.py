"""Dev tool for profilers: E4 or D3T (csrc/panelchain.hip) as the chain ("chain") or as the per-layer launches it replaces ("layers"), M = 64 x 2048.
    python tools/one_panel_chain.py {chain|layers} {0|1} [reps]"""
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
shapes = [(512, 512), (512, 512), (1024, 512)] if chain == 0 else [(512, 512), (256, 512)]
ws = [(torch.randn(s, generator=g) * (2.0 / s[1]) ** 0.5).half().cuda() for s in shapes]
bs = [(torch.randn(s[0], generator=g) * 0.1).cuda() for s in shapes]
frags = []
for w in ws:
    f = torch.empty_like(w)
    _lib.check(lib.pcd_gemm_pack_wfrag(w.data_ptr(), 512, 512, w.shape[0], f.data_ptr(), _lib.stream_ptr()))
    frags.append(f)
bufs = [torch.randn(M, 512, generator=g).half().cuda()] + [torch.empty(M, s[0], dtype=torch.float16, device="cuda") for s in shapes]
fp = (C.c_void_p * len(ws))(*[t.data_ptr() for t in frags]); bp = (C.c_void_p * len(ws))(*[t.data_ptr() for t in bs])
for _ in range(reps):
    if what == "chain":
        _lib.check(lib.pcd_panel_chain(chain, bufs[0].data_ptr(), M, fp, bp, 0, bufs[-1].data_ptr(), shapes[-1][0], 256, _lib.stream_ptr()))
    else:
        for i, (w, b, f) in enumerate(zip(ws, bs, frags)):
            d = _lib.GemmDesc()
            d.a1, d.lda1, d.k1 = bufs[i].data_ptr(), 512, 512
            d.w, d.ldw, d.bias, d.relu, d.m, d.c = w.data_ptr(), 512, b.data_ptr(), 1, M, w.shape[0]
            _lib.check(lib.pcd_gemm_f16_wfrag(C.byref(d), f.data_ptr(), bufs[i + 1].data_ptr(), w.shape[0], _lib.stream_ptr()))
torch.cuda.synchronize()
