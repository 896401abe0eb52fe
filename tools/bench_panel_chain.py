"""Dev tool: the row-panel chains (csrc/panelchain.hip) against the per-layer launches they replace (pcd_gemm_f16_wfrag: gemm_xs_kernel), M = 64 x 2048,
random fp16 data.  The variants are interleaved in one process, several rounds after a ramp; median and min per variant (the method of
tools/bench_wide_chain.py).  Also checks that the two give the same bits."""
import sys, os, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import torch, shapegen_amd
from shapegen_amd import _lib
torch.set_grad_enabled(False)
lib = _lib.load()
M = 64 * 2048
ROUNDS, REPS = 7, 10
g = torch.Generator().manual_seed(0)
S = _lib.stream_ptr


def timed(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for chain, name, shapes in ((0, "E4 ", [(512, 512), (512, 512), (1024, 512)]), (1, "D3T", [(512, 512), (256, 512)])):
    ws = [(torch.randn(s, generator=g) * (2.0 / s[1]) ** 0.5).half().cuda() for s in shapes]
    bs = [(torch.randn(s[0], generator=g) * 0.1).cuda() for s in shapes]
    x = torch.randn(M, 512, generator=g).half().cuda()
    frags = []
    for w in ws:
        f = torch.empty_like(w)
        _lib.check(lib.pcd_gemm_pack_wfrag(w.data_ptr(), w.shape[1], w.shape[1], w.shape[0], f.data_ptr(), S()))
        frags.append(f)
    fp = (C.c_void_p * len(ws))(*[t.data_ptr() for t in frags]); bp = (C.c_void_p * len(ws))(*[t.data_ptr() for t in bs])
    out = torch.empty(M, shapes[-1][0], dtype=torch.float16, device="cuda")
    bufs = [x] + [torch.empty(M, s[0], dtype=torch.float16, device="cuda") for s in shapes]

    def chain_fn():
        _lib.check(lib.pcd_panel_chain(chain, x.data_ptr(), M, fp, bp, 0, out.data_ptr(), out.shape[1], 256, S()))

    def layers_fn():
        for i, (w, b, f) in enumerate(zip(ws, bs, frags)):
            d = _lib.GemmDesc()
            d.a1, d.lda1, d.k1 = bufs[i].data_ptr(), 512, 512
            d.w, d.ldw, d.bias, d.relu, d.m, d.c = w.data_ptr(), 512, b.data_ptr(), 1, M, w.shape[0]
            _lib.check(lib.pcd_gemm_f16_wfrag(C.byref(d), f.data_ptr(), bufs[i + 1].data_ptr(), w.shape[0], S()))

    chain_fn(); layers_fn(); torch.cuda.synchronize()
    same = torch.equal(out, bufs[-1])
    for _ in range(3): timed(chain_fn); timed(layers_fn)          # ramp
    tc, tl = [], []
    for _ in range(ROUNDS):
        tc.append(timed(chain_fn)); tl.append(timed(layers_fn))
    flop = 2.0 * M * sum(s[0] * s[1] for s in shapes)
    med_c, med_l = statistics.median(tc), statistics.median(tl)
    print(f"{name}: chain median {med_c:7.1f} us min {min(tc):7.1f} us = {flop / med_c / 1e6:5.0f} TFLOP/s | per-layer launches median {med_l:7.1f} us "
          f"min {min(tl):7.1f} us = {flop / med_l / 1e6:5.0f} TFLOP/s | same bits: {same}", flush=True)
