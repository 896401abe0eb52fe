"""Dev tool: the row-panel chains (csrc/panelchain.hip) against the launches they replace, M = 64 x 2048, random fp16 data.
    E4   against lin 8, 9, 10 per layer (pcd_gemm_f16_wfrag: gemm_xs_kernel)
    D3T  against lin 17, 18 per layer
    D43  against lin 15, lin 16 per layer + D3T
The arms are interleaved in one process, several rounds after a ramp; median and min per arm (the method of tools/bench_wide_chain.py).  Every arm runs
TWICE per round ("again"): the distance between the two medians of the same arm is the tool's own spread, below which a difference says nothing.
Also checks that the arms give the same bits.
    python tools/bench_panel_chain.py [--against OTHER/libpcd_hip.so]
--against: E4, D3T and the replaced launches of another build of the library (the parent commit's) as further arms, interleaved with this build's."""
import sys, os, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import torch, shapegen_amd
from shapegen_amd import _lib
torch.set_grad_enabled(False)
lib = _lib.load()
other = None
if "--against" in sys.argv:
    other = C.CDLL(sys.argv[sys.argv.index("--against") + 1])
    for name in ("pcd_panel_chain", "pcd_gemm_f16_wfrag"):
        getattr(other, name).restype, getattr(other, name).argtypes = _lib._SIGS[name]
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


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def run_arms(name, flop, arms, outs):
    """arms: {label: fn}; outs: {label: the tensor its fn leaves the result in}"""
    for fn in arms.values(): fn()
    torch.cuda.synchronize()
    first = next(iter(outs.values()))
    same = all(torch.equal(first, o) for o in outs.values())
    for _ in range(3):                                                   # ramp
        for fn in arms.values(): timed(fn)
    t = {(k, i): [] for k in arms for i in (0, 1)}
    for _ in range(ROUNDS):
        for i in (0, 1):
            for k, fn in arms.items(): t[(k, i)].append(timed(fn))
    spread = 0.0
    for k in arms:
        m0, m1 = statistics.median(t[(k, 0)]), statistics.median(t[(k, 1)])
        spread = max(spread, abs(m0 - m1))
        print(f"{name} {k:34s}: median {m0:7.1f} us min {min(t[(k, 0)]):7.1f} us = {flop / m0 / 1e6:5.0f} TFLOP/s | again: median {m1:7.1f} us "
              f"min {min(t[(k, 1)]):7.1f} us", flush=True)
    print(f"{name}: same bits: {same} | the tool's own spread (the same arm twice, the largest of the arms): {spread:.1f} us", flush=True)


def layer_fn(L, a, a2, w, b, f, out):
    d = _lib.GemmDesc()
    d.a1, d.lda1, d.k1 = a.data_ptr(), a.shape[1], a.shape[1]
    if a2 is not None:
        d.a2, d.lda2, d.k2 = a2.data_ptr(), a2.shape[1], a2.shape[1]
    d.w, d.ldw, d.bias, d.relu, d.m, d.c = w.data_ptr(), w.shape[1], b.data_ptr(), 1, M, w.shape[0]
    return lambda: _lib.check(L.pcd_gemm_f16_wfrag(C.byref(d), f.data_ptr(), out.data_ptr(), w.shape[0], S()))


def make(shapes):
    ws = [(torch.randn(s, generator=g) * (2.0 / s[1]) ** 0.5).half().cuda() for s in shapes]
    bs = [(torch.randn(s[0], generator=g) * 0.1).cuda() for s in shapes]
    frags = []
    for w in ws:
        f = torch.empty_like(w)
        _lib.check(lib.pcd_gemm_pack_wfrag(w.data_ptr(), w.shape[1], w.shape[1], w.shape[0], f.data_ptr(), S()))
        frags.append(f)
    return ws, bs, frags


def empty(c):
    return torch.empty(M, c, dtype=torch.float16, device="cuda")


for chain, name, shapes in ((0, "E4 ", [(512, 512), (512, 512), (1024, 512)]), (1, "D3T", [(512, 512), (256, 512)])):
    ws, bs, frags = make(shapes)
    x = torch.randn(M, 512, generator=g).half().cuda()
    fp, bp = ptrs(frags), ptrs(bs)
    arms, outs = {}, {}
    for label, L in (("chain", lib), ("chain, other build", other)):
        if L is None: continue
        out = empty(shapes[-1][0])
        arms[label] = (lambda L=L, out=out: _lib.check(L.pcd_panel_chain(chain, x.data_ptr(), M, fp, bp, 0, out.data_ptr(), out.shape[1], 256, S())))
        outs[label] = out
    bufs = [x] + [empty(s[0]) for s in shapes]
    fns = [layer_fn(lib, bufs[i], None, ws[i], bs[i], frags[i], bufs[i + 1]) for i in range(len(shapes))]
    arms["per-layer launches"] = lambda fns=fns: [f() for f in fns]
    outs["per-layer launches"] = bufs[-1]
    run_arms(name, 2.0 * M * sum(s[0] * s[1] for s in shapes), arms, outs)

# D43: lin 15, 16, 17, 18; lin 16 reads [lin 15's output | x3]
shapes = [(512, 1024), (512, 1024), (512, 512), (256, 512)]
ws, bs, frags = make(shapes)
x = torch.randn(M, 1024, generator=g).half().cuda()
x3 = torch.randn(M, 512, generator=g).half().cuda()
fp, bp = ptrs(frags), ptrs(bs)
arms, outs = {}, {}
out = empty(256)
arms["chain"] = lambda: _lib.check(lib.pcd_panel_chain_dec(x.data_ptr(), x3.data_ptr(), M, fp, bp, 0, out.data_ptr(), 256, 256, S()))
outs["chain"] = out
for label, L in (("lin 15 + lin 16 + D3T", lib), ("lin 15 + lin 16 + D3T, other build", other)):
    if L is None: continue
    d4, d3a, d3 = empty(512), empty(512), empty(256)
    f15 = layer_fn(L, x, None, ws[0], bs[0], frags[0], d4)
    f16 = layer_fn(L, d4, x3, ws[1], bs[1], frags[1], d3a)
    fp2, bp2 = ptrs(frags[2:]), ptrs(bs[2:])
    def replaced(L=L, f15=f15, f16=f16, d3a=d3a, d3=d3, fp2=fp2, bp2=bp2):
        f15(); f16()
        _lib.check(L.pcd_panel_chain(1, d3a.data_ptr(), M, fp2, bp2, 0, d3.data_ptr(), 256, 256, S()))
    arms[label] = replaced
    outs[label] = d3
run_arms("D43", 2.0 * M * sum(s[0] * s[1] for s in shapes), arms, outs)
