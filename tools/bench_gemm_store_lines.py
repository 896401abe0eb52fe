"""Dev tool: what are whole-line output stores worth in gemm_xs_kernel?  The kernel's ten dripped chunks per wave and tile leave as 8 rows x 128 bytes (whole
128-byte lines), its six direct ones as 16 rows x 64 bytes (half lines).  The ablation instance can send either kind out in the OTHER shape -- same bytes,
same count, same vmcnt accounting, WRONG places of the same tile: pcd_gemm_set_config(35) the drip stores as half lines, (36) the direct stores as whole
lines, (37) both; 38 is that instance with the product's stores (the control of those), 19 the instance without global stores.
bench_gemm_xs_ablation.py's method: min of 3 x 10 launches after a 30-launch ramp, one process; the product instance and the control are timed twice per
shape, first and last, for the tool's own spread.  Results: profiles/gemm_store_lines.md."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import shapegen_amd
from shapegen_amd import _lib, ops
torch.set_grad_enabled(False)
lib = _lib.load()
g = torch.Generator(device="cuda").manual_seed(0)
def ev(fn, n=10, reps=3):
    for _ in range(30): fn()
    best = 1e9
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / n * 1e3)
    return best
M = 131072
runs = [(16, "product"), (38, "ablation instance, product's stores"), (35, "drip stores as half lines"), (36, "direct stores as whole lines"),
        (37, "drip as half lines, direct as whole lines"), (19, "no global stores"), (38, "ablation instance, product's stores (again)"), (16, "product (again)")]
total = {}
for K, C in [(1024, 2048), (1024, 1024), (512, 512)]:
    a = torch.randn(M, K, device="cuda", generator=g).clamp_min(0).half()
    w = (torch.randn(C, K, device="cuda", generator=g) / K ** 0.5).half()
    bias = torch.randn(C, device="cuda", generator=g) * 0.1
    wfrag = torch.empty_like(w)
    _lib.check(lib.pcd_gemm_pack_wfrag(w.data_ptr(), K, K, C, wfrag.data_ptr(), _lib.stream_ptr()))
    d = ops._desc(a, w, bias, relu=True)
    out = torch.empty(M, C, dtype=torch.float16, device="cuda")
    print(f"K={K} C={C} M={M}", flush=True)
    for code, name in runs:
        lib.pcd_gemm_set_config(code)
        t = ev(lambda: lib.pcd_gemm_f16_wfrag(d, wfrag.data_ptr(), out.data_ptr(), C, _lib.stream_ptr()))
        total[name] = total.get(name, 0.0) + t
        print(f"    code {code:2d} ({name}): {t:8.1f} us", flush=True)
    lib.pcd_gemm_set_config(16)
    del a, w, out
print("sum over the three shapes")
for name, t in total.items():
    print(f"    {name}: {t:8.1f} us")
