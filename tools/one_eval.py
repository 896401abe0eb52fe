"""Dev tool: the evaluation of test_point_ddpm.py:85-92 at BASELINE size -- 64 pairs of 2048-point clouds, Chamfer +
Sinkhorn EMD + voxel BCE -- through metrics.pair_metrics (one enqueue).  By default 5 times on the host clock (for rocprofv3
--kernel-trace --stats); with --rounds R, R evaluations after --warmup, each between two device events: median and range in ms,
also written to --out as JSON."""
import argparse, json, sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import shapegen_amd
from shapegen_amd import metrics as M
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
g = torch.Generator().manual_seed(0)
a = (torch.rand(64, 2048, 3, generator=g) * 2 - 1).cuda()
b = (a + 0.05 * torch.randn(64, 2048, 3, generator=g).cuda()).contiguous()
for _ in range(args.warmup):
    M.pair_metrics(a, b, True)
if args.rounds:
    ms = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rows = M.pair_metrics(a, b, True)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    result = {"what": "pair_metrics(64 x 2048 x 2048, sinkhorn, max_iter 100)", "rounds": args.rounds, "median_ms": ms[len(ms) // 2],
              "min_ms": ms[0], "max_ms": ms[-1], "mean_rows": rows.mean(0).tolist()}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))
else:
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(5):
        rows = M.pair_metrics(a, b, True)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 5
    print(f"pair_metrics(64 x 2048 x 2048, sinkhorn=True): {dt * 1e3:.2f} ms per evaluation; mean rows {rows.mean(0).tolist()}")
