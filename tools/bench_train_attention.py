"""Dev tool: time the attention backbone's training step (forward + backward + AdamW, `AttentionTrainer`) at the
reference's training shape (batch 16 x 2048 points, train_point_ddpm.py) with HIP events, and the attention backward
alone (pcd_set_attention_backward_f16: delta pre-pass, dK/dV kernel, dQ kernel) at d = 16, 32, 64 (C = 64, 128, 256,
4 heads).  Rates are on the useful 10 * B * N^2 * C FLOP of the backward against the 2.5 PFLOP/s dense fp16 peak.
Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import shapegen_amd  # noqa: E402,F401
from shapegen_amd import _lib  # noqa: E402
from shapegen_amd.diffusion import PointCloudDiffusion  # noqa: E402

PEAK = 2.5e15
B, N = int(os.environ.get("B", 16)), int(os.environ.get("N", 2048))
STEPS = int(os.environ.get("STEPS", 10))


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def main():
    torch.manual_seed(0)
    res = {"B": B, "N": N}
    lib, st = _lib.load(), _lib.stream_ptr()
    heads = 4
    for c in (64, 128, 256):
        qkv = (torch.randn(B * N, 3 * c, device="cuda") * 1.5).half()
        dout = torch.randn(B * N, c, device="cuda").half()
        out = torch.empty(B * N, c, dtype=torch.float16, device="cuda")
        lse = torch.empty(B * heads * N, dtype=torch.float32, device="cuda")
        dq = torch.empty(B * N, 3 * c, dtype=torch.float16, device="cuda")
        ws = torch.empty(lib.pcd_set_attention_backward_workspace_bytes(B, N, c, heads) // 4, device="cuda")
        _lib.check(lib.pcd_set_attention_lse_f16(qkv.data_ptr(), B, N, c, heads, out.data_ptr(), lse.data_ptr(), st), "lse")
        fwd = timed(lambda: lib.pcd_set_attention_lse_f16(qkv.data_ptr(), B, N, c, heads, out.data_ptr(), lse.data_ptr(), st), 20)
        bwd = timed(lambda: lib.pcd_set_attention_backward_f16(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), B, N, c,
                                                               heads, dq.data_ptr(), ws.data_ptr(), ws.numel() * 4, st), 20)
        flop = 10.0 * B * N * N * c
        res[f"d{c // heads}"] = {"fwd_lse_us": round(fwd * 1e6, 1), "bwd_us": round(bwd * 1e6, 1),
                                 "bwd_tflops": round(flop / bwd / 1e12, 1), "bwd_frac_peak": round(flop / bwd / PEAK, 4)}
    model = PointCloudDiffusion(num_points=N, backbone="attention").to("cuda").train()
    tr = model.configure_optimizers()["optimizer"]
    x0 = torch.randn(B, N, 3, device="cuda") * 0.4

    def one():
        t = torch.rand(B, device="cuda")
        x_t, noise, _, _ = model.add_noise(x0, t)
        tr.forward(x_t, t)
        tr.backward(noise)
        tr.step()
    dt = timed(one, STEPS)
    res["step_ms"] = round(dt * 1e3, 2)
    res["shapes_per_s"] = round(B / dt, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
