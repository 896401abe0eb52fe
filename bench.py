"""Headline benchmark: denoising-steps/sec of the point-cloud diffusion sampler hot path.

    python bench.py --gpus N --steps K --warmup W [--config cfg2|cfg3|cfg4|cfg5] [--backbone pointnet|attention]
                    [--full] [--dump-outputs DIR]

Default (`--config cfg2`, BASELINE.json configs[1]): one "step" = one ancestral denoising step (`sample2`
loop body, reference diffusion.py:241-257) of a whole batch: denoiser forward (HIP kernels) + on-device Philox
noise + fused DDPM update; 2048 points, batch 64 per GPU, fp16 operands / fp32 accumulation, 1000-step
schedule (the W warm-up and K timed steps are the first steps of that schedule; past its end it starts over).
Inputs are resident in HBM before the timed region.  With N > 1 every rank runs the same per-GPU batch (weak
scaling, no data-path collective: shapes are independent).

A plain run sets up, warms up, times the K steps and prints the line: `value` / `ms_per_step` and, for the
pointnet backbone launched eagerly, `roofline` from the HIP events the timed steps themselves record.  Everything
else (the other launch mode, `roofline_attention`, `config.other_configs`, the CPU baselines; cfg3's eager GEMM
profile, cfg5's latent / VAE legs) runs only under `--full`, where the `--no-*` options still leave parts out.

`--dump-outputs DIR` writes, after the timed steps, what the timed path computed in its last step as float32
`DIR/<name>.npy` (rank 0): cfg2 `x` = the sampler state (B, 2048, 3); cfg3 `clouds` (global batch, 2048, 3);
cfg4 `latents` (32, 256) and `points` / `counts` (the voxel->points clouds, concatenated); cfg5 `points` / `counts`
of the gathered clouds.  Inputs are seeded: the same arguments give the same inputs in every run.

Launching: with N > 1 and no WORLD_SIZE in the environment this process never touches the GPU: it starts N
child processes (one rank per GPU, RCCL rendezvous on 127.0.0.1; `shapegen_amd/launcher.py`), polls all of them,
terminates the siblings of the first rank that fails, enforces `--timeout`, keeps per-rank logs, relays rank 0's JSON
line and exits non-zero (with the ranks' stderr tails) if any rank failed.  Under `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` the ranks are
already there and each process is one rank.

Other workloads (parity-test configurations of BASELINE.json, reported with the same JSON contract):
  --config cfg3   DDIM `sample`, 50 steps, 64 shapes per GPU through `dist.sample_sharded` (clouds all-gathered)
  --config cfg4   latent diffusion on one GPU: VAE3DLarge encode of 32 grids, 1000-step latent DDIM, decode,
                  voxel->points; `roofline` = the latent step against HBM, `roofline_vae_decode` against MFMA
  --config cfg5   latent diffusion: 1000-step latent DDIM, 32 latents per GPU, VAE decode, voxel->points,
                  RCCL all-gather of the ragged clouds, per-sample Chamfer / Sinkhorn-EMD / voxel-BCE rows

Prints ONE JSON line (rank 0) with the driver's contract plus
  "roofline":            dominant kernel (global_feat.3 GEMM 2048->4096 with fused max) timed live with HIP
                         events on the launch stream, against the dense fp16 MFMA peak;
  "roofline_attention":  the set-attention kernel (QK^T / softmax / PV, reference networks.py:61,80-81) at
                         batch 64 x 2048 points, C = 256, 4 heads, timed the same way (N = 1 only);
  "cpu_baseline":        the CPU oracle (PyTorch-CPU fp32 restatement) timed on the host cores on a bounded
                         sample of the same workload at its real shape (rank 0, N = 1 only);
  "cpu_baseline_cfg1":   BASELINE configs[0] (DDIM, B = 4, N = 512, 100 steps) run in full on the oracle;
  "config.other_configs": the other single-GPU workloads measured after the headline region (cfg3 DDIM-50 steps/s,
                         cfg4 end to end, latent step, VAE encode / decode), so the driver's record carries them.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B_PER_GPU = 64
N_POINTS = 2048
SCHEDULE_STEPS = 1000
MFMA_F16_DENSE_PEAK_TFLOPS = 2500.0           # MI355X_MICROARCH.md: ~2.5 PF dense fp16/bf16
GF3_FLOP_PER_LAUNCH = 2.0 * B_PER_GPU * N_POINTS * 2048 * 4096   # algorithmic FLOP of the dominant GEMM
ATT_C, ATT_HEADS = 256, 4
ATT_FLOP_PER_LAUNCH = 4.0 * B_PER_GPU * N_POINTS * N_POINTS * ATT_C      # QK^T + PV (4 B N^2 C)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)     # 100 x ~4 ms; the GPU reaches steady clocks after ~10 steps
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", choices=("cfg2", "cfg3", "cfg4", "cfg5"), default="cfg2")
    ap.add_argument("--timeout", type=float, default=600.0, help="overall limit of an N > 1 run, seconds")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the config.other_configs legs of the default line")
    ap.add_argument("--backbone", choices=("pointnet", "attention"), default="pointnet",
                    help="denoiser behind the cfg2 sampler: UNetPointNetLarge (the reference's wiring) or "
                         "UNetAttentionPointExperimental (the set-attention carrier)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-attention", action="store_true", help="skip the roofline_attention leg")
    ap.add_argument("--graph", action="store_true",
                    help="time the hipGraph replay path in the headline region instead of eager launches (the eager "
                         "default at N = 1 lets the dominant kernel be timed by HIP events inside the timed region; the "
                         "other launch mode's number is reported beside it either way).  With N > 1 graph replay -- what "
                         "sample2() itself drives -- is the default: a rank's step then costs its host one launch, not 29")
    ap.add_argument("--eager", action="store_true", help="N > 1: time eager launches in the headline region")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beside the headline (other launch mode, attention roofline, other "
                         "configs, CPU baselines, profiling runs); a plain run does only the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step as DIR/<name>.npy (float32)")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------ launcher (GPU-free)
def launch_children(args) -> int:
    """Parent of an N-rank run.  Runs BEFORE anything imports torch.cuda (`shapegen_amd.launcher` is standard library
    only): one child per GPU, all polled, siblings of a failed rank terminated, overall --timeout, per-rank logs."""
    from shapegen_amd import launcher
    return launcher.main_launch(os.path.abspath(__file__), sys.argv[1:], args.gpus, args.timeout)


# ------------------------------------------------------------------------------------------ helpers
def synth_weights(backbone="pointnet"):
    import numpy as np
    import torch
    from shapegen_amd import specs
    spec = (specs.unet_pointnet_large_spec(prefix="model.") if backbone == "pointnet"
            else specs.unet_attention_spec(prefix="model."))
    gain = 1.3 if backbone == "pointnet" else 1.0
    return {k: torch.from_numpy(np.asarray(v)) for k, v in specs.synth_state_dict(spec, seed=0, gain=gain).items()}


DUMP_MAX_BYTES = 64 << 20


def ragged(clouds):
    """A list of (n_i, 3) clouds as one (sum n_i, 3) array of points and the (len,) array of n_i."""
    import torch
    counts = torch.tensor([int(c.shape[0]) for c in clouds], dtype=torch.float32)
    points = torch.cat([c.detach().float().cpu().reshape(-1, 3) for c in clouds]) if clouds else torch.zeros(0, 3)
    return {"points": points, "counts": counts}


def dump_outputs(path, arrays):
    """`arrays` (name -> tensor) as float32 `path/<name>.npy`.  An array over its share of DUMP_MAX_BYTES keeps a fixed,
    seeded, sorted sample of its rows (first axis), so that two runs write the same rows."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    share = DUMP_MAX_BYTES // max(1, len(arrays))
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.nbytes > share and a.ndim > 0 and a.shape[0] > 1:
            keep = max(1, share // max(1, a.nbytes // a.shape[0]))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(path, f"{name}.npy"), a)


def usable_cores() -> int:
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def host_memory_gb() -> float:
    """Memory this process may still take: MemAvailable capped by the cgroup limit (v2 or v1) where one is set."""
    avail = 0.0
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                avail = int(line.split()[1]) / 1e6
    except Exception:
        pass
    for lim, cur in (("/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory.current"),
                     ("/sys/fs/cgroup/memory/memory.limit_in_bytes", "/sys/fs/cgroup/memory/memory.usage_in_bytes")):
        try:
            v = open(lim).read().strip()
            if v != "max" and int(v) < (1 << 60):
                avail = min(avail, (int(v) - int(open(cur).read())) / 1e9) if avail else (int(v) - int(open(cur).read())) / 1e9
        except Exception:
            pass
    return avail


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(sd, reps=3):
    """Oracle (port of the reference's PyTorch-CPU path, diffusion.py:241-257 over networks.py:779-818) MEASURED at the
    configuration's real shape: `reps` DDPM steps at B = 64, N = 2048 after one warm-up step (a step keeps ~8 GB of fp32
    activations alive: the (64, 4096, 2048) global feature and the (64, 5120, 2048) concat the reference materialises).
    Only if the host cannot hold that is the batch halved until it fits, and `sample` says so."""
    import torch
    from oracle import torch_oracle as O   # checker/baseline only
    cores = usable_cores()
    torch.set_num_threads(cores)
    batch, mem = B_PER_GPU, host_memory_gb()
    while batch > 1 and mem and batch * 0.25 > mem:          # 0.125 GB per shape measured, x2 margin
        batch //= 2
    g = torch.Generator().manual_seed(24)
    x = torch.randn(batch, N_POINTS, 3, generator=g)
    model = lambda xx, tt: O.unet_pointnet_large(sd, "model.", xx, tt)
    z = [torch.randn(batch, N_POINTS, 3, generator=g) for _ in range(reps + 1)]

    def one(i, xx):
        t = torch.ones(batch) * (SCHEDULE_STEPS - 1 - i) / SCHEDULE_STEPS
        n, s = O.offset_cosine_schedule(t)
        eps = model(xx, t)
        x0 = O.remove_noise(xx, eps, n, s)
        tp = torch.ones(batch) * (SCHEDULE_STEPS - 2 - i) / SCHEDULE_STEPS
        npv, sp = O.offset_cosine_schedule(tp)
        return sp.view(-1, 1, 1) * x0 + (torch.sqrt(npv / n) * n).view(-1, 1, 1) * z[i]

    with torch.no_grad():
        x = one(0, x)
        t0 = time.perf_counter()
        for i in range(1, reps + 1):
            x = one(i, x)
        dt = (time.perf_counter() - t0) / reps
    scale = B_PER_GPU / batch
    what = (f"{reps} DDPM steps measured at the real shape B={batch}, N={N_POINTS} after one warm-up step" if batch == B_PER_GPU else
            f"{reps} DDPM steps at B={batch}, N={N_POINTS} (host memory {mem:.0f} GB does not hold B={B_PER_GPU}), scaled x{scale:.0f}")
    return {"value": 1.0 / (dt * scale), "unit": "denoising-steps/sec", "cores": cores, "kind": "port",
            "sample": f"{what}; torch CPU fp32, {cores} threads, {cpu_model()}", "seconds_per_step": dt * scale}


def cpu_baseline_cfg1(sd):
    """BASELINE configs[0] in full on the oracle: DDIM `sample` (what test_point_ddpm.py:36 calls), B = 4, N = 512,
    100 steps, after two warm-up forwards (SURVEY section 6 anchor: the reference itself ran 5.41 steps/s on 8 cores)."""
    import torch
    from oracle import torch_oracle as O   # checker/baseline only
    cores = usable_cores()
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(24)
    x = torch.randn(4, 512, 3, generator=g)
    model = lambda xx, tt: O.unet_pointnet_large(sd, "model.", xx, tt)
    with torch.no_grad():
        for _ in range(2):
            model(x, torch.ones(4))
        t0 = time.perf_counter()
        O.ddim_sample(model, x, 100)
        dt = time.perf_counter() - t0
    return {"value": 100 / dt, "unit": "denoising-steps/sec", "cores": cores, "kind": "port",
            "sample": f"BASELINE configs[0] in full: 100 DDIM steps, B=4, N=512 ({dt:.1f} s); torch CPU fp32, {cores} threads, {cpu_model()}"}


def cpu_baseline_latent(sd, steps=200):
    """Oracle for BASELINE configs[3]: `steps` latent DDIM steps at B = 32 (diffusion.py:637-645 over networks.py:1051-1086)
    and VAE3DLarge encode / decode of 32 grids (networks.py:2299-2339), each after one warm-up call."""
    import torch
    from oracle import torch_oracle as O   # checker/baseline only
    from shapegen_amd import specs
    cores = usable_cores()
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(24)
    z = torch.randn(32, 256, generator=g)
    model = lambda zz, tt: O.latent_unet(sd, "model.", zz, tt)
    with torch.no_grad():
        O.ddim_sample(model, z, 3)
        t0 = time.perf_counter()
        O.ddim_sample(model, z, steps)
        per_step = (time.perf_counter() - t0) / steps
        vox = (torch.rand(32, 1, 32, 32, 32, generator=g) > 0.9).float()
        O.vae_decode(sd, "vae.", z[:2], specs.VAE_DEC)
        t0 = time.perf_counter()
        O.vae_decode(sd, "vae.", z, specs.VAE_DEC)
        dec = time.perf_counter() - t0
        t0 = time.perf_counter()
        O.vae_encode(sd, "vae.", vox, specs.VAE_ENC)
        enc = time.perf_counter() - t0
    return {"value": 1.0 / per_step, "unit": "denoising-steps/sec", "cores": cores, "kind": "port",
            "sample": f"{steps} latent DDIM steps at B=32 after a 3-step warm-up; VAE3DLarge decode / encode of 32 grids once each; "
                      f"torch CPU fp32, {cores} threads, {cpu_model()}",
            "latent_us_per_step": per_step * 1e6, "vae_decode_ms": dec * 1e3, "vae_encode_ms": enc * 1e3,
            "cfg4_ms_extrapolated": (enc + dec + 1000 * per_step) * 1e3}


class Ranks:
    """Process-group plumbing of one rank."""

    def __init__(self, args):
        import torch
        self.rank = int(os.environ.get("RANK", "0"))
        self.local = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        if self.world != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={self.world}")
        # PCD_BENCH_SHARE_GPU=1 (tests on a one-GPU box only): every rank uses cuda:0 and the collectives run
        # over gloo, staged through the host; RCCL needs one device per rank
        self.shared = os.environ.get("PCD_BENCH_SHARE_GPU") == "1"
        self.device = torch.device("cuda", 0 if self.shared else self.local)
        torch.cuda.set_device(self.device)
        self.dist = None
        self.backend = None
        # PCD_DIST_FORCE_COLLECTIVE=1: a one-rank world still builds its process group, so that the RCCL branch of every
        # collective below runs on a one-GPU box (tests/test_gpu_dist.py::test_rccl_branch_on_one_gpu); not a scaling run
        if self.world > 1 or os.environ.get("PCD_DIST_FORCE_COLLECTIVE") == "1":
            import torch.distributed as dist
            self.backend = "gloo" if self.shared else "nccl"
            kw = {} if self.shared else {"device_id": self.device}
            import datetime
            # explicit rendezvous / collective timeout (the launcher sets it to half its own --timeout): a rank whose
            # peer died raises here instead of waiting for the 10-minute default
            kw["timeout"] = datetime.timedelta(seconds=int(os.environ.get("PCD_COLLECTIVE_TIMEOUT_S", "300")))
            dist.init_process_group(self.backend, **kw)
            self.dist = dist

    def sync_all(self):
        import torch
        torch.cuda.synchronize()
        if self.dist is not None:
            self.dist.barrier()
            torch.cuda.synchronize()

    def max_over_ranks(self, seconds: float) -> float:
        import torch
        if self.dist is None:
            return seconds
        tt = torch.tensor([seconds], dtype=torch.float64, device="cpu" if self.shared else self.device)
        self.dist.all_reduce(tt, op=self.dist.ReduceOp.MAX)
        return float(tt.item())

    def gather_seconds(self, seconds: float):
        """Every rank's own elapsed time, in rank order (one all-gather of a double per rank)."""
        import torch
        if self.dist is None:
            return [seconds]
        mine = torch.tensor([seconds], dtype=torch.float64, device="cpu" if self.shared else self.device)
        got = [torch.zeros_like(mine) for _ in range(self.world)]
        self.dist.all_gather(got, mine)
        return [float(g.item()) for g in got]

    def collective_ranks(self):
        """World size as seen by a collective on the data-path backend (an all-gather of one int per rank)."""
        import torch
        if self.dist is None:
            return 1
        one = torch.ones(1, dtype=torch.int32, device="cpu" if self.shared else self.device)
        got = [torch.zeros_like(one) for _ in range(self.world)]
        self.dist.all_gather(got, one)
        return int(sum(int(g.item()) for g in got))

    def finish(self):
        if self.dist is not None:
            self.dist.barrier()
            self.dist.destroy_process_group()


def attention_roofline(device, launches=100):
    """HIP events (torch's current stream is the stream the kernel is launched on) around pcd_set_attention_f16 at B=64, N=2048,
    4 heads: C = 256 (d_head 64, the north-star shape: the headline numbers) and, under `by_d`, C = 128 / 64 (d_head 32 / 16: the
    other widths of the attention U-Net, reference networks.py:628-646)."""
    import torch
    from shapegen_amd import _lib
    lib = _lib.load()

    def run(chan, count, warm):
        g = torch.Generator(device="cpu").manual_seed(7)
        qkv = torch.randn(B_PER_GPU * N_POINTS, 3 * chan, generator=g).to(device, torch.float16)     # unit-variance q, k, v
        out = torch.empty(B_PER_GPU * N_POINTS, chan, dtype=torch.float16, device=device)

        def launch():
            _lib.check(lib.pcd_set_attention_f16(qkv.data_ptr(), B_PER_GPU, N_POINTS, chan, ATT_HEADS, out.data_ptr(), 0, 0,
                                                 _lib.stream_ptr()), "set_attention")
        # warm-up: the chip takes ~100 launches (27 ms) from idle to its running clocks (tools/bench_attn_sustained.py: the first
        # 100-launch chunk measures 10 % below the following nine); the timed train starts after that ramp
        for _ in range(warm):
            launch()
        # one event pair around the whole train of launches (an event record between kernels costs tens of microseconds of
        # its own, comparable to the kernel)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(count):
            launch()
        e1.record()
        torch.cuda.synchronize()
        if not torch.isfinite(out.float()).all():
            raise SystemExit("set attention produced non-finite values")
        ms = e0.elapsed_time(e1) / count
        flop = 4.0 * B_PER_GPU * N_POINTS * N_POINTS * chan
        return ms, flop / (ms * 1e-3) / 1e12, lib.pcd_set_attention_last_kernel().decode()

    # every head width is timed the same way: 200 launches of ramp, then `launches` timed; "kernel" is the name the library
    # reports for the launch it actually made (pcd_set_attention_last_kernel), not an assumption of this script
    ms, achieved, kname = run(ATT_C, launches, 200)
    by_d = {str(ATT_C // ATT_HEADS): {"achieved": achieved, "frac": achieved / MFMA_F16_DENSE_PEAK_TFLOPS, "avg_launch_ms": ms,
                                      "kernel": kname}}
    for chan in (128, 64):
        m2, a2, k2 = run(chan, launches, 200)
        by_d[str(chan // ATT_HEADS)] = {"achieved": a2, "frac": a2 / MFMA_F16_DENSE_PEAK_TFLOPS, "avg_launch_ms": m2, "kernel": k2,
                                        "note": "VALU-issue bound (16 v_exp_f32 + 8 packs + 8 packed adds + the MFMAs' own issue slots per 32 x 32 score tile: "
                                                "~265 cycles against 128 / 96 of matrix pipe at d 32 / 16; profiles/r05_i)"}
    busy, busy_head, busy_stale = measured_mfma_busy("set_attention_sp_kernel", "attention.hip")
    return {"bound": "mfma", "kernel": kname + " (QK^T, softmax, PV; d_head 64; software-pipelined, 2 query blocks per wave)",
            "achieved": achieved, "peak": MFMA_F16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": achieved / MFMA_F16_DENSE_PEAK_TFLOPS, "traffic": None,
            "mfma_busy": busy, "mfma_busy_measured_at": busy_head, "mfma_busy_stale": busy_stale,
            "avg_launch_ms": ms, "launches_timed": launches, "flop_per_launch": ATT_FLOP_PER_LAUNCH,
            "shape": {"batch": B_PER_GPU, "points": N_POINTS, "channels": ATT_C, "heads": ATT_HEADS}, "by_d": by_d}


def _sha16(path):
    import hashlib
    try:
        return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]
    except OSError:
        return None


def measured_traffic():
    """HBM/fabric bytes per launch of the dominant kernel from the committed PMC recipe (tools/pmc_gf3.sh writes
    profiles/gf3_pmc_latest.json with the git hash AND the sha256 of csrc/gemm_f16.hip it was taken at).  Returns
    (bytes, git_head, stale): stale = the kernel source is no longer the one that was measured (the GPU box has no
    .git, so the source hash is what can be compared at run time)."""
    pmc = os.path.join(ROOT, "profiles", "gf3_pmc_latest.json")
    try:
        rec = json.load(open(pmc))
    except Exception:
        return None, None, None
    now = _sha16(os.path.join(ROOT, "3d-shape-generation_amd", "csrc", "gemm_f16.hip"))
    stale = rec.get("kernel_source_sha16") is None or rec.get("kernel_source_sha16") != now
    return rec.get("hbm_bytes_per_launch"), rec.get("git_head"), stale


def measured_mfma_busy(kernel, source):
    """MFMA-pipe utilisation of `kernel` from the committed SQ-counter recipe (tools/pmc_sq.sh -> profiles/sq_pmc_latest.json), with the same staleness rule as
    `measured_traffic`: (fraction, git_head, stale)."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "sq_pmc_latest.json")))
        k = rec["kernels"][kernel]
    except Exception:
        return None, None, None
    now = _sha16(os.path.join(ROOT, "3d-shape-generation_amd", "csrc", source))
    return k.get("mfma_busy"), rec.get("git_head"), (k.get("kernel_source_sha16") != now)


LATENT_WEIGHT_BYTES = 38174720.0              # 19 087 360 fp16 weights streamed per latent step
VAE_DECODE_FLOP_PER_SAMPLE = 40.20e9
VAE_ENCODE_FLOP_PER_SAMPLE = 24.48e9
HBM_PEAK_GBS = 8000.0                         # MI355X_MICROARCH.md: 8 TB/s HBM3E


def build_latent_model(device):
    import numpy as np
    import torch
    from shapegen_amd import specs
    from shapegen_amd.diffusion import LatentDiffusion
    from shapegen_amd.vae import VAE3DLarge
    sd = specs.synth_state_dict(specs.latent_unet_spec(prefix="model."), seed=0, gain=1.3)
    sd.update(specs.synth_state_dict(specs.vae3d_large_spec(prefix="vae."), seed=0, gain=1.3))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    m = LatentDiffusion(VAE3DLarge())
    m.load_state_dict(sd, strict=True)
    return m.to(device).eval(), sd


def latent_legs(m, device, B=32, T=SCHEDULE_STEPS):
    """BASELINE configs[3] on one GPU, piece by piece, inputs resident in HBM: VAE3DLarge.encode of B grids, the T-step
    latent DDIM loop (LatentDiffusion.sample's loop: diffusion.py:637-645), decode + voxel->points; every piece is run
    once untimed first.  HIP events on torch's current stream, which is the stream every kernel of the path is launched on."""
    import torch
    g = torch.Generator().manual_seed(24)
    vox = (torch.rand(B, 1, 32, 32, 32, generator=g) > 0.9).float().to(device)

    def timed(fn, reps, ramp=1):
        # `ramp` untimed calls first: from idle the chip needs tens of milliseconds of load to reach its running clocks (the same ramp the
        # attention legs take: the first chunk of a train of launches measures ~10 % slow); the VAE legs are ~1-ms calls timed in a
        # train of 10, so they get 30 calls (~40 ms) of ramp -- with one warm-up call they were being timed ON the ramp
        for _ in range(ramp):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, (time.perf_counter() - t0) / reps * 1e3, out

    def timed_vae(fn):
        # three trains of 10 calls after one 30-call ramp, the MEDIAN train: a call is ~20 launches of 30-200 us, and one host-side stall during a train
        # (seen: encode 0.965 v. 0.839 ms in two runs on one box minutes apart) would otherwise read as slower kernels
        trains = [timed(fn, 10, ramp=30 if i == 0 else 0) for i in range(3)]
        return sorted(trains, key=lambda r: r[0])[1]

    enc_ms, _, (mu, logvar) = timed_vae(lambda: m.vae.encode(vox))
    zT = m.vae.reparameterize(mu, logvar)

    def loop():
        z = m._start(B, zT)
        tab = m.ddim_table(T, B)
        return m._run(z, tab, m.model.time_bias(tab.t), m._forward_fn(), "ddim")

    # wall clock per call (host table building included); the MEDIAN of three calls: one call is ~36 ms, and a single host-side stall of a few ms
    # on a shared box (seen: 44 v. 36 us per step in two runs minutes apart) would otherwise read as a slower kernel
    walls = []
    for i in range(3):
        _, w_ms, z0 = timed(loop, 1, ramp=1 if i == 0 else 0)
        walls.append(w_ms)
    loop_wall_ms = sorted(walls)[1]
    dec_ms, _, dec = timed_vae(lambda: m.vae.decode(z0))
    _, fin_wall_ms, clouds = timed(lambda: m._finish(z0, 0.4), 3)

    def whole():
        mu_, lv_ = m.vae.encode(vox)
        return m.sample(num_samples=B, num_steps=T, z_T=m.vae.reparameterize(mu_, lv_))

    _, whole_wall_ms, _ = timed(whole, 2)
    if not torch.isfinite(z0).all():
        raise SystemExit("non-finite latents after the latent loop")
    return {"batch": B, "steps": T, "encode_ms": enc_ms, "loop_ms": loop_wall_ms, "latent_us_per_step": loop_wall_ms * 1e3 / T,
            "decode_ms": dec_ms, "decode_and_voxel_to_points_ms": fin_wall_ms, "cfg4_ms": whole_wall_ms,
            "clouds": [int(c.shape[0]) for c in clouds[:4]], "latents": z0, "all_clouds": clouds}


# dependent exchanges of one latent step in csrc/latent_persist.hip's plan and the idle hand-off latencies (profiles/r03_d)
LATENT_EDGES_LOCAL, LATENT_EDGES_CROSS = 12, 6
HANDOFF_LOCAL_US, HANDOFF_CROSS_US = 0.397, 0.920


def latent_rooflines(legs):
    B = legs["batch"]
    step_s = legs["latent_us_per_step"] * 1e-6
    lat = LATENT_WEIGHT_BYTES / step_s / 1e9
    dec = VAE_DECODE_FLOP_PER_SAMPLE * B / (legs["decode_ms"] * 1e-3) / 1e12
    enc = VAE_ENCODE_FLOP_PER_SAMPLE * B / (legs["encode_ms"] * 1e-3) / 1e12
    return ({"bound": "hbm", "kernel": "latent denoiser step (SimpleLatentUNetPointNet forward + DDIM update; all launches of one step)",
             "achieved": lat, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": lat / HBM_PEAK_GBS, "traffic": None,
             "avg_launch_ms": step_s * 1e3, "launches_timed": legs["steps"], "bytes_per_launch": LATENT_WEIGHT_BYTES,
             "note": "algorithmic bytes = the fp16 weights of the 12 Linear layers, streamed once per step (they fit the 256 MB "
                     "Infinity Cache, so the bytes come from on-die cache, not HBM); wall clock of the whole loop / steps",
             # The HBM figure assumes the 12 layers could overlap; they are a chain of all-to-all dependencies.  The bound this kernel
             # can be held to is the chain's hand-off latency: 18 dependent exchanges per step (12 Linear layers + 6 GroupNorm
             # finishes whose group spans workgroups), 12 of them inside one XCD's L2 (plain stores) and 6 across XCDs (write-through),
             # priced at the IDLE one-way store -> load latency tools/ubench_handoff.hip measures (profiles/r03_d): no compute,
             # no operand fetch, no contention.
             "latency_floor_us": LATENT_EDGES_LOCAL * HANDOFF_LOCAL_US + LATENT_EDGES_CROSS * HANDOFF_CROSS_US,
             "frac_of_latency_floor": (LATENT_EDGES_LOCAL * HANDOFF_LOCAL_US + LATENT_EDGES_CROSS * HANDOFF_CROSS_US) / (step_s * 1e6),
             "latency_model": {"edges_same_xcd": LATENT_EDGES_LOCAL, "edges_across_xcds": LATENT_EDGES_CROSS,
                               "handoff_same_xcd_us": HANDOFF_LOCAL_US, "handoff_across_xcds_us": HANDOFF_CROSS_US,
                               "source": "tools/ubench_handoff.hip, profiles/r03_d_handoff_latency.txt"}},
            {"bound": "mfma", "kernel": "VAE3DLarge.decode, batch 32 (all launches of one decode)", "achieved": dec,
             "peak": MFMA_F16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": dec / MFMA_F16_DENSE_PEAK_TFLOPS, "traffic": None,
             "avg_launch_ms": legs["decode_ms"], "launches_timed": 10, "flop_per_launch": VAE_DECODE_FLOP_PER_SAMPLE * B},
            {"bound": "mfma", "kernel": "VAE3DLarge.encode, batch 32 (all launches of one encode)", "achieved": enc,
             "peak": MFMA_F16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": enc / MFMA_F16_DENSE_PEAK_TFLOPS, "traffic": None,
             "avg_launch_ms": legs["encode_ms"], "launches_timed": 10, "flop_per_launch": VAE_ENCODE_FLOP_PER_SAMPLE * B})


def gf3_roofline(gf3_ms, launches, how=None):
    achieved = GF3_FLOP_PER_LAUNCH / (gf3_ms * 1e-3) / 1e12
    traffic, traffic_head, stale = measured_traffic()
    busy, busy_head, busy_stale = measured_mfma_busy("gemm_xw_kernel", "gemm_f16.hip")
    r = {"bound": "mfma", "kernel": "gemm_xw_kernel = the 256x256 tile, 2x4 waves, persistent; activation panel through LDS, fragment-order weights straight from global memory (global_feat.3 2048->4096 + max over N)",
         "achieved": achieved, "peak": MFMA_F16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s",
         "frac": achieved / MFMA_F16_DENSE_PEAK_TFLOPS, "traffic": traffic, "traffic_measured_at": traffic_head,
         "traffic_stale": stale, "mfma_busy": busy, "mfma_busy_measured_at": busy_head, "mfma_busy_stale": busy_stale, "avg_launch_ms": gf3_ms, "launches_timed": launches, "flop_per_launch": GF3_FLOP_PER_LAUNCH}
    if how:
        r["measured"] = how
    return r


def eager_gf3_profile(model, fn):
    """Average duration of the dominant GEMM over the launches `fn` makes, by HIP events on the launch stream inside
    pcd_unet_forward; events cannot be recorded in a captured graph, so `fn` runs with graph replay off."""
    from shapegen_amd import _lib
    lib = _lib.load()
    handle = model.model._handle
    keep = model.use_graphs
    model.use_graphs = False
    try:
        _lib.check(lib.pcd_unet_profile(handle, 1))
        fn()
        tot_ms, launches = C.c_double(0), C.c_int(0)
        _lib.check(lib.pcd_unet_profile_read(handle, C.byref(tot_ms), C.byref(launches)))
        _lib.check(lib.pcd_unet_profile(handle, 0))
    finally:
        model.use_graphs = keep
    return tot_ms.value / max(launches.value, 1), launches.value


# ------------------------------------------------------------------------------------------ cfg2 (headline)
def run_cfg2(args, R: Ranks):
    import torch
    from shapegen_amd import _lib
    from shapegen_amd.diffusion import PointCloudDiffusion, Stepper

    sd = synth_weights(args.backbone)
    kw = {} if args.backbone == "pointnet" else {"backbone": "attention"}
    model = PointCloudDiffusion(num_points=N_POINTS, **kw)
    model.load_state_dict(sd, strict=True)
    model = model.to(R.device).eval()
    total = args.warmup + args.steps
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    tab = model.ddpm_table(SCHEDULE_STEPS, B_PER_GPU)
    bias = model.model.time_bias(tab.t)
    lib = _lib.load()
    pointnet = args.backbone == "pointnet"
    handle = model.model._handle if pointnet else None

    def new_stepper(seed):
        torch.manual_seed(seed)
        x = model._randn_like(torch.empty(B_PER_GPU, N_POINTS, 3, device=model.device))   # x_T resident in HBM
        # the product's own step object (diffusion.Stepper, what sample2() drives): device-side step select +
        # denoiser forward + Philox noise + fused DDPM update, state updated in place
        return x, Stepper(model, x, tab, bias, model._forward_fn(), "ddpm")

    def leg(use_graph, seed):
        x, stp = new_stepper(seed)
        for k in range(args.warmup):
            if k and k % SCHEDULE_STEPS == 0:
                stp.counter.zero_()          # the device-side step counter stops at the last step: start the schedule over
            stp.step(k, True)
        if use_graph:
            stp.capture()
        if pointnet:
            _lib.check(lib.pcd_unet_profile(handle, 0 if use_graph else 1))
        R.sync_all()
        t0 = time.perf_counter()
        for k in range(args.warmup, total):
            if k and k % SCHEDULE_STEPS == 0:
                stp.counter.zero_()
            if use_graph:
                stp.replay()
            else:
                stp.step(k, True)
        R.sync_all()
        elapsed = time.perf_counter() - t0
        tot_ms, launches = C.c_double(0), C.c_int(0)
        if pointnet:
            _lib.check(lib.pcd_unet_profile_read(handle, C.byref(tot_ms), C.byref(launches)))
            _lib.check(lib.pcd_unet_profile(handle, 0))
        if not torch.isfinite(x).all():
            raise SystemExit("non-finite state after the timed steps")
        return R.max_over_ranks(elapsed), tot_ms.value, launches.value, elapsed, x

    # (--full) the set-attention kernel's own roofline first, on an idle chip (100 launches = 27 ms; after the ~1 s of the two legs
    # below the chip is power-throttled, which is a statement about the GEMM run that heated it, not about this kernel)
    att = attention_roofline(R.device) if (args.full and R.world == 1 and not args.no_attention) else None
    head_graph = args.graph or (R.world > 1 and not args.eager)
    elapsed, tot_ms, launches, own, x_head = leg(head_graph, 24 + R.rank)
    outputs = {"x": x_head.float().cpu()} if args.dump_outputs else None        # the sampler state after the last timed step
    if args.full:
        other_elapsed, o_ms, o_launches, _, _ = leg(not head_graph, 24 + R.rank)      # the other launch mode, same K steps
        if head_graph:       # HIP events cannot be recorded inside a captured step: the eager leg carries them
            tot_ms, launches = o_ms, o_launches
    per_rank = R.gather_seconds(own)
    rccl_ranks = R.collective_ranks()
    if R.rank != 0:
        return None, None
    world = R.world
    name = "UNetPointNetLarge" if pointnet else "UNetAttentionPointExperimental"
    out = {
        "metric": "denoising-steps/sec (whole node), 2048-pt DDPM, batch 64",
        "value": world * args.steps / elapsed,
        "unit": "denoising-steps/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f16", "data": "synthetic",
        "config": {"workload": f"BASELINE configs[1]: point-cloud DDPM (sample2), 2048 points, batch 64 per GPU, "
                               f"1000-step cosine schedule, fp16 operands/fp32 accumulate, random-init synthetic weights, "
                               f"denoiser {name}",
                   "batch_per_gpu": B_PER_GPU, "points": N_POINTS, "sampler": "ddpm/sample2", "backbone": args.backbone,
                   "launch": "hipGraph replay" if head_graph else "eager",
                   "point_steps_per_sec": world * args.steps * B_PER_GPU * N_POINTS / elapsed,
                   "rccl_ranks": rccl_ranks, "collective_backend": R.backend,
                   # every rank's own clock over the same K steps: an efficiency loss at N > 1 is attributable to a rank
                   "per_rank_steps_per_sec": {"min": args.steps / max(per_rank), "max": args.steps / min(per_rank),
                                              "slowest_rank": per_rank.index(max(per_rank))},
                   "rank_cpus": os.environ.get("PCD_RANK_CPUS"), "rank_host_threads": os.environ.get("OMP_NUM_THREADS")},
    }
    if args.full:
        out["config"][("eager" if head_graph else "graph_replay") + "_steps_per_sec"] = world * args.steps / other_elapsed
    if pointnet and launches:      # an eager leg ran: its HIP events timed the dominant GEMM
        out["roofline"] = gf3_roofline(tot_ms / launches, launches)
    if att is not None:
        att["measured"] = "before the timed region, after 200 warm-up launches"
        out["roofline_attention"] = att
        if not pointnet:
            out["roofline"] = att
    if args.full and world == 1 and pointnet and not args.no_other_configs:
        oc = other_configs(model, R.device)
        # the headline region is short (K steps of ~3.6 ms); the chip is power limited, so a SUSTAINED figure stands beside it: 200
        # consecutive steps of the same loop through graph replay (25 replays of the 8-step graph sample2() itself uses) after a ramp
        x, stp = new_stepper(24)
        for k in range(8):
            stp.step(k, True)
        stp.capture(8)
        for _ in range(6):
            stp.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(25):
            stp.replay()
        torch.cuda.synchronize()
        oc["cfg2_sustained_200_steps_per_sec"] = 200 / (time.perf_counter() - t0)
        oc["cfg2_sustained_note"] = "200 consecutive DDPM steps (25 replays of an 8-step hipGraph) after 56 steps of ramp, same shapes as the headline"
        # the selectable attention backbone (UNetAttentionPointExperimental, networks.py:597-722) under the same sampler and shapes
        am = PointCloudDiffusion(num_points=N_POINTS, backbone="attention")
        am.load_state_dict(synth_weights("attention"), strict=True)
        am = am.to(R.device).eval()
        abias = am.model.time_bias(tab.t)
        torch.manual_seed(24)
        ax = am._randn_like(torch.empty(B_PER_GPU, N_POINTS, 3, device=am.device))
        astp = Stepper(am, ax, tab, abias, am._forward_fn(), "ddpm")
        for k in range(10):
            astp.step(k, True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(10, 50):
            astp.step(k, True)
        torch.cuda.synchronize()
        oc["attention_backbone_steps_per_sec"] = 40 / (time.perf_counter() - t0)
        if not torch.isfinite(ax).all():
            raise SystemExit("non-finite state in the attention-backbone leg")
        del am, astp, ax
        out["config"]["other_configs"] = oc
    if args.full and world == 1 and not args.no_cpu_baseline and pointnet:
        out["cpu_baseline"] = cpu_baseline(sd)
        out["cpu_baseline_cfg1"] = cpu_baseline_cfg1(sd)
    return out, outputs


def other_configs(model, device):
    """The other single-GPU workloads of BASELINE.json, measured AFTER the headline region so that the driver's default
    line carries them (each is also a `--config` of its own with its own roofline block): configs[2]'s per-GPU workload
    (DDIM `sample`, 50 steps, 64 shapes: whole sampler calls) and configs[3] (latent path at B = 32)."""
    import torch
    T = 50
    model.sample(B_PER_GPU, N_POINTS, num_steps=T)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2):
        model.sample(B_PER_GPU, N_POINTS, num_steps=T)
    torch.cuda.synchronize()
    cfg3 = 2 * T / (time.perf_counter() - t0)
    m, _ = build_latent_model(device)
    legs = latent_legs(m, device)
    lat, dec, enc = latent_rooflines(legs)
    return {"cfg3_ddim50_steps_per_sec": cfg3, "cfg4_ms": legs["cfg4_ms"], "cfg4_steps_per_sec": legs["steps"] / (legs["loop_ms"] * 1e-3),
            "latent_us_per_step": legs["latent_us_per_step"], "latent_step_frac_of_hbm_roofline": lat["frac"],
            "vae_decode_ms": legs["decode_ms"], "vae_decode_frac_of_mfma_peak": dec["frac"],
            "vae_encode_ms": legs["encode_ms"], "vae_encode_frac_of_mfma_peak": enc["frac"],
            "note": "cfg3: two whole DDIM-50 sampler calls at B=64, N=2048 (tables, graph capture included); cfg4: encode 32 grids + "
                    "1000 latent DDIM steps + decode + voxel->points, wall clock; VAE legs by HIP events: the median of three trains of 10 calls after a 30-call clock ramp"}


# ------------------------------------------------------------------------------------------ cfg3
def run_cfg3(args, R: Ranks):
    """BASELINE configs[2]: DDIM `sample`, 2048 points, 50 steps, 64 shapes per GPU (512 on 8 GPUs), batch-sharded;
    the only collective is the all-gather of the output clouds after the loop."""
    import torch
    from shapegen_amd import dist as D
    from shapegen_amd.diffusion import PointCloudDiffusion
    T = 50
    model = PointCloudDiffusion(num_points=N_POINTS)
    model.load_state_dict(synth_weights(), strict=True)
    model = model.to(R.device).eval()
    torch.manual_seed(24)
    runs = max(1, args.steps // T)
    gb = B_PER_GPU * R.world
    for _ in range(max(1, args.warmup // T)):
        D.sample_sharded(model, gb, N_POINTS, T)
    R.sync_all()
    t0 = time.perf_counter()
    for _ in range(runs):
        clouds = D.sample_sharded(model, gb, N_POINTS, T)
    R.sync_all()
    elapsed = R.max_over_ranks(time.perf_counter() - t0)
    ranks = R.collective_ranks()
    assert tuple(clouds.shape) == (gb, N_POINTS, 3) and torch.isfinite(clouds).all()
    # (--full) dominant kernel, timed live after the timed region: one more sampler call with graph replay off (HIP events
    # cannot be recorded inside a captured step), same 50 steps, same shapes
    if args.full:
        gf3_ms, gf3_launches = eager_gf3_profile(model, lambda: D.sample_sharded(model, gb, N_POINTS, T, gather=False))
    if R.rank != 0:
        return None, None
    outputs = {"clouds": clouds.float().cpu()} if args.dump_outputs else None
    steps = runs * T
    out = {"metric": "denoising-steps/sec (whole node), 2048-pt DDIM 50 steps, batch 64 per GPU", "value": R.world * steps / elapsed,
           "unit": "denoising-steps/sec", "n_gpus": R.world, "steps": steps, "warmup": max(1, args.warmup // T) * T,
           "ms_per_step": elapsed / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f16", "data": "synthetic",
           "config": {"workload": "BASELINE configs[2]: point-cloud DDIM (sample), 2048 points, 50 steps, batch 64 per GPU "
                                  "batch-sharded, output clouds all-gathered; whole sampler calls timed (tables, graph capture, gather included)",
                      "global_batch": gb, "runs": runs, "rccl_ranks": ranks, "collective_backend": R.backend}}
    if args.full:
        out["roofline"] = gf3_roofline(gf3_ms, gf3_launches, "eager run of the same 50 steps after the timed region (rank 0)")
    return out, outputs


# ------------------------------------------------------------------------------------------ cfg5
def run_cfg5(args, R: Ranks):
    """BASELINE configs[4]: latent diffusion, 1000 latent DDIM steps on 32 latents per GPU, VAE decode, voxel->points,
    all-gather of the ragged clouds, per-sample Chamfer / Sinkhorn EMD / voxel BCE rows against the input grids' clouds."""
    import torch
    from shapegen_amd import dist as D
    from shapegen_amd.utils import voxel_tensor_to_point_clouds
    B, T = 32, SCHEDULE_STEPS
    m, _ = build_latent_model(R.device)
    torch.manual_seed(24)
    gb = B * R.world
    lo, hi = D.shard_range(gb, R.rank, R.world)
    g = torch.Generator().manual_seed(24)
    vox = (torch.rand(gb, 1, 32, 32, 32, generator=g) > 0.9).float()[lo:hi].to(R.device)
    orig = voxel_tensor_to_point_clouds(vox, 0.5)

    def once():
        R.sync_all()
        t0 = time.perf_counter()
        with D.shard_context(m, lo, gb):
            clouds = m.sample(num_samples=hi - lo, num_steps=T)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        allc = D.all_gather_clouds(clouds)
        rows, mean = D.evaluate_sharded(orig, clouds, use_approximate_gpu_emd=True)
        R.sync_all()
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, allc, rows

    once()
    loop_s, eval_s, allc, rows = once()
    loop_s, eval_s = R.max_over_ranks(loop_s), R.max_over_ranks(eval_s)
    ranks = R.collective_ranks()
    assert len(allc) == gb and rows.shape == (gb, 3)
    if R.rank != 0:
        return None, None
    outputs = ragged(allc) if args.dump_outputs else None
    out = {"metric": "denoising-steps/sec (whole node), latent diffusion 1000 steps, batch 32 per GPU", "value": R.world * T / loop_s,
           "unit": "denoising-steps/sec", "n_gpus": R.world, "steps": T, "warmup": T, "ms_per_step": loop_s / T * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
           "config": {"workload": "BASELINE configs[4]: latent diffusion, 1000 DDIM steps over (32, 256) latents per GPU + VAE3DLarge decode "
                                  "+ voxel->points (timed as the loop), then all-gather of ragged clouds + per-sample Chamfer/Sinkhorn-EMD/voxel-BCE",
                      "global_batch": gb, "eval_seconds": eval_s, "mean_metrics": [float(v) for v in rows.nanmean(dim=0)],
                      "rccl_ranks": ranks, "collective_backend": R.backend}}
    if args.full:        # after the timed region: the latent step / decode on their own (rank 0)
        lat, dec, _ = latent_rooflines(latent_legs(m, R.device))
        out["roofline"], out["roofline_vae_decode"] = lat, dec
    return out, outputs


# ------------------------------------------------------------------------------------------ cfg4
def run_cfg4(args, R: Ranks):
    """BASELINE configs[3]: VAE3DLarge.encode of 32 grids -> 1000 latent DDIM steps (`LatentDiffusion.sample`,
    diffusion.py:619-653) -> decode -> voxel->points, one GPU per rank (replicas when N > 1: no collective on this path)."""
    m, sd = build_latent_model(R.device)
    R.sync_all()
    legs = latent_legs(m, R.device)
    R.sync_all()
    loop_s = R.max_over_ranks(legs["loop_ms"] * 1e-3)
    ranks = R.collective_ranks()
    if R.rank != 0:
        return None, None
    outputs = dict(latents=legs["latents"].float().cpu(), **ragged(legs["all_clouds"])) if args.dump_outputs else None
    lat, dec, enc = latent_rooflines(legs)
    T = legs["steps"]
    out = {"metric": "denoising-steps/sec (whole node), latent diffusion 1000 steps, batch 32 per GPU", "value": R.world * T / loop_s,
           "unit": "denoising-steps/sec", "n_gpus": R.world, "steps": T, "warmup": T, "ms_per_step": loop_s / T * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
           "config": {"workload": "BASELINE configs[3]: latent diffusion on one GPU per rank: VAE3DLarge encode of 32 voxel grids, 1000 DDIM steps over "
                                  "(32, 256) latents (timed as the loop: value), VAE3DLarge decode, voxel->points; synthetic weights",
                      "batch_per_gpu": legs["batch"], "encode_ms": legs["encode_ms"], "decode_ms": legs["decode_ms"],
                      "decode_and_voxel_to_points_ms": legs["decode_and_voxel_to_points_ms"], "cfg4_ms_end_to_end": legs["cfg4_ms"],
                      "latent_us_per_step": legs["latent_us_per_step"], "clouds_first4": legs["clouds"],
                      "rccl_ranks": ranks, "collective_backend": R.backend},
           "roofline": lat, "roofline_vae_decode": dec, "roofline_vae_encode": enc}
    if args.full and R.world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_latent(sd)
    return out, outputs


def main():
    args = parse_args()
    # (several ranks on ONE GPU, PCD_BENCH_SHARE_GPU=1: the library itself keeps the persistent latent kernel off when ranks of
    # a job share a device -- LatentDiffusion._persistent_allowed -- and falls back if a launch cannot complete)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_children(args))           # the parent stays GPU-free
    if args.gpus > 1:
        # a rank that `python -m torch.distributed.run` started (the driver's N > 1 form): its CPU slice and thread budget, before torch
        # is imported (ranks of launch_children come pinned already and this is a no-op)
        from shapegen_amd import launcher
        launcher.apply_rank_affinity()

    import torch
    import shapegen_amd  # noqa: F401
    torch.set_grad_enabled(False)
    R = Ranks(args)
    out, outputs = {"cfg2": run_cfg2, "cfg3": run_cfg3, "cfg4": run_cfg4, "cfg5": run_cfg5}[args.config](args, R)
    if R.rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, outputs)
        print(json.dumps(out), flush=True)
    R.finish()


if __name__ == "__main__":
    main()
