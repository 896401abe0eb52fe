"""Diffusion processes with the reference's Python surface (reference diffusion.py):
`PointCloudDiffusion` (:14-358) and `LatentDiffusion` (:361-734).

Host code only sequences the loop: the per-step constants (continuous-time t sequence,
noise/signal rates) are computed on the host CPU with the reference's exact torch ops so
that step indexing is bit-exact, uploaded once per call, and every
per-timestep computation runs in HIP kernels (`_lib`).  The training surface (`training_step`,
`diffusion_loss`, `configure_optimizers`) forwards to the HIP trainers in `training.py`.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from .networks import UNetPointNetLarge


class _HParams(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


# ------------------------------------------------------------------ host schedule math
def _offset_cosine(t: torch.Tensor, min_signal: float, max_signal: float):
    """diffusion.py:208-223, on CPU tensors."""
    a0 = torch.acos(torch.tensor(max_signal))
    a1 = torch.acos(torch.tensor(min_signal))
    ang = a0 + t * (a1 - a0)
    return torch.sin(ang), torch.cos(ang)


def _linear(t: torch.Tensor, lo: float, hi: float, dim: int = 0):
    """diffusion.py:189-205 (bug-for-bug: cumprod over the batch axis, which is `dim` of t)."""
    betas = lo + t.clone() * (hi - lo)
    abar = torch.cumprod(1 - betas, dim=dim)
    return 1 - abar, abar


class StepTable:
    """Per-step scalars of one sampler run as fp32 device matrices (T, R): R = 1 when every
    shape shares the rates (cosine schedule), R = batch for the linear schedule whose
    batch-axis cumprod (diffusion.py:202) gives each shape its own rates.  `skip_last_update`:
    the last row only predicts x_0 (the reference's `sample` alone updates the state after its last prediction)."""

    @staticmethod
    def _col(v: torch.Tensor, device):
        return v.to(torch.float32).reshape(v.shape[0], -1).contiguous().to(device)

    def __init__(self, t, n, s, a, b, device, skip_last_update: bool = False):
        f = lambda v: self._col(v, device)
        self.t, self.n, self.s, self.a, self.b = f(t.reshape(t.shape[0], -1)[:, :1]).reshape(-1), f(n), f(s), f(a), f(b)
        self.steps = t.shape[0]
        self.width = self.n.shape[1]
        self.stride = 0 if self.width == 1 else 1
        self.skip_last_update = skip_last_update

    def offset(self, k: int) -> int:
        return 4 * k * self.width

    def columns(self) -> List[torch.Tensor]:
        """The per-step rate tables in the order the update kernels read them."""
        return [self.n, self.s, self.a, self.b]


def completion_rows(num_steps: int, jump: int, resample: int) -> List[Tuple[int, Optional[int]]]:
    """The walk of `complete` over time indices, one entry per network evaluation: (i, None) steps from i to i - 1;
    (i, to) steps to i - 1 and is then thrown forward to index `to` = i - 1 + jump.  RePaint's schedule: every index in
    range(0, T - jump, jump) is left `resample - 1` times by a jump before the walk passes it."""
    left = {k: resample - 1 for k in range(0, num_steps - jump, jump)} if resample > 1 else {}
    rows, i = [], num_steps - 1
    while i > 0:
        lands = i - 1
        if left.get(lands, 0) > 0:
            left[lands] -= 1
            rows.append((i, lands + jump))
            i = lands + jump
        else:
            rows.append((i, None))
            i = lands
    rows.append((0, None))
    return rows


class CompletionTable(StepTable):
    """StepTable of `complete`: the DDPM columns plus n_prev (known rows) and the forward jump ja, jb (0, 0 on a row without
    one).  `draws[k]` is the index of row k's first normal draw in consumption order; a jump row uses `draws[k] + 1` too."""

    def __init__(self, rows, t, n, s, a, b, n2, ja, jb, device):
        super().__init__(t, n, s, a, b, device, skip_last_update=True)
        self.n2, self.ja, self.jb = (self._col(c, device) for c in (n2, ja, jb))
        self.rows = rows
        self.jumps = any(to is not None for _, to in rows)
        self.draws, j = [], 0
        for _, to in rows:
            self.draws.append(j)
            j += 1 if to is None else 2

    def columns(self) -> List[torch.Tensor]:
        return [self.n, self.s, self.a, self.b, self.n2, self.ja, self.jb]


class DpmTable(StepTable):
    """StepTable of `sample_dpm`: the DDIM columns n, s, n_next, s_next plus the multistep coefficient c = h_k / (2 h_{k-1}) (0 on
    the first row and for order 1) and q = s / n.  `skip_last_update`: the log-SNR grid ends at t_last and its last row only
    predicts x_0; the uniform grid's last row updates as `sample`'s does."""

    def __init__(self, t, n, s, n2, s2, c, q, device, skip_last_update: bool):
        super().__init__(t, n, s, n2, s2, device, skip_last_update)
        self.c, self.q = self._col(c, device), self._col(q, device)

    def columns(self) -> List[torch.Tensor]:
        return [self.n, self.s, self.a, self.b, self.c, self.q]


class _DiffusionBase(nn.Module):
    """Schedule + elementwise ops + the three sampler loops, shared by both processes."""

    def _init_schedule(self, noise_schedule: str):
        self.noise_schedule = noise_schedule
        self.linear_min_rate, self.linear_max_rate = 0.0001, 0.02
        self.cosine_min_signal_rate, self.cosine_max_signal_rate = 0.02, 0.95
        self.diffusion_schedule = (self.offset_cosine_diffusion_schedule if noise_schedule == "cosine"
                                   else self.linear_diffusion_schedule)

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    # reference diffusion.py:208-223 / 189-205: computed on the host, returned on t's device
    def offset_cosine_diffusion_schedule(self, diffusion_times: torch.Tensor):
        n, s = _offset_cosine(diffusion_times.detach().to("cpu", torch.float32),
                              self.cosine_min_signal_rate, self.cosine_max_signal_rate)
        return n.to(diffusion_times.device), s.to(diffusion_times.device)

    def linear_diffusion_schedule(self, diffusion_times: torch.Tensor):
        n, s = _linear(diffusion_times.detach().to("cpu", torch.float32), self.linear_min_rate, self.linear_max_rate)
        return n.to(diffusion_times.device), s.to(diffusion_times.device)

    # ------------------------------------------------------------------ elementwise ops
    def _rates(self, v: torch.Tensor, batch: int) -> Tuple[torch.Tensor, int]:
        v = v.to(self.device, torch.float32).reshape(-1).contiguous()
        if v.numel() == 1:
            return v, 0
        if v.numel() != batch:
            raise ValueError(f"rates have {v.numel()} entries for a batch of {batch}")
        return v, 1

    # Philox stream layout.  One draw of a (batch, ...) tensor consumes `span` counters (4 normals each); a process
    # that holds samples [lo, lo + b) of a global batch of `total` (set by dist.shard_context) reads the
    # sub-block that starts `lo * per-sample counters` into the draw and advances by the GLOBAL span, so ranks
    # never share counters and (per-sample size divisible by 4) sample i gets the same numbers whatever the
    # number of ranks.
    _shard = None

    def _philox_span(self, numel: int, batch: int) -> Tuple[int, int]:
        per4 = (numel // max(batch, 1) + 3) // 4
        lo, total = self._shard if self._shard is not None else (0, batch)
        return lo * per4, max(total, batch) * per4

    def _randn_like(self, x: torch.Tensor) -> torch.Tensor:
        out = torch.empty_like(x, dtype=torch.float32)
        seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self._philox_offset = getattr(self, "_philox_offset", 0)
        batch = x.shape[0] if x.dim() > self._sample_dims else 1
        shard_off, span = self._philox_span(out.numel(), batch)
        _lib.check(_lib.load().pcd_randn(out.data_ptr(), out.numel(), seed, self._philox_offset + shard_off,
                                         _lib.stream_ptr()), "randn")
        self._philox_offset += span
        return out

    def add_noise(self, x_0: torch.Tensor, t: torch.Tensor, noise: Optional[torch.Tensor] = None):
        """diffusion.py:138-152 -> (x_t, noise, noise_rates, signal_rates).  `noise` may be injected."""
        self._require_cuda(x_0)
        x_0 = x_0.to(torch.float32).contiguous()
        if noise is None:
            noise = self._randn_like(x_0)
        noise = noise.to(self.device, torch.float32).contiguous()
        noise_rates, signal_rates = self.diffusion_schedule(t)
        b = x_0.shape[0] if x_0.dim() > self._sample_dims else 1
        n, st = self._rates(noise_rates, b)
        s, _ = self._rates(signal_rates, b)
        x_t = torch.empty_like(x_0)
        _lib.check(_lib.load().pcd_add_noise(x_0.data_ptr(), noise.data_ptr(), n.data_ptr(), s.data_ptr(), st,
                                             x_0.numel(), x_0.numel() // b, x_t.data_ptr(), _lib.stream_ptr()), "add_noise")
        if x_0.dim() == self._sample_dims:   # the reference's rates.view(-1,1,1) broadcast adds a batch axis
            x_t = x_t.unsqueeze(0)
        return x_t, noise, noise_rates, signal_rates

    def remove_noise(self, x_t, predicted_noise, noise_rates, signal_rates):
        """diffusion.py:154-168."""
        self._require_cuda(x_t, predicted_noise)
        x_t = x_t.to(torch.float32).contiguous()
        eps = predicted_noise.to(torch.float32).contiguous()
        b = x_t.shape[0]
        n, st = self._rates(noise_rates, b)
        s, _ = self._rates(signal_rates, b)
        x0 = torch.empty_like(x_t)
        _lib.check(_lib.load().pcd_remove_noise(x_t.data_ptr(), eps.data_ptr(), n.data_ptr(), s.data_ptr(), st,
                                                x_t.numel(), x_t.numel() // b, x0.data_ptr(), _lib.stream_ptr()), "remove_noise")
        return x0

    def _require_cuda(self, *ts):
        if self.device.type != "cuda":
            raise RuntimeError("this framework runs only on an MI355X device: call .to('cuda') first")
        for t in ts:
            if t is not None and t.device != self.device:
                raise RuntimeError(f"tensor on {t.device}, model on {self.device}")
        _lib.load()

    # --------------------------------------------------------------- per-step tables
    def _width(self, batch: int) -> int:
        return 1 if self.noise_schedule == "cosine" else batch

    def _host_schedule(self, t: torch.Tensor, width: int = 1):
        """Rates of the (T,) times `t` as (T, width) matrices, all T steps in one set of elementwise ops: row k holds what the
        reference's schedule call returns for a (width,) vector of t[k] (the same fp32 operations per element; the linear
        schedule's batch-axis cumprod runs along the row, and over a row of one element -- `sample3`'s 0-d t -- is the identity).
        tests/table_statement.py is the per-step loop these are checked against, bit for bit."""
        t = t[:, None].expand(-1, width)
        if self.noise_schedule == "cosine":
            return _offset_cosine(t, self.cosine_min_signal_rate, self.cosine_max_signal_rate)
        return _linear(t, self.linear_min_rate, self.linear_max_rate, dim=-1)

    def ddim_table(self, num_steps: int, batch: int = 1) -> StepTable:
        """`sample` (diffusion.py:277-286): t_k = 1 - k/T, next_t = t_k - 1/T.  k * step is formed in float64 and rounded
        once, like the Python scalar in the reference's `ones - k * step`."""
        w = self._width(batch)
        step = 1.0 / num_steps
        t = torch.ones(num_steps) - (torch.arange(num_steps, dtype=torch.float64) * step).to(torch.float32)
        n, s = self._host_schedule(t, w)
        n2, s2 = self._host_schedule(t - step, w)
        return StepTable(t, n, s, n2, s2, self.device)

    def _ddpm_columns(self, i: torch.Tensor, num_steps: int, width: int):
        """`sample2`'s scalars (diffusion.py:241-255) at the fp32 time indices `i`, of which only the last is 0:
        t = i/T, n, s, a = sqrt(n_prev/n), b = s_prev, n_prev."""
        one = torch.ones(i.shape[0])
        t = one * i / num_steps
        n, s = self._host_schedule(t, width)
        npv, sp = self._host_schedule(one * (i - 1) / num_steps, width)
        co = torch.sqrt(npv / n)
        return t, n, s, co, sp, npv

    def ddpm_table(self, num_steps: int, batch: int = 1) -> StepTable:
        """`sample2` (diffusion.py:241-255): t = i/T for i = T-1..0; a = sqrt(n_prev/n), b = s_prev."""
        i = torch.arange(num_steps - 1, -1, -1, dtype=torch.float32)
        t, n, s, co, sp, _ = self._ddpm_columns(i, num_steps, self._width(batch))
        co[-1], sp[-1] = 0.0, 0.0                                  # i = 0: x_t = x_0, no update
        return StepTable(t, n, s, co, sp, self.device, skip_last_update=True)

    def from_state_table(self, start_t0, num_steps: int) -> StepTable:
        """`sample3` (diffusion.py:323-335): linspace(start_t[0], 0, T); only start_t[0] is used,
        and the schedule sees a 0-d t, so the rates are shared by the batch for both schedules."""
        steps = torch.linspace(torch.as_tensor(start_t0, dtype=torch.float32).cpu().reshape(()),
                               torch.zeros(1)[0], num_steps)
        n, s = self._host_schedule(steps)
        n2, s2 = torch.zeros_like(n), torch.zeros_like(s)
        n2[:-1], s2[:-1] = n[1:], s[1:]
        return StepTable(steps, n, s, n2, s2, self.device, skip_last_update=True)

    def completion_table(self, num_steps: int, jump: int = 10, resample: int = 1, batch: int = 1) -> CompletionTable:
        """`complete`: one row per network evaluation (`completion_rows`).  n, s, a, b are `ddpm_table`'s at the row's index i,
        n_prev goes with s_prev, and a row that jumps to index `to` carries ja = s(to/T) / s_prev, jb = sqrt(1 - ja^2), formed in
        float64 and rounded once (exact for the cosine schedule, s^2 + n^2 = 1); ja = jb = 0 marks a row without a jump."""
        w = self._width(batch)
        rows = completion_rows(num_steps, jump, resample)
        L = len(rows)
        t, n, s, co, sp, npv = self._ddpm_columns(torch.tensor([r[0] for r in rows], dtype=torch.float32), num_steps, w)
        to = torch.tensor([r[0] if r[1] is None else r[1] for r in rows], dtype=torch.float32)
        _, sb = self._host_schedule(torch.ones(L) * to / num_steps, w)
        ja = sb.double() / sp.double()
        jb = torch.sqrt(1 - ja * ja)
        has = torch.tensor([r[1] is not None for r in rows])[:, None]
        ja, jb = torch.where(has, ja.float(), torch.zeros(())), torch.where(has, jb.float(), torch.zeros(()))
        co[-1], sp[-1], npv[-1] = 0.0, 0.0, 0.0                     # i = 0: the result is x_0, no update
        return CompletionTable(rows, t, n, s, co, sp, npv, ja, jb, self.device)

    @staticmethod
    def _check_dpm_args(num_steps, order, spacing, t_last):
        if int(num_steps) < 1:
            raise ValueError(f"num_steps must be >= 1, got {num_steps}")
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, got {order!r}")
        if spacing not in ("logsnr", "uniform"):
            raise ValueError(f"spacing must be 'logsnr' or 'uniform', got {spacing!r}")
        if not 0.0 < float(t_last) < 1.0:
            raise ValueError(f"t_last must lie in (0, 1), got {t_last}")

    def dpm_table(self, num_steps: int, order: int = 2, spacing: str = "logsnr", t_last: float = 1e-3) -> DpmTable:
        """`sample_dpm` (not in the reference): DPM-Solver++ 2M on a grid uniform in log-SNR, lambda(t) = log(cos ang / sin ang) with
        ang = a0 + t (a1 - a0).  "logsnr": lambda_k runs linearly from lambda(1) to lambda(t_last) and t_k is its inverse, formed in
        float64 and rounded once to fp32 (t_0 = 1 and t_{K-1} = t_last exactly); the rates are the reference schedule's at the fp32
        time the network sees, and the last row only predicts.  "uniform": `ddim_table`'s rows.  q = s / n, h_k = log(s2 / n2) -
        log(s / n) and c_k = h_k / (2 h_{k-1}) are formed from the fp32 rates in float64 and rounded once.  tests/dpm_statement.py."""
        self._check_dpm_args(num_steps, order, spacing, t_last)
        if self.noise_schedule != "cosine":
            raise ValueError("sample_dpm needs the cosine schedule (the linear schedule's batch-axis cumprod has no monotone log-SNR); "
                             f"got schedule {self.noise_schedule!r}")
        K = int(num_steps)
        if spacing == "uniform":
            base = self.ddim_table(K, 1)
            t, n, s, n2, s2 = (v.cpu().reshape(-1) for v in (base.t, base.n, base.s, base.a, base.b))
            updates = K
        else:
            a0, a1 = math.acos(self.cosine_max_signal_rate), math.acos(self.cosine_min_signal_rate)
            lam = lambda u: math.log(math.cos(a0 + u * (a1 - a0)) / math.sin(a0 + u * (a1 - a0)))
            l0, l1 = lam(1.0), lam(float(t_last))
            ts = [1.0] + [(math.atan(math.exp(-(l0 + (l1 - l0) * k / (K - 1)))) - a0) / (a1 - a0) for k in range(1, K - 1)]
            if K > 1:
                ts.append(float(t_last))
            t = torch.tensor(ts, dtype=torch.float64).to(torch.float32)
            if K > 1 and not bool((t[1:] < t[:-1]).all()):
                raise ValueError(f"the log-SNR grid of {K} steps down to t_last = {t_last} is not strictly decreasing in fp32")
            n, s = (v.reshape(-1) for v in self._host_schedule(t))
            n2, s2 = torch.zeros(K), torch.zeros(K)
            n2[:-1], s2[:-1] = n[1:], s[1:]
            updates = K - 1
        c, q, h_prev = [0.0] * K, [0.0] * K, None
        for k in range(updates):
            nk, sk, n2k, s2k = (float(v[k]) for v in (n, s, n2, s2))
            q[k] = sk / nk
            h = math.log(s2k / n2k) - math.log(sk / nk)
            if order == 2 and k > 0:
                c[k] = h / (2.0 * h_prev)
            h_prev = h
        c, q = (torch.tensor(v, dtype=torch.float64).to(torch.float32) for v in (c, q))
        return DpmTable(t, n, s, n2, s2, c, q, self.device, skip_last_update=updates < K)

    # ------------------------------------------------------------------ class conditioning
    def _guide(self, labels, guidance_scale, batch: int):
        """Validate `labels` / `guidance_scale` on the host.  None for a model without classes (labels or a scale other
        than 1 raise), else the Stepper's (class_bias, labels (B,) int32, w): w is None when every scale is exactly 1 (the
        unconditional forward is skipped), a (1,) fp32 tensor for one scale, (B,) for one per shape."""
        w = torch.as_tensor(guidance_scale).detach().to("cpu")
        if w.is_complex() or w.dtype == torch.bool or w.dim() > 1 or (w.dim() == 1 and w.shape[0] != batch):
            raise ValueError(f"guidance_scale must be a number or a ({batch},) tensor, got {tuple(w.shape)} {w.dtype}")
        w = w.to(torch.float32)
        if not bool(torch.isfinite(w).all()):
            raise ValueError("guidance_scale must be finite")
        off = bool((w == 1.0).all())
        if not getattr(self, "num_classes", 0):
            if labels is not None:
                raise ValueError("labels were given to a model without classes (num_classes=0)")
            if not off:
                raise ValueError("guidance_scale other than 1 needs a class-conditional model (num_classes > 0)")
            return None
        lab = self.model.check_labels(labels, batch)
        return self.model.class_bias(), lab, None if off else w.reshape(-1).to(self.device).contiguous()

    def _split_batch(self, batch):
        """(shapes, labels or None) of a training batch: a tensor, or a (shapes, labels) pair."""
        if isinstance(batch, (tuple, list)):
            if len(batch) != 2:
                raise ValueError(f"a labelled batch is (shapes, labels), got {len(batch)} entries")
            return batch[0], batch[1]
        return batch, None

    def _training_labels(self, labels, batch: int, drop: bool):
        """Device labels of a training (drop: each replaced by the null class with probability p_uncond, one torch.rand draw
        after t's) or validation batch.  A model without classes draws nothing and returns None."""
        if not getattr(self, "num_classes", 0):
            if labels is not None:
                raise ValueError("a labelled batch was given to a model without classes (num_classes=0)")
            return None
        lab = self.model.check_labels(labels, batch)
        if drop:
            null = torch.full_like(lab, self.num_classes)
            lab = torch.where(torch.rand(batch, device=self.device) < self.p_uncond, null, lab)
        return lab

    # ------------------------------------------------------------------ stepping
    GRAPH_MIN_STEPS = 8
    GRAPH_STEPS = 8            # timesteps captured per HIP graph (one graph launch costs ~10 us of host time: the
    use_graphs = True          # 100 us latent step was launch-bound at one step per graph)

    def _run(self, x, tab: "StepTable", bias_table: torch.Tensor, forward, kind: str, noises=None, known=None, guide=None):
        """kind 'ddim' | 'ddpm' | 'dpm' (`tab` a DpmTable) | 'complete' (`known` = (p, counts) on the device, `tab` a CompletionTable).
        forward(x, tb_cur, eps_out) enqueues the denoiser for the current step.  `guide` = (class_bias, labels, w) of a
        class-conditional run (`PointCloudDiffusion._guide`)."""
        stp = Stepper(self, x, tab, bias_table, forward, kind, noises, known, guide)
        T = tab.steps
        n_uniform = T - 1 if tab.skip_last_update else T              # steps that all look the same
        k = 0
        if self.use_graphs and noises is None and n_uniform - 1 >= self.GRAPH_MIN_STEPS:
            stp.step(0, True)                                          # eager warm-up (loads every kernel)
            per = self.GRAPH_STEPS
            stp.capture(per)
            k = 1
            while k + per <= n_uniform:
                stp.replay()
                k += per
        while k < n_uniform:                                           # without graphs, or their remainder: eager, same enqueue
            stp.step(k, True)
            k += 1
        if k < T:
            stp.step(k, False)
        if stp.spans:                                                  # every row consumed its spans, the last one's unread
            self._philox_offset = stp.philox_start + stp.philox_stride * T
        return stp.x0

    def _run_table(self, x, tab: "StepTable", kind: str, **kw):
        return self._run(x, tab, self.model.time_bias(tab.t), self._forward_fn(), kind, **kw)

    def _run_from_state(self, num_samples, fresh, x, start_t, num_steps, **kw):
        """`sample3` (diffusion.py:306-337): DDIM from the given state and time, or (x None) from `fresh()` at t = 1."""
        self.eval()
        if x is None:
            x, start_t = fresh(), None
        else:
            x = x.to(self.device, torch.float32).contiguous().clone()
        if start_t is None:
            start_t = torch.ones(num_samples)
        return self._run_table(x, self.from_state_table(start_t.reshape(-1)[0], num_steps), "ddim", **kw)

    def _l1_loss(self, pred, noise):
        """mean |pred - noise| of an eval-mode `diffusion_loss`."""
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        scratch = torch.empty_like(pred)
        _lib.check(_lib.load().pcd_l1_loss(pred.data_ptr(), noise.data_ptr(), pred.numel(), 1.0, out.data_ptr(), scratch.data_ptr(),
                                           _lib.stream_ptr()), "l1_loss")
        return out[0] / pred.numel()


class Stepper:
    """One timestep = select (device side: copy step k's time bias and rates to fixed buffers, k++) ->
    denoiser forward -> fused update, all on fixed pointers and with the state updated in place, so the
    same enqueue is valid for every k.  Long runs capture it once in a HIP graph and replay it (host
    cost per step: one graph launch instead of ~30 kernel launches).

    With `guide` = (class_bias (rows, tb_elems), labels (B,) int32, w (1,) | (B,) fp32 | None) the select composes one bias row
    per shape plus the null-class row (`pcd_step_select_labels`), the forward is conditional, and unless w is None (every
    guidance scale exactly 1) a second, unconditional forward of the same x and `pcd_cfg_combine` follow; eps then holds the
    guided prediction the update kernel reads.  Without `guide` the enqueue is what it was before guidance existed."""

    KINDS = ("ddim", "ddpm", "dpm", "complete")

    def __init__(self, owner, x, tab: StepTable, bias_table, forward, kind, noises=None, known=None, guide=None):
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {', '.join(map(repr, self.KINDS))}, got {kind!r}")
        self.lib = _lib.load()
        self.x, self.tab, self.forward, self.kind, self.noises = x, tab, forward, kind, noises
        dev = x.device
        self.T, self.R = tab.steps, tab.width
        self.rates = torch.stack(tab.columns()).contiguous()                     # (4, T, R); (6, T, R) 'dpm', (7, T, R) 'complete'
        self.cols = self.rates.shape[0]
        self.bias_table = bias_table.contiguous()
        self.tb_elems = self.bias_table.shape[1]
        self.counter = torch.zeros(2, dtype=torch.int32, device=dev)
        self.tb_cur = torch.empty(self.tb_elems, dtype=torch.float32, device=dev)
        self.rates_cur = torch.empty(self.cols * self.R, dtype=torch.float32, device=dev)
        self.eps = torch.empty_like(x)
        self.guide = guide
        if guide is not None:
            self.class_bias, self.labels, self.w = guide
            self.tb_rows = torch.empty(x.shape[0] + 1, self.tb_elems, dtype=torch.float32, device=dev)
            self.tb_null = self.tb_rows[x.shape[0]]
            self.eps_u = torch.empty_like(x) if self.w is not None else None
        self.x0 = torch.empty_like(x)
        self.per_shape = x.numel() // x.shape[0]
        self.seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        shard_off, span = owner._philox_span(x.numel(), x.shape[0])   # counters one (global) draw consumes
        self.philox_start = getattr(owner, "_philox_offset", 0)        # the owner's stream position before this run
        self.philox_base = self.philox_start + shard_off              # this process's sub-block of every draw
        # What a kind is, besides its table's columns and last-row rule: the update entry, the scratch its injected draws need,
        # and the Philox spans a row consumes.
        buf = lambda: torch.empty_like(x) if noises is not None else None
        self.z = self.z2 = None
        if kind == "ddim":
            self._update, self.spans = self._ddim, 0
        elif kind == "dpm":
            self._update, self.spans = self._dpm, 0
        elif kind == "ddpm":
            self._update, self.spans = self._ddpm_philox if noises is None else self._ddpm_injected, 1
            self.z = buf()
        else:
            # a run with jumps gives EVERY row two spans (z, then z2: unused where the row has no jump), so one captured
            # step fits all rows; a run without consumes sample2's counters
            self._update, self.spans = self._complete_philox if noises is None else self._complete_injected, 2 if tab.jumps else 1
            self.p, self.counts = known
            self.row_elems = x.shape[-1]
            self.z = buf()
            self.z2 = buf() if tab.jumps else None
            self.philox_z2 = span
        self.philox_stride = span * self.spans
        self.graph = None

    def step(self, k: int, update: bool = True):
        lib, x = self.lib, self.x
        st = _lib.stream_ptr()
        rp = self.rates_cur.data_ptr()
        if self.guide is None:
            _lib.check(lib.pcd_step_select_cols(self.counter.data_ptr(), self.T, self.bias_table.data_ptr(), self.tb_elems,
                                                self.tb_cur.data_ptr(), self.rates.data_ptr(), self.cols, self.R, rp, st), "step_select")
            self.forward(x, self.tb_cur, self.eps)
        else:
            cb = self.class_bias
            _lib.check(lib.pcd_step_select_labels(self.counter.data_ptr(), self.T, self.bias_table.data_ptr(), self.tb_elems,
                                                  self.tb_rows.data_ptr(), cb.data_ptr(), cb.shape[0], self.labels.data_ptr(), x.shape[0],
                                                  cb.shape[0] - 1, self.rates.data_ptr(), self.cols, self.R, rp, st), "step_select_labels")
            self.forward(x, self.tb_rows, self.eps, 1)
            if self.w is not None:                        # same x, same workspace: eps_u, then eps = eps_u + w (eps - eps_u)
                self.forward(x, self.tb_null, self.eps_u, 0)
                _lib.check(lib.pcd_cfg_combine(self.eps.data_ptr(), self.eps_u.data_ptr(), self.w.data_ptr(), int(self.w.numel() > 1),
                                               x.numel(), self.per_shape, st), "cfg_combine")
        self._update(k, x.data_ptr() if update else 0, st)   # in place: every element is read before it is written

    # ---- the update entries: (row k, x_next pointer or 0 on a row that only predicts x_0, stream)
    def _inject(self, buf, j: int) -> int:
        buf.copy_(self.noises[j].to(self.x.device, torch.float32).reshape(buf.shape))
        return buf.data_ptr()

    def _ddim(self, k: int, nxt: int, st: int):
        x, R, rp = self.x, self.R, self.rates_cur.data_ptr()
        _lib.check(self.lib.pcd_ddim_update(x.data_ptr(), self.eps.data_ptr(), rp, rp + 4 * R, rp + 8 * R, rp + 12 * R,
                                            self.tab.stride, x.numel(), self.per_shape, self.x0.data_ptr(), nxt, st), "ddim_update")

    def _dpm(self, k: int, nxt: int, st: int):            # x0 is also the history: the previous step's x0 is read, this step's written
        x = self.x
        _lib.check(self.lib.pcd_dpm_update(x.data_ptr(), self.eps.data_ptr(), self.rates_cur.data_ptr(), self.R, self.tab.stride,
                                           x.numel(), self.per_shape, self.x0.data_ptr(), nxt, st), "dpm_update")

    def _ddpm_injected(self, k: int, nxt: int, st: int):
        x, R, rp = self.x, self.R, self.rates_cur.data_ptr()
        zp = self._inject(self.z, k) if nxt else 0
        _lib.check(self.lib.pcd_ddpm_update(x.data_ptr(), self.eps.data_ptr(), zp, rp, rp + 4 * R, rp + 8 * R, rp + 12 * R,
                                            self.tab.stride, x.numel(), self.per_shape, self.x0.data_ptr(), nxt, st), "ddpm_update")

    def _ddpm_philox(self, k: int, nxt: int, st: int):
        if not nxt:                                       # the last row draws nothing: the plain kernel predicts x_0
            return self._ddpm_injected(k, 0, st)
        # on-device noise: the draw and the update are one launch (z is never stored; bitwise pcd_randn_step + pcd_ddpm_update)
        x, R, rp = self.x, self.R, self.rates_cur.data_ptr()
        _lib.check(self.lib.pcd_ddpm_update_philox(x.data_ptr(), self.eps.data_ptr(), rp, rp + 4 * R, rp + 8 * R, rp + 12 * R,
                                                   self.tab.stride, x.numel(), self.per_shape, self.x0.data_ptr(), nxt, self.seed,
                                                   self.philox_base, self.philox_stride, self.counter.data_ptr(), st),
                   "ddpm_update_philox")

    def _complete_philox(self, k: int, nxt: int, st: int):
        x, tab = self.x, self.tab
        _lib.check(self.lib.pcd_complete_update_philox(x.data_ptr(), self.eps.data_ptr(), self.p.data_ptr(), self.counts.data_ptr(),
                                                       self.rates_cur.data_ptr(), self.R, tab.stride, x.numel(), self.per_shape,
                                                       self.row_elems, int(tab.jumps), self.x0.data_ptr(), nxt, self.seed,
                                                       self.philox_base, self.philox_stride, self.philox_z2, self.counter.data_ptr(),
                                                       st), "complete_update_philox")

    def _complete_injected(self, k: int, nxt: int, st: int):
        x, tab = self.x, self.tab
        zp = z2p = 0
        if nxt:
            j = tab.draws[k]
            zp = self._inject(self.z, j)
            if tab.rows[k][1] is not None:
                z2p = self._inject(self.z2, j + 1)
        _lib.check(self.lib.pcd_complete_update(x.data_ptr(), self.eps.data_ptr(), zp, z2p, self.p.data_ptr(), self.counts.data_ptr(),
                                                self.rates_cur.data_ptr(), self.R, tab.stride, x.numel(), self.per_shape, self.row_elems,
                                                self.x0.data_ptr(), nxt, st), "complete_update")

    def capture(self, steps: int = 1):
        """Capture `steps` consecutive generic steps in one graph (must follow at least one eager step: kernels
        loaded, workspaces allocated).  Every step reads its constants through the device-side counter, so the same
        graph is valid wherever it is replayed.
        No garbage collection runs inside the capture: a dead module that a reference cycle kept alive (a model and its trainer) gives its C
        handles back in `__del__`, and the library frees their device memory with hipFree, which is not allowed while a stream is
        capturing (and torch.cuda.graph does not collect before it begins).  The collector stays off until the capture has ended; what
        is dead waits for the next collection after it, which costs nothing here."""
        import gc
        torch.cuda.synchronize()
        was_enabled = gc.isenabled()
        gc.disable()
        try:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                for _ in range(steps):
                    self.step(-1, True)
        finally:
            if was_enabled:
                gc.enable()

    def replay(self):
        self.graph.replay()


class PointCloudDiffusion(_DiffusionBase):
    """Drop-in for reference diffusion.py:14-358 (sampling surface)."""
    _sample_dims = 2   # one sample is (N, 3)

    def __init__(self, num_points, dim=256, time_dim=256, lr=1e-4, noise_schedule="cosine", backbone="pointnet", num_classes=0,
                 p_uncond=0.1):
        """`num_classes` > 0 (not in the reference) makes the denoiser class-conditional (`UNetPointNetLarge.class_emb`, pointnet
        backbone only): the samplers take `labels` and `guidance_scale` (classifier-free guidance), and training replaces each
        label by the null class `num_classes` with probability `p_uncond`.  Both enter `hparams` only for a class model.
        `backbone` is this build's other addition to the reference signature: "pointnet" =
        UNetPointNetLarge, the denoiser diffusion.py:28 wires in; "attention" = UNetAttentionPointExperimental
        (networks.py:597-722), which the reference only reaches by editing the import at diffusion.py:11.  The
        state_dict keys are `model.*` of the chosen class either way."""
        super().__init__()
        self.hparams = _HParams(num_points=num_points, dim=dim, time_dim=time_dim, lr=lr,
                                noise_schedule=noise_schedule)
        num_classes = int(num_classes)
        if num_classes < 0 or not 0.0 <= float(p_uncond) <= 1.0:
            raise ValueError(f"num_classes must be >= 0 and p_uncond in [0, 1], got {num_classes} and {p_uncond}")
        if num_classes and backbone != "pointnet":
            raise ValueError(f"class conditioning (num_classes={num_classes}) is available for backbone 'pointnet' only, got {backbone!r}")
        if num_classes:
            self.hparams["num_classes"], self.hparams["p_uncond"] = num_classes, float(p_uncond)
        self.num_classes, self.p_uncond = num_classes, float(p_uncond)
        if backbone == "pointnet":
            self.model = UNetPointNetLarge(dim, time_dim, num_classes)
        elif backbone == "attention":
            from .networks import UNetAttentionPointExperimental
            self.model = UNetAttentionPointExperimental(num_points, dim=dim, time_dim=time_dim)
            self.hparams["backbone"] = backbone
        else:
            raise ValueError(f"backbone must be 'pointnet' or 'attention', got {backbone!r}")
        self.backbone = backbone
        self.num_points = num_points
        self.lr = lr
        self._init_schedule(noise_schedule)

    @classmethod
    def load_from_checkpoint(cls, path, map_location="cpu", weights="raw", **kwargs):
        """Lightning-free loader for the reference's `.ckpt` layout (test_point_ddpm.py:161).  `weights="ema"` loads the
        averaged weights of a run trained with an EMA decay (an error for a file without them)."""
        from .checkpoint import load_lightning_checkpoint
        hp, sd = load_lightning_checkpoint(path, map_location, weights)
        hp.update(kwargs)
        obj = cls(**{k: hp[k] for k in ("num_points", "dim", "time_dim", "lr", "noise_schedule", "backbone", "num_classes", "p_uncond")
                     if k in hp})
        obj.load_state_dict(sd, strict=True)
        return obj

    def _forward_fn(self):
        return lambda x, tb_cur, eps, stride=0: self.model.forward_with_bias(x, tb_cur, stride, out=eps)

    # ------------------------------------------------------------------ training surface (diffusion.py:56-86, 170-186)
    def configure_optimizers(self):
        """AdamW(lr, weight_decay=1e-5) + ReduceLROnPlateau(min, factor 0.5, patience 5) on `val_loss`
        (diffusion.py:60-68); the optimizer object is the HIP trainer, which also owns forward/backward."""
        from .training import AttentionTrainer, PointTrainer, ReduceLROnPlateau
        if getattr(self, "_trainer", None) is None:
            cls = AttentionTrainer if self.backbone == "attention" else PointTrainer
            self._trainer = cls(self.model, lr=self.lr, weight_decay=1e-5)
        return {"optimizer": self._trainer,
                "lr_scheduler": {"scheduler": ReduceLROnPlateau(self._trainer, factor=0.5, patience=5), "monitor": "val_loss"}}

    def diffusion_loss(self, x_0, t, noise=None, labels=None):
        """diffusion.py:170-186: L1 between the drawn noise and the prediction at x_t.  In train() mode the forward
        uses batch statistics and the parameter gradients are left in the trainer (loss and backward are one pass:
        there is no autograd graph to keep); in eval() mode it is the sampler's folded forward.  `labels`: the classes of a
        class-conditional model's batch (None = the null class)."""
        x_t, noise, _, _ = self.add_noise(x_0, t, noise)
        if self.training:
            tr = self.configure_optimizers()["optimizer"]
            if self.num_classes or labels is not None:
                tr.forward(x_t, t.to(self.device, torch.float32), labels=labels)
            else:
                tr.forward(x_t, t.to(self.device, torch.float32))
            return tr.backward(noise)
        if self.num_classes or labels is not None:
            pred = self.model(x_t, t.to(self.device, torch.float32), labels)
        else:
            pred = self.model(x_t, t.to(self.device, torch.float32))
        return self._l1_loss(pred, noise)

    def training_step(self, batch, batch_idx=0):
        """diffusion.py:70-86: t ~ U(0,1) per shape; returns the loss (gradients are ready for `optimizer.step`)."""
        x_0, labels = self._split_batch(batch)
        x_0 = x_0.to(self.device)
        t = torch.rand(x_0.shape[0], device=self.device)
        return self.diffusion_loss(x_0, t, labels=self._training_labels(labels, x_0.shape[0], True))

    def validation_step(self, batch, batch_idx=0):
        """diffusion.py:88-100 (loss part; the TensorBoard figures of :106-135 are not reproduced)."""
        x_0, labels = self._split_batch(batch)
        x_0 = x_0.to(self.device)
        t = torch.rand(x_0.shape[0], device=self.device)
        return self.diffusion_loss(x_0, t, labels=self._training_labels(labels, x_0.shape[0], False))

    def _start(self, num_samples, num_points, x_T):
        if x_T is not None and tuple(x_T.shape) != (num_samples, num_points, 3):
            raise ValueError(f"x_T must be {(num_samples, num_points, 3)}, got {tuple(x_T.shape)}")
        self.eval()
        self._require_cuda(x_T)
        if x_T is None:
            return self._randn_like(torch.empty(num_samples, num_points, 3, device=self.device))
        return x_T.to(torch.float32).contiguous().clone()

    @torch.no_grad()
    def sample(self, num_samples, num_points, num_steps=1000, x_T=None, labels=None, guidance_scale=1.0):
        """DDIM (diffusion.py:261-289).  Returns the last x_0.  `x_T` injects the start noise.  Class-conditional models:
        `labels` (B,) integers in [0, num_classes] (num_classes, or None, = unconditional) and `guidance_scale` w, a number or
        (B,) tensor: eps = eps_u + w (eps_c - eps_u) (classifier-free guidance; w = 1 costs one forward per step).  The
        arithmetic is tests/cfg_statement.py."""
        guide = self._guide(labels, guidance_scale, num_samples)
        x = self._start(num_samples, num_points, x_T)
        return self._run_table(x, self.ddim_table(num_steps, num_samples), "ddim", guide=guide)

    @torch.no_grad()
    def sample_dpm(self, num_samples, num_points, num_steps=20, order=2, spacing="logsnr", t_last=1e-3, x_T=None, labels=None,
                   guidance_scale=1.0):
        """Second-order multistep sampling of the probability-flow ODE (DPM-Solver++ 2M, not in the reference): `num_steps` network
        evaluations on a grid uniform in log-SNR from t = 1 to `t_last`.  Returns the last x_0, like `sample`, whose start draw
        it consumes.  Cosine schedule only.  `order=1, spacing="uniform"` is `sample` bit for bit.  The arithmetic is
        tests/dpm_statement.py.  `labels`, `guidance_scale`: as in `sample`."""
        guide = self._guide(labels, guidance_scale, num_samples)
        tab = self.dpm_table(num_steps, order, spacing, t_last)
        return self._run_table(self._start(num_samples, num_points, x_T), tab, "dpm", guide=guide)

    @torch.no_grad()
    def sample2(self, num_samples, num_points, num_steps=1000, x_T=None, noises=None, labels=None, guidance_scale=1.0):
        """DDPM ancestral sampling (diffusion.py:225-259).  `noises[j]` injects the j-th draw.  `labels`, `guidance_scale`: as in
        `sample`."""
        guide = self._guide(labels, guidance_scale, num_samples)
        x = self._start(num_samples, num_points, x_T)
        return self._run_table(x, self.ddpm_table(num_steps, num_samples), "ddpm", noises=noises, guide=guide)

    @torch.no_grad()
    def complete(self, partial, num_points, num_steps=1000, known_counts=None, resample=1, jump=10, x_T=None, noises=None,
                 labels=None, guidance_scale=1.0):
        """Shape completion (not in the reference): shape b keeps rows [0, known_counts[b]) of `partial` (B, M, 3), bitwise, as
        the first rows of the (B, num_points, 3) result, and the remaining rows are generated around them.  The loop is
        `sample2` on the unknown rows; after every reverse step the known rows are set to the known points noised forward to
        that step's time.  `resample` > 1 runs RePaint's schedule (cosine schedule only): each time the walk reaches an index
        in range(0, T - jump, jump) the whole cloud is noised forward `jump` indices and denoised again, `resample - 1` times
        per index, `T + jump * jumps` network evaluations in all (`completion_rows`).  `x_T` injects the start draw and
        `noises[k]` the k-th later draw in consumption order (one per row, a jump row's second right after its first).
        The arithmetic is tests/completion_statement.py.  `labels`, `guidance_scale`: as in `sample` (the known rows stay bitwise
        the given points whatever the guidance)."""
        T, r, j = int(num_steps), int(resample), int(jump)
        if partial.dim() != 3 or partial.shape[2] != 3 or partial.shape[1] > num_points:
            raise ValueError(f"partial must be (B, M <= {num_points}, 3), got {tuple(partial.shape)}")
        B, M = partial.shape[0], partial.shape[1]
        if T < 1 or r < 1:
            raise ValueError(f"num_steps and resample must be >= 1, got {num_steps} and {resample}")
        if r > 1 and (self.noise_schedule != "cosine" or not 1 <= j < T):
            raise ValueError("resample > 1 needs the cosine schedule (the forward jump relies on s^2 + n^2 = 1) and 1 <= jump < "
                             f"num_steps; got schedule {self.noise_schedule!r}, jump {jump}, num_steps {num_steps}")
        if known_counts is None:
            counts = torch.full((B,), M, dtype=torch.int32)
        else:
            counts = torch.as_tensor(known_counts)
            if counts.dim() != 1 or counts.shape[0] != B or counts.is_floating_point() or counts.is_complex() or counts.dtype == torch.bool:
                raise ValueError(f"known_counts must be a ({B},) integer tensor, got {tuple(counts.shape)} {counts.dtype}")
            if B and (int(counts.min()) < 0 or int(counts.max()) > min(M, num_points)):
                raise ValueError(f"known_counts must lie in [0, {min(M, num_points)}], got [{int(counts.min())}, {int(counts.max())}]")
        if not bool(torch.isfinite(partial).all()):
            raise ValueError("partial has non-finite coordinates")
        guide = self._guide(labels, guidance_scale, B)
        self._require_cuda(partial)
        x = self._start(B, num_points, x_T)
        p = torch.zeros_like(x)
        p[:, :M].copy_(partial)
        counts = counts.to(self.device, torch.int32).contiguous()
        tab = self.completion_table(T, j, r, B)
        _lib.check(_lib.load().pcd_complete_start(x.data_ptr(), p.data_ptr(), counts.data_ptr(), tab.n.data_ptr(), tab.s.data_ptr(),
                                                  tab.stride, x.numel(), num_points * 3, 3, _lib.stream_ptr()), "complete_start")
        return self._run_table(x, tab, "complete", noises=noises, known=(p, counts), guide=guide)

    @torch.no_grad()
    def sample3(self, num_samples, num_points, x=None, start_t=None, num_steps=1000):
        """DDIM from a given state/time (diffusion.py:291-337)."""
        return self._run_from_state(num_samples, lambda: self._start(num_samples, num_points, None), x, start_t, num_steps)


class LatentDiffusion(_DiffusionBase):
    """Drop-in for reference diffusion.py:361-734 (sampling surface) over the latents of a frozen VAE."""
    _sample_dims = 1   # one sample is (latent_dim,)
    _class_conditional = False                 # `ConditionalLatentDiffusion` is the class with classes
    _HP_KEYS = ("latent_dim", "dim", "time_dim", "lr", "noise_schedule", "is_voxel_based")

    def __init__(self, vae, latent_dim=256, dim=512, time_dim=256, lr=1e-4, noise_schedule="cosine",
                 is_voxel_based=True, num_classes=0):
        super().__init__()
        # `num_classes` is for the subclass alone: ConditionalLatentDiffusion.__init__ is the only sanctioned caller that passes it
        if num_classes and not self._class_conditional:
            raise ValueError("LatentDiffusion has no classes: class conditioning in latent space is ConditionalLatentDiffusion(vae, "
                             "num_classes=...)")
        from .networks import SimpleLatentUNetPointNet
        self.hparams = _HParams(latent_dim=latent_dim, dim=dim, time_dim=time_dim, lr=lr,
                                noise_schedule=noise_schedule, is_voxel_based=is_voxel_based)
        self.vae = vae
        for p in self.vae.parameters():
            p.requires_grad = False
        self.num_classes = int(num_classes)
        self.model = SimpleLatentUNetPointNet(latent_dim, dim, time_dim, num_classes=self.num_classes)
        self.lr = lr
        self._init_schedule(noise_schedule)
        self.init_weights()

    def init_weights(self):
        """diffusion.py:392-408, quirk included: the reference's loop skips the child NAMED 'vae' but then
        walks `self.modules()`, which contains the VAE's modules too, so every nn.Linear of the VAE (`fc_mu`,
        `fc_logvar`, `decoder_input`, and VAE3D's `encoder.5`) is re-initialised in place with kaiming-normal
        (fan_out, relu) weights and zero bias when a LatentDiffusion is constructed around it.  Conv3d / BatchNorm3d
        are not in the reference's isinstance lists and stay.  Load VAE weights AFTER constructing LatentDiffusion
        (a LatentDiffusion checkpoint carries the `vae.*` keys, so load_from_checkpoint does)."""
        import math
        sd = dict(self.vae.named_parameters())
        with torch.no_grad():
            for name, w in sd.items():
                if name.endswith(".weight") and w.dim() == 2 and name[:-6] + "bias" in sd:      # an nn.Linear
                    w.normal_(0.0, math.sqrt(2.0 / w.shape[0]))
                    sd[name[:-6] + "bias"].zero_()
        if hasattr(self.vae, "invalidate"):
            self.vae.invalidate()

    @classmethod
    def load_from_checkpoint(cls, path, vae=None, map_location="cpu", weights="raw", **kwargs):
        """`vae=` is required: the reference saves hyper-parameters with ignore=['vae'] (diffusion.py:375)."""
        from .checkpoint import load_lightning_checkpoint
        if vae is None:
            raise TypeError(f"{cls.__name__}.load_from_checkpoint needs vae=")
        hp, sd = load_lightning_checkpoint(path, map_location, weights)
        hp.update(kwargs)
        obj = cls(vae, **{k: hp[k] for k in cls._HP_KEYS if k in hp})
        obj.load_state_dict(sd, strict=True)
        return obj

    def _forward_fn(self):
        return lambda x, tb_cur, eps, stride=0: self.model.forward_with_bias(x, tb_cur, stride, out=eps)

    # The DDIM loops (`sample`, `sample3`) of a batch <= 64 run as ONE persistent launch for all their steps
    # (csrc/latent_persist.hip) when this process can have the whole GPU: 256 workgroups, one per CU, each with the whole LDS,
    # must be co-resident.  Otherwise -- larger batches, DDPM (`sample2`), PCD_LATENT_PERSISTENT=0 / use_persistent = False, a CU
    # mask, several ranks of this job on one device -- the per-layer launches run.  A persistent launch that still cannot
    # complete (a foreign process holding CUs: every wait inside is bounded) is not an error: the loop is re-run from the saved
    # start state on the per-layer launches, with one warning, and the module stays on them.  A class-conditional run
    # (`guide`) takes the same launch: labelled only up to 64 shapes, guided up to 32 (a shape's conditional and null-class rows
    # share a tile and are combined inside the launch).
    use_persistent = os.environ.get("PCD_LATENT_PERSISTENT", "1") != "0"
    GUIDED_PERSIST_MAX = 32

    def _persistent_allowed(self, x) -> bool:
        if not self.use_persistent or x.dim() != 2:
            return False
        # ranks of one job sharing a device (a one-GPU rehearsal of the multi-rank path): two persistent grids cannot be resident together.
        # Said explicitly (PCD_SHARED_GPU=1, or bench.py's PCD_BENCH_SHARE_GPU=1), or inferred when more local ranks exist than devices
        # are visible and no per-rank visibility mask is in play (with a mask every rank sees "one device" that is its own).  Whatever
        # this misses is caught by the fail-soft path below at the price of one abandoned launch (0.2 s) and a warning.
        if os.environ.get("PCD_SHARED_GPU") == "1" or os.environ.get("PCD_BENCH_SHARE_GPU") == "1":
            return False
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            masked = any(os.environ.get(k) for k in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"))
            local_world = int(os.environ.get("LOCAL_WORLD_SIZE", dist.get_world_size()))
            if not masked and local_world > max(torch.cuda.device_count(), 1):
                return False
        return self.model.persist_supported(x.shape[0])

    def _run(self, x, tab, bias_table, forward, kind, noises=None, guide=None, **kw):
        guided = guide is not None and guide[2] is not None
        if kind == "ddim" and noises is None and not (guided and x.shape[0] > self.GUIDED_PERSIST_MAX) and self._persistent_allowed(x):
            # A non-finite start state cannot go through the kernel's exchange (a value IS its own ready flag: NaN / set sign bits
            # mean "not written yet"), so such a call takes the per-layer launches, where GroupNorm keeps the damage inside its row.
            if bool(torch.isfinite(x).all()):
                start = x.clone()                                                        # <= 64 KB: the launch updates x in place
                rates = torch.stack([tab.n, tab.s, tab.a, tab.b]).contiguous()           # (4, T, R)
                counter = torch.zeros(2, dtype=torch.int32, device=x.device)
                x0 = torch.empty_like(x)
                # the last step's update of z is computed and discarded when `tab.skip_last_update` (sample3): x0 is the result
                if guide is None:
                    self.model.ddim_steps_persist(x, x0, bias_table.contiguous(), rates, counter, tab.steps)
                else:
                    self.model.ddim_steps_persist_guided(x, x0, bias_table.contiguous(), rates, counter, tab.steps, *guide)
                status = self.model.persist_status()
                if status == 0:
                    return x0
                import warnings
                warnings.warn(f"persistent latent kernel abandoned its launch (wait kind {status >> 16}, workgroup {status & 0xffff}): either "
                              "the CUs of this GPU are not all available to this process, or an intermediate value became non-finite (its "
                              "exchange reads NaN / set sign bits as 'not written yet'); re-running on the per-layer launches, which "
                              "propagate non-finite values like the reference, and staying there (LatentDiffusion.use_persistent = False)",
                              RuntimeWarning, stacklevel=3)
                self.use_persistent = False
                x.copy_(start)
        return super()._run(x, tab, bias_table, forward, kind, noises, guide=guide, **kw)

    # ------------------------------------------------------------------ training surface (diffusion.py:410-443, 522-537)
    def configure_optimizers(self, max_epochs: int = 100):
        """AdamW(lr, weight_decay=1e-5) on the denoiser (the VAE is frozen, diffusion.py:377-378) +
        CosineAnnealingLR(T_max=max_epochs, eta_min=1e-6) (diffusion.py:414-419); the optimizer is the HIP trainer."""
        from .training import CosineAnnealingLR, LatentTrainer
        if getattr(self, "_trainer", None) is None:
            self._trainer = LatentTrainer(self.model, lr=self.lr, weight_decay=1e-5)
            self._scheduler = CosineAnnealingLR(self._trainer, T_max=max_epochs, eta_min=1e-6)
        return {"optimizer": self._trainer, "lr_scheduler": self._scheduler}

    def diffusion_loss(self, z_0, t, noise=None, dropout_mask=None, labels=None):
        """diffusion.py:522-537.  train(): the denoiser runs with Dropout active and the gradients are left in the trainer.
        `labels`: the classes of a class-conditional model's batch (None = the null class)."""
        z_t, noise, _, _ = self.add_noise(z_0, t, noise)
        cond = {"labels": labels} if self.num_classes or labels is not None else {}
        if self.training:
            tr = self.configure_optimizers()["optimizer"]
            tr.forward(z_t, t.to(self.device, torch.float32), dropout_mask, **cond)
            return tr.backward(noise)
        return self._l1_loss(self.model(z_t, t.to(self.device, torch.float32), **cond), noise)

    def _latent_step(self, batch, drop: bool):
        x, labels = self._split_batch(batch)
        x = x.to(self.device)
        mu, logvar = self.vae.encode(x)
        z = self.vae.reparameterize(mu, logvar)
        t = torch.rand(z.shape[0], device=self.device)
        return self.diffusion_loss(z, t, labels=self._training_labels(labels, z.shape[0], drop))

    def training_step(self, batch, batch_idx=0):
        """diffusion.py:424-443: z = reparameterize(encode(x)) through the frozen VAE, t ~ U(0,1), L1 loss.  A class-conditional
        model takes (grids, labels) and replaces each label by the null class with probability p_uncond (one torch.rand draw after
        t's)."""
        return self._latent_step(batch, True)

    validation_step = training_step        # diffusion.py:445-467: same computation under eval() (figures not reproduced)

    def _start(self, num_samples, z_T):
        self.eval()
        self._require_cuda(z_T)
        if z_T is None:
            return self._randn_like(torch.empty(num_samples, self.hparams.latent_dim, device=self.device))
        return z_T.to(self.device, torch.float32).contiguous().clone()

    @staticmethod
    def _check_output(output):
        if output not in ("points", "mesh"):
            raise ValueError(f"output must be 'points' or 'mesh', got {output!r}")

    def _finish(self, z_0, threshold, return_latent=False, output="points"):
        from .utils import voxel_tensor_to_meshes, voxel_tensor_to_point_clouds
        x_0 = self.vae.decode(z_0)
        if self.hparams.is_voxel_based:
            convert = voxel_tensor_to_meshes if output == "mesh" else voxel_tensor_to_point_clouds
            pcs = convert(x_0, threshold=threshold)
            return (pcs, z_0) if return_latent else pcs
        # the reference's sample()/sample3() leave `point_clouds` unbound here (diffusion.py:650-653)
        raise UnboundLocalError("local variable 'point_clouds' referenced before assignment "
                                "(is_voxel_based=False is not supported by the reference's samplers either)")

    @torch.no_grad()
    def sample(self, num_samples, num_steps=1000, threshold=0.4, z_T=None, return_latent=False, output="points", labels=None,
               guidance_scale=1.0):
        """DDIM in latent space, VAE decode, voxel -> points (diffusion.py:619-653).  `output="mesh"` (here and in `sample2`, `sample3`,
        `sample_dpm`): the decoded grids leave as `utils.Mesh` surfaces of the same threshold (`utils.voxel_tensor_to_meshes`) instead.
        `labels`, `guidance_scale` (here and in the other samplers; `ConditionalLatentDiffusion` only): as in
        `PointCloudDiffusion.sample`; the arithmetic is tests/latent_cfg_statement.py."""
        self._check_output(output)
        guide = self._guide(labels, guidance_scale, num_samples)
        z = self._start(num_samples, z_T)
        return self._finish(self._run_table(z, self.ddim_table(num_steps, num_samples), "ddim", guide=guide), threshold, return_latent,
                            output)

    @torch.no_grad()
    def sample_dpm(self, num_samples, num_steps=20, order=2, spacing="logsnr", t_last=1e-3, threshold=0.4, z_T=None,
                   return_latent=False, output="points", labels=None, guidance_scale=1.0):
        """`PointCloudDiffusion.sample_dpm` in latent space, then VAE decode and voxel -> points like `sample`.  Runs on the per-layer
        launches (the persistent kernel implements the DDIM update only)."""
        self._check_output(output)
        if z_T is not None and tuple(z_T.shape) != (num_samples, self.hparams.latent_dim):
            raise ValueError(f"z_T must be {(num_samples, self.hparams.latent_dim)}, got {tuple(z_T.shape)}")
        guide = self._guide(labels, guidance_scale, num_samples)
        tab = self.dpm_table(num_steps, order, spacing, t_last)
        return self._finish(self._run_table(self._start(num_samples, z_T), tab, "dpm", guide=guide), threshold, return_latent, output)

    @torch.no_grad()
    def sample2(self, num_samples, num_steps=1000, threshold=0.4, z_T=None, noises=None, return_latent=False, output="points",
                labels=None, guidance_scale=1.0):
        """DDPM in latent space (diffusion.py:575-616)."""
        self._check_output(output)
        guide = self._guide(labels, guidance_scale, num_samples)
        z = self._start(num_samples, z_T)
        return self._finish(self._run_table(z, self.ddpm_table(num_steps, num_samples), "ddpm", noises=noises, guide=guide), threshold,
                            return_latent, output)

    @torch.no_grad()
    def sample3(self, num_samples, z=None, start_t=None, num_steps=1000, threshold=0.4, return_latent=False, output="points",
                labels=None, guidance_scale=1.0):
        """DDIM from a given latent/time (diffusion.py:655-707)."""
        self._check_output(output)
        guide = self._guide(labels, guidance_scale, num_samples)
        z0 = self._run_from_state(num_samples, lambda: self._start(num_samples, None), z, start_t, num_steps, guide=guide)
        return self._finish(z0, threshold, return_latent, output)


class ConditionalLatentDiffusion(LatentDiffusion):
    """`LatentDiffusion` over a class-conditional denoiser (not in the reference): `SimpleLatentUNetPointNet(num_classes=K)` owns
    `class_emb` (K + 1 rows, the last the null class).  The samplers take `labels` (B,) in [0, K] (K, or None, = unconditional)
    and `guidance_scale` w, a number or a (B,) tensor: eps = eps_u + w (eps_c - eps_u), one forward per step when every scale is
    exactly 1.  `sample` / `sample3` of up to 32 guided (64 labelled) shapes stay ONE persistent launch for all their steps;
    `sample2`, `sample_dpm`, larger batches and the fp32 mode run the per-layer launches, two forwards per guided step.
    Training takes (grids, labels) batches and replaces each label by the null class with probability `p_uncond`."""
    _class_conditional = True
    _HP_KEYS = LatentDiffusion._HP_KEYS + ("num_classes", "p_uncond")

    def __init__(self, vae, num_classes, p_uncond=0.1, **latent_kwargs):
        num_classes = int(num_classes)
        if num_classes < 1 or not 0.0 <= float(p_uncond) <= 1.0:
            raise ValueError(f"num_classes must be >= 1 and p_uncond in [0, 1], got {num_classes} and {p_uncond}")
        super().__init__(vae, num_classes=num_classes, **latent_kwargs)
        self.p_uncond = float(p_uncond)
        self.hparams["num_classes"], self.hparams["p_uncond"] = num_classes, self.p_uncond

    def validation_step(self, batch, batch_idx=0):
        """`training_step` under eval() with the labels as given (no drop to the null class, no draw)."""
        return self._latent_step(batch, False)
