"""Training step of the point denoiser on the HIP kernels.

Reference: `PointCloudDiffusion.training_step / diffusion_loss / configure_optimizers` (diffusion.py:56-86,
170-186): t ~ U(0,1) per shape, x_t = s x_0 + n eps, eps_hat = model(x_t, t) with the model in train() mode
(BatchNorm1d uses batch statistics and updates its running estimates, networks.py:31-48), loss =
F.l1_loss(eps, eps_hat), optimizer AdamW(lr, weight_decay=1e-5).

What runs where: every dense product (forward z = a W^T, backward-data da = dz W, backward-weight
dW = dz^T a) is the fp16 MFMA GEMM (`pcd_gemm_f16*`), fp32 accumulation; BatchNorm forward/backward, the
max-pool argmax/scatter, reductions, transposes, the loss and AdamW are the kernels of csrc/train.hip.  This
module is the host-side sequencing (what Lightning's `trainer.fit` + autograd do for the reference); torch is
used for buffers and for re-slicing weights.  Master weights, statistics, parameter gradients and the optimizer
state are fp32; activations and activation gradients are fp16 with a static loss scale.

Unlike the sampler there is no algebraic folding here: BatchNorm statistics depend on the batch, so every
Conv1d output is materialised, including the (B, N, 4096) `global_feat` tensor.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import contextlib

import torch

from . import _lib
from .packing import timestep_freqs
from .specs import POINT_DEC, POINT_ENC, POINT_REFINE

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def _gemm_desc(a1, k1, w, ldw, m, c, a2=None, k2=0, bias=None, shape_bias=None, rps=0, relu=0):
    """Descriptor of the fp16 MFMA GEMM z [m][c] = [a1 | a2] W^T (+ bias) for device pointers; each A block is packed
    (row stride = its width k), W has row stride ldw."""
    g = _lib.GemmDesc()
    g.a1, g.lda1, g.k1 = a1, k1, k1
    g.a2, g.lda2, g.k2 = a2, k2, k2
    g.w, g.ldw = w, ldw
    g.bias = bias
    g.shape_bias, g.rows_per_shape = shape_bias, rps
    g.relu, g.m, g.c = relu, m, c
    return g


def _flatten_parameters(model, dev):
    """Re-point every trainable `nn.Parameter` of `model` into one flat fp32 buffer (the optimizer is then a single
    launch and `state_dict()` always shows the trained weights); returns (P, G, M1, M2, views, grad views)."""
    named = [(n, q) for n, q in model.named_parameters() if q.requires_grad]
    total = sum(q.numel() for _, q in named)
    P = torch.empty(total, dtype=torch.float32, device=dev)
    G, M1, M2 = torch.zeros_like(P), torch.zeros_like(P), torch.zeros_like(P)
    views: Dict[str, torch.Tensor] = {}
    grads: Dict[str, torch.Tensor] = {}
    off = 0
    for name, prm in named:
        n = prm.numel()
        view = P[off:off + n].view(prm.shape)
        view.copy_(prm.data)
        prm.data = view
        views[name] = view
        grads[name] = G[off:off + n].view(prm.shape)
        off += n
    return P, G, M1, M2, views, grads


def _allreduce_gradients(G: torch.Tensor) -> int:
    """Data-parallel training: SUM the flat gradient buffer over the ranks (one collective per step: RCCL all-reduce over
    xGMI under the `nccl` backend; staged through the host under `gloo`, which the CPU-side tests use).  Returns the
    world size; the caller folds the 1/world of the mean into the optimizer's gradient scale."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return 1
    if dist.get_backend() == "nccl":
        dist.all_reduce(G)
    else:
        h = G.cpu()
        dist.all_reduce(h)
        G.copy_(h)
    return dist.get_world_size()


def _collective_inplace(fn, t: torch.Tensor, *args) -> None:
    """Run an in-place collective (`dist.broadcast`, `dist.all_reduce`) on a device tensor: directly under `nccl` (RCCL),
    staged through the host under `gloo`."""
    import torch.distributed as dist
    if dist.get_backend() == "nccl" or t.device.type == "cpu":
        fn(t, *args)
    else:
        h = t.cpu()
        fn(h, *args)
        t.copy_(h)


class _Trainer:
    """What every trainer shares: the module's own `nn.Parameter`s re-pointed into one flat fp32 buffer (so `state_dict()`
    always shows the trained weights and checkpoints keep the reference's keys), the workspace, the GEMM and few-row fp32
    product helpers, the time embedding of the denoisers and the AdamW step behind a torch.optim-like surface.
    Gradients are kept multiplied by `loss_scale`.  A subclass builds its layer tables after this constructor and ends
    with `refresh_weights()`, which derives whatever the kernels read from the fp32 master weights."""

    def __init__(self, model, lr: float, weight_decay: float, betas, eps: float, loss_scale: float):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.model = model
        self.lr, self.wd, self.betas, self.eps, self.loss_scale = lr, weight_decay, betas, eps, float(loss_scale)
        self.dev = model.device
        if self.dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} needs the model on an MI355X (model.to('cuda'))")
        self.step_count = 0
        self.EMA: Optional[torch.Tensor] = None    # flat fp32 moving average of P, kept by the optimizer launch (`enable_ema`)
        self.ema_decay: Optional[float] = None
        self.guard = False                         # `set_gradient_guard`: norm + non-finite scan in front of a guarded AdamW
        self.clip_norm: Optional[float] = None
        self.guard_state: Optional[torch.Tensor] = None     # the device state block of include/pcd_hip.h (16 int32 words)
        self.accum = 1                             # `set_accumulation`: micro-batches per optimizer step
        self.A: Optional[torch.Tensor] = None      # flat fp32 sum of the micro-batches' G
        self._micro = 0                            # micro-batches in A
        # ---- one flat fp32 buffer for parameters, one for gradients, two for the AdamW moments
        self.P, self.G, self.M1, self.M2, self.p, self.g = _flatten_parameters(model, self.dev)
        self.names = list(self.p)                  # the trained parameters (subclasses may add aliases to p and g)
        self.buf = dict(model.named_buffers())
        self.freqs = timestep_freqs(256)
        self._ws: Dict[str, torch.Tensor] = {}
        self.saved: Dict[str, tuple] = {}          # inputs of the few-row products, for their backward
        # load_state_dict copies into the flat buffer in place: what refresh_weights derives must follow
        model.register_load_state_dict_post_hook(lambda module, incompatible: self.refresh_weights())

    def refresh_weights(self):
        self.model.invalidate()        # the sampler's packed weights are stale now

    # ------------------------------------------------------------------ workspace
    def _st(self):
        return _lib.stream_ptr()

    def _chk(self, rc, what):
        _lib.check(rc, what)

    def _buf(self, key: str, shape, dtype=torch.float32, zero: bool = False) -> torch.Tensor:
        """The workspace tensor `key`, (re)allocated when the shape or dtype changes (zero-filled then if `zero`)."""
        t = self._ws.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.dev)
            self._ws[key] = t
        return t

    def _scratch(self, key: str, numel: int, dtype=torch.float16) -> torch.Tensor:
        """A flat scratch buffer that only ever grows (shared by the layers: transposes, slabs, ...)."""
        t = self._ws.get(key)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = torch.empty(numel, dtype=dtype, device=self.dev)
            self._ws[key] = t
        return t

    def _ones(self, n: int) -> torch.Tensor:
        """A row of n fp32 ones (the bias gradient 1^T dy of a few-row product); nothing writes it after allocation."""
        t = self._ws.get("ones")
        if t is None or t.numel() != n:
            t = self._ws["ones"] = torch.ones(1, n, dtype=torch.float32, device=self.dev)
        return t

    # ------------------------------------------------------------------ products
    def _mm(self, a, lda, ta, b, ldb, tb, m, n, k, bias, acc, c, ldc):
        self._chk(self.lib.pcd_matmul_f32(a, lda, ta, b, ldb, tb, m, n, k, bias, acc, c, ldc, self._st()), "matmul_f32")

    def _gemm(self, g, out: torch.Tensor, resid: Optional[torch.Tensor] = None):
        """out [m][c] = the product of descriptor g: fp32 for an fp32 `out`, else fp16 (+ resid, fp16 [m][c], if given)."""
        if out.dtype == torch.float32:
            self._chk(self.lib.pcd_gemm_f16_out32(C.byref(g), out.data_ptr(), g.c, self._st()), "gemm_f16_out32")
        elif resid is None:
            self._chk(self.lib.pcd_gemm_f16(C.byref(g), out.data_ptr(), g.c, self._st()), "gemm_f16")
        else:
            self._chk(self.lib.pcd_gemm_f16_residual(C.byref(g), resid.data_ptr(), g.c, out.data_ptr(), g.c, self._st()), "gemm_resid")

    def _weight_grad(self, dz: torch.Tensor, m: int, c: int, inputs, out: int, ldo: int) -> None:
        """Backward-weight product dW = dz^T [a_1 | a_2 | ...] for row-major fp16 dz [m][c] and inputs (a_i [m][k_i], k_i):
        fp32 into the device pointer `out` (row stride ldo), block i from column k_1 + ... + k_(i-1) on."""
        lib, st = self.lib, self._st()
        dzT = self._scratch("bwd.dzT", c * m)
        self._chk(lib.pcd_transpose_f16(dz.data_ptr(), m, c, dzT.data_ptr(), st), "transpose")
        for a, k in inputs:
            aT = self._scratch("bwd.aT", k * m)
            self._chk(lib.pcd_transpose_f16(a.data_ptr(), m, k, aT.data_ptr(), st), "transpose")
            g = _gemm_desc(dzT.data_ptr(), m, aT.data_ptr(), m, c, k)
            # a C x k output is a handful of tiles with an m-deep reduction: split the reduction so that one launch
            # carries >= ~512 tiles, then add the fp32 slabs in a fixed order
            tiles = -(-c // 128) * -(-k // 128)
            splits = 1
            while splits * tiles < 512 and (m // 64) % (splits * 2) == 0 and m // (splits * 2) >= 256:
                splits *= 2
            if splits == 1:
                self._chk(lib.pcd_gemm_f16_out32(C.byref(g), out, ldo, st), "gemm_dW")
            else:
                slabs = self._scratch("bwd.slabs", splits * c * k, torch.float32)
                self._chk(lib.pcd_gemm_f16_splitk(C.byref(g), splits, slabs.data_ptr(), st), "gemm_dW_splitk")
                self._chk(lib.pcd_sum_slabs_f32(slabs.data_ptr(), splits, c, k, out, ldo, st), "sum_slabs")
            out += k * 4

    def _lin(self, name: str, inputs, col0: int = 0) -> torch.Tensor:
        """y = [inputs] W^T + b as few-row fp32 products (`pcd_matmul_f32`: weights read once): an nn.Linear, whose
        torch.cat input (networks.py:1062,1074-1077) is a split product, or the per-shape part of a Conv1d(k=1), whose
        weight columns start at col0.  Returns the workspace buffer `name.y` [rows][C]."""
        w, b = self.p[name + ".weight"], self.p[name + ".bias"]
        c, ldw = w.shape[0], w.shape[1]
        rows = inputs[0][0].shape[0]
        y = self._buf(name + ".y", (rows, c), torch.float32)
        off = col0
        for i, (a, k) in enumerate(inputs):
            self._mm(a.data_ptr(), k, 0, w.data_ptr() + off * 4, ldw, 1, rows, c, k, b.data_ptr() if i == 0 else None, 1 if i else 0,
                     y.data_ptr(), c)
            off += k
        self.saved[name] = (tuple(inputs), col0)
        return y

    def _lin_backward(self, name: str, dy: torch.Tensor, targets, bias: bool = True, acc: int = 0) -> None:
        """Backward of the last `_lin(name, ...)` from dy [rows][C]: db = 1^T dy (not with `bias` False: a bias in front of
        a BatchNorm keeps its analytic zero), then per input dW = dy^T a into its column block of the weight gradient
        (added to it with `acc`) and the input gradient dy W into targets[i] = None | ('set'|'add', tensor)."""
        inputs, col0 = self.saved[name]
        w, gw = self.p[name + ".weight"], self.g[name + ".weight"]
        c, ldw = w.shape[0], w.shape[1]
        rows = dy.shape[0]
        if bias:
            self._mm(self._ones(rows).data_ptr(), rows, 0, dy.data_ptr(), c, 0, 1, c, rows, None, 0, self.g[name + ".bias"].data_ptr(), c)
        off = col0
        for (a, k), tgt in zip(inputs, targets):
            self._mm(dy.data_ptr(), c, 1, a.data_ptr(), k, 0, c, k, rows, None, acc, gw.data_ptr() + off * 4, ldw)
            if tgt is not None:
                mode, dst = tgt
                self._mm(dy.data_ptr(), c, 0, w.data_ptr() + off * 4, ldw, 0, rows, k, c, None, 1 if mode == "add" else 0,
                         dst.data_ptr(), k)
            off += k

    # ------------------------------------------------------------------ time embedding
    def _time_embedding(self, t: torch.Tensor) -> torch.Tensor:
        """time_mlp(sinusoid(t)) [B][256]: the sinusoid on the host with the reference's ops (networks.py:820-838),
        Linear -> SiLU -> Linear on the device."""
        tt = t.detach().to("cpu", torch.float32)
        e = tt[:, None] * self.freqs[None, :]
        emb = torch.cat((torch.sin(e), torch.cos(e)), dim=-1).to(self.dev)
        self.h1 = self._lin("time_mlp.0", [(emb, 256)])
        s1 = self._buf("t.s1", tuple(self.h1.shape))
        self._chk(self.lib.pcd_silu_f32(self.h1.data_ptr(), self.h1.numel(), s1.data_ptr(), self._st()), "silu")
        self.temb = self._lin("time_mlp.2", [(s1, 256)])
        return self.temb

    def _time_mlp_backward(self, dtemb: torch.Tensor) -> None:
        """time_mlp's parameter gradients from dtemb, the gradient of `_time_embedding`'s output."""
        ds = self._buf("bwd.ds", tuple(dtemb.shape))
        self._lin_backward("time_mlp.2", dtemb, [("set", ds)])
        dh = self._buf("bwd.dh", tuple(dtemb.shape))
        self._chk(self.lib.pcd_silu_backward_f32(self.h1.data_ptr(), ds.data_ptr(), ds.numel(), dh.data_ptr(), self._st()), "silu_bwd")
        self._lin_backward("time_mlp.0", dh, [None])

    # ------------------------------------------------------------------ optimizer
    def grads(self) -> Dict[str, torch.Tensor]:
        """Unscaled parameter gradients (copies), keyed like `named_parameters()`."""
        return {k: self.g[k].clone() / self.loss_scale for k in self.names}

    def enable_ema(self, decay: float) -> None:
        """Keep an exponential moving average of the trained weights: a flat fp32 buffer `EMA`, initialised to the current
        parameters, which `optimizer_step` then updates in the AdamW launch itself (`pcd_adamw_ema_step`)."""
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"ema decay must be in [0, 1), got {decay}")
        if self.EMA is None:
            self.EMA = self.P.clone()
        self.ema_decay = decay

    def set_gradient_guard(self, clip_norm: Optional[float] = None, skip_nonfinite: bool = False) -> None:
        """Arm (or, with the defaults, disarm) the guard in front of the optimizer.  Armed, every `optimizer_step` takes
        the norm of the gradient buffer on the device (`pcd_grad_norm_f32`: after the all-reduce, so it is the norm of the
        mean gradient and the same on every rank) and the AdamW launch obeys what that found without a host round trip:
        a step whose gradient holds a NaN or an infinity is dropped whole (parameters, moments and EMA untouched, AdamW's
        step not advanced), and with `clip_norm` the gradient is scaled by min(1, clip_norm / (norm + 1e-6)) as
        `torch.nn.utils.clip_grad_norm_` does.  Clipping implies skipping.  Unarmed, the step is the plain launch.
        Arming allocates the device state block and writes its counters (not for use inside a step): every step so far
        counts as applied.  Disarming folds the skipped steps out of `step_count` and drops the block, so the clipped /
        skipped history does not survive a later re-arming; changing the settings of an armed guard keeps the counters."""
        clip = None if clip_norm is None else float(clip_norm)
        if clip is not None and not clip > 0.0:
            raise ValueError(f"clip_norm must be positive, got {clip_norm}")
        armed = clip is not None or bool(skip_nonfinite)
        if armed and self.guard_state is None:
            self.guard_state = torch.zeros(16, dtype=torch.int32, device=self.dev)
            self._set_guard_counters(self.step_count, 0, 0)    # applied + skipped stays the number of steps so far
        if not armed and self.guard_state is not None:
            self.step_count -= self.guard_stats()["skipped"]   # the plain launch forms its bias corrections from step_count
            self.guard_state = None
        self.guard, self.clip_norm = armed, clip

    def _set_guard_counters(self, applied: int, skipped: int, clipped: int, last_norm: float = 0.0) -> None:
        words = torch.zeros(16, dtype=torch.int32)
        words[:1].view(torch.float32)[0] = last_norm
        words[6], words[7], words[8] = applied, skipped, clipped
        self.guard_state.copy_(words)

    def guard_stats(self) -> dict:
        """{applied, skipped, clipped, last_norm} of the guard: the one place that reads the device state block (it waits
        for the device).  Unarmed: every step so far counts as applied and last_norm is None."""
        if self.guard_state is None:
            return {"applied": self.step_count, "skipped": 0, "clipped": 0, "last_norm": None}
        h = self.guard_state.cpu()
        return {"applied": int(h[6]), "skipped": int(h[7]), "clipped": int(h[8]), "last_norm": float(h[:1].view(torch.float32)[0])}

    def set_accumulation(self, k: int) -> None:
        """Take one optimizer step per k micro-batches: `micro_step` adds each micro-batch's G into a second flat buffer A
        and steps on A at the k-th (or at `flush`), with the gradient scale loss_scale * world * k (every micro-loss
        counts 1/k, also in a partial flush)."""
        k = int(k)
        if k < 1:
            raise ValueError(f"accumulation needs k >= 1, got {k}")
        if self._micro:
            raise RuntimeError("set_accumulation with micro-batches pending: flush() first")
        self.accum = k
        if k > 1 and self.A is None:
            self.A = torch.zeros_like(self.G)
        if k == 1:
            self.A = None

    def micro_step(self) -> bool:
        """What follows every backward: the optimizer step itself without accumulation, else one more micro-batch into A
        and the optimizer step when it is the k-th.  Returns whether the optimizer stepped."""
        if self.accum == 1:
            self.optimizer_step()
            return True
        self._chk(self.lib.pcd_grad_accumulate_f32(self.A.data_ptr(), self.G.data_ptr(), self.G.numel(), int(self._micro == 0), self._st()),
                  "grad_accumulate")
        self._micro += 1
        if self._micro < self.accum:
            return False
        self.optimizer_step()
        return True

    def flush(self) -> bool:
        """The optimizer step on the micro-batches accumulated so far, if any (the end of an epoch)."""
        if self._micro == 0:
            return False
        self.optimizer_step()
        return True

    def optimizer_step(self):
        b1, b2 = self.betas
        grad, scale = self.G, self.loss_scale
        if self.accum > 1:
            if self._micro == 0:
                raise RuntimeError("optimizer_step under accumulation without a micro-batch: call micro_step() after each backward")
            grad, scale, self._micro = self.A, scale * self.accum, 0
        self.step_count += 1
        scale *= _allreduce_gradients(grad)            # data parallel: mean gradient over the ranks (BatchNorm stays per rank)
        if self.guard:
            self._chk(self.lib.pcd_grad_norm_f32(grad.data_ptr(), grad.numel(), scale, self.clip_norm or 0.0, self.step_count, b1, b2,
                                                 self.guard_state.data_ptr(), self._st()), "grad_norm")
            self._chk(self.lib.pcd_adamw_guarded_step(self.P.data_ptr(), grad.data_ptr(), self.M1.data_ptr(), self.M2.data_ptr(),
                                                      None if self.EMA is None else self.EMA.data_ptr(), self.P.numel(), self.lr,
                                                      b1, b2, self.eps, self.wd, self.ema_decay or 0.0, self.guard_state.data_ptr(),
                                                      self._st()), "adamw_guarded")
        elif self.EMA is None:
            self._chk(self.lib.pcd_adamw_step(self.P.data_ptr(), grad.data_ptr(), self.M1.data_ptr(), self.M2.data_ptr(),
                                              self.P.numel(), self.lr, b1, b2, self.eps, self.wd, self.step_count,
                                              scale, self._st()), "adamw")
        else:
            self._chk(self.lib.pcd_adamw_ema_step(self.P.data_ptr(), grad.data_ptr(), self.M1.data_ptr(), self.M2.data_ptr(),
                                                  self.EMA.data_ptr(), self.P.numel(), self.lr, b1, b2, self.eps, self.wd,
                                                  self.step_count, scale, self.ema_decay, self._st()), "adamw_ema")
        self.refresh_weights()

    # torch.optim-like aliases so the object can stand where the reference's optimizer does
    def step(self):
        self.optimizer_step()

    def zero_grad(self):
        pass                                # every backward overwrites the whole gradient buffer

    def param_layout(self) -> List[Tuple[str, int]]:
        """(name, element count) of the trained parameters in the order they lie in the flat buffers."""
        return [(k, self.p[k].numel()) for k in self.names]

    def state_dict(self):
        """Everything the optimizer carries from step to step besides the parameters themselves (those, and BatchNorm's
        running statistics, travel in the module's `state_dict()`).  The tensors are the live device buffers.  The keys
        `guard` (settings and counters of an armed gradient guard) and `accumulate` are there only when in use."""
        st = {"step": self.step_count, "lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd,
              "loss_scale": self.loss_scale, "exp_avg": self.M1, "exp_avg_sq": self.M2, "ema": self.EMA,
              "ema_decay": self.ema_decay, "layout": self.param_layout()}
        if self.guard:             # `step` counts every optimizer step, dropped ones too: AdamW's own step is guard["applied"]
            st["guard"] = {"clip_norm": self.clip_norm, **self.guard_stats()}
        if self.accum > 1:
            st["accumulate"] = self.accum
        return st

    def load_state_dict(self, state) -> None:
        """Inverse of `state_dict()`.  The parameter layout (names and sizes in flat order) must be this trainer's."""
        layout = [(str(k), int(n)) for k, n in state["layout"]]
        if layout != self.param_layout():
            mine = self.param_layout()
            bad = next((i for i, (a, b) in enumerate(zip(layout, mine)) if a != b), min(len(layout), len(mine)))
            raise RuntimeError(f"optimizer state is for another parameter layout: {len(layout)} tensors against {len(mine)} here, first "
                               f"difference at position {bad} ({layout[bad] if bad < len(layout) else None} / {mine[bad] if bad < len(mine) else None})")
        for key, dst in (("exp_avg", self.M1), ("exp_avg_sq", self.M2)):
            src = state[key]
            if src.numel() != dst.numel():
                raise RuntimeError(f"optimizer state {key} has {src.numel()} elements, the flat buffer {dst.numel()}")
            dst.copy_(src.reshape(-1).to(self.dev, torch.float32))
        self.step_count, self.lr = int(state["step"]), float(state["lr"])
        self.betas = tuple(float(b) for b in state.get("betas", self.betas))
        self.eps, self.wd = float(state.get("eps", self.eps)), float(state.get("weight_decay", self.wd))
        self.loss_scale = float(state.get("loss_scale", self.loss_scale))
        ema = state.get("ema")
        if ema is None:
            self.EMA = self.ema_decay = None
        else:
            if ema.numel() != self.P.numel():
                raise RuntimeError(f"EMA buffer has {ema.numel()} elements, the flat parameter buffer {self.P.numel()}")
            self.enable_ema(state["ema_decay"])
            self.EMA.copy_(ema.reshape(-1).to(self.dev, torch.float32))
        guard = state.get("guard")
        if guard is not None:
            self.set_gradient_guard(guard.get("clip_norm"), True)
            self._set_guard_counters(int(guard["applied"]), int(guard["skipped"]), int(guard["clipped"]), float(guard.get("last_norm") or 0.0))
        elif self.guard:           # a state without the key (an unarmed run, or a file from before the guard) into an armed trainer:
            self._set_guard_counters(self.step_count, 0, 0)    # the settings stay, and every step of that run was applied
        if state.get("accumulate") is not None:
            self._micro = 0
            self.set_accumulation(int(state["accumulate"]))
        self.refresh_weights()

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The module's `state_dict()` with every trained parameter taken from the moving average (copies); buffers
        (BatchNorm's running statistics are not averaged) as they are."""
        if self.EMA is None:
            raise RuntimeError("no EMA weights: call enable_ema(decay) before training")
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        off = 0
        for name, n in self.param_layout():
            sd[name] = self.EMA[off:off + n].view(self.p[name].shape).clone()
            off += n
        return sd

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside, the module computes with the averaged weights (they are swapped into the flat parameter buffer and
        everything the kernels read is rebuilt); the raw weights come back on exit, also after an exception."""
        if self.EMA is None:
            raise RuntimeError("no EMA weights: call enable_ema(decay) before training")
        raw = self.P.clone()
        self.P.copy_(self.EMA)
        self.refresh_weights()
        try:
            yield self
        finally:
            self.P.copy_(raw)
            self.refresh_weights()


class _Conv:
    """One Conv1d(k=1) [+ BatchNorm1d + ReLU]: names of its parameters and its saved tensors."""

    def __init__(self, conv: str, bn: Optional[str], cin: int, cout: int):
        self.conv, self.bn, self.cin, self.cout = conv, bn, cin, cout
        self.z = self.a = self.mean = self.var = None
        self.inputs: List[Tuple[torch.Tensor, int]] = []


class PointTrainer(_Trainer):
    """Forward + backward + AdamW for `UNetPointNetLarge` (networks.py:725-818)."""

    def __init__(self, model, lr: float = 1e-4, weight_decay: float = 1e-5, betas=(0.9, 0.999), eps: float = 1e-8,
                 loss_scale: float = 1024.0):
        super().__init__(model, lr, weight_decay, betas, eps, loss_scale)
        self.w16: Dict[str, torch.Tensor] = {}
        self.w16t: Dict[str, torch.Tensor] = {}
        self.debug: Optional[Dict[str, torch.Tensor]] = None    # tests set a dict: per-layer da / dz copies are kept
        self._build_layers()
        self.refresh_weights()

    def _build_layers(self):
        """The layer table in execution order."""
        self.enc = [[_Conv(f"{n}.conv{i}", f"{n}.bn{i}", a, b) for i, (a, b) in
                     enumerate([(259 if cin is None else cin, mid), (mid, mid), (mid, cout)], start=1)]
                    for n, cin, mid, cout in POINT_ENC]
        self.gf = [_Conv("global_feat.0", "global_feat.1", 1024, 2048), _Conv("global_feat.3", "global_feat.4", 2048, 4096)]
        self.dec = [[_Conv(f"{n}.conv{i}", f"{n}.bn{i}", a, b) for i, (a, b) in
                     enumerate([(cin, mid), (mid, mid), (mid, cout)], start=1)] for n, cin, mid, cout in POINT_DEC]
        self.out0 = _Conv("output.0", "output.1", 64, 64)
        self.refine = {c: _Conv(n, None, c, c) for n, c in POINT_REFINE}

    def _all_convs(self):
        for blk in self.enc:
            yield from blk
        yield from self.gf
        for blk in self.dec:
            yield from blk
        yield self.out0
        yield from self.refine.values()

    def _f16_operands(self, key: str, w2: torch.Tensor) -> None:
        """fp16 copies of the fp32 weight matrix w2 [C][K]: W for the forward product, W^T [K][C] for backward-data."""
        c, k = w2.shape
        a = self.w16.get(key)
        if a is None:
            a = self.w16[key] = torch.empty(c, k, dtype=torch.float16, device=self.dev)
            self.w16t[key] = torch.empty(k, c, dtype=torch.float16, device=self.dev)
        self._chk(self.lib.pcd_f32_to_f16(w2.data_ptr(), a.data_ptr(), a.numel(), self._st()), "f32_to_f16")
        self._chk(self.lib.pcd_transpose_f16(a.data_ptr(), c, k, self.w16t[key].data_ptr(), self._st()), "transpose")

    def refresh_weights(self):
        """fp16 operand copies of the fp32 master weights.  enc1.conv1 (K = 3 + 256) and the global half of dec4.conv1
        stay fp32."""
        for L in self._all_convs():
            w = self.p[L.conv + ".weight"]
            if L.conv == "enc1.conv1":
                self.w_xyz = w[:, :3, 0].contiguous()
                continue
            if L.conv == "dec4.conv1":
                w2 = w[:, 4096:, 0].contiguous()               # the refine4(x4) half; the 4096 global columns stay fp32
            else:
                w2 = w.view(w.shape[0], w.shape[1])
            self._f16_operands(L.conv, w2)
        self.model.invalidate()        # the sampler's packed (BN-folded) weights are stale now

    # ------------------------------------------------------------------ forward
    def _bn_relu(self, L: _Conv, z: torch.Tensor, m: int, train_stats: bool):
        lib, st = self.lib, self._st()
        c = L.cout
        L.z = z
        L.mean = self._buf(L.conv + ".mean", (c,), torch.float32)
        L.var = self._buf(L.conv + ".var", (c,), torch.float32)
        scratch = self._buf("bn.scratch", (2 * 4096,), torch.float32)
        rm = self.buf[L.bn + ".running_mean"] if train_stats else None
        rv = self.buf[L.bn + ".running_var"] if train_stats else None
        self._chk(lib.pcd_bn_batch_stats(z.data_ptr(), m, c, BN_MOMENTUM, L.mean.data_ptr(), L.var.data_ptr(),
                                         rm.data_ptr() if rm is not None else None, rv.data_ptr() if rv is not None else None,
                                         scratch.data_ptr(), st), "bn_stats")
        if train_stats:
            self.buf[L.bn + ".num_batches_tracked"] += 1
        L.a = self._buf(L.conv + ".a", (m, c), torch.float16)
        self._chk(lib.pcd_bn_apply_f16(z.data_ptr(), m, c, L.mean.data_ptr(), L.var.data_ptr(),
                                       self.p[L.bn + ".weight"].data_ptr(), self.p[L.bn + ".bias"].data_ptr(), BN_EPS, 1,
                                       L.a.data_ptr(), st), "bn_apply")
        return L.a

    def _conv(self, L: _Conv, inputs, m: int, bn: bool, update_stats: bool, shape_bias=None, rps=0):
        """z = [inputs] W^T + b, then BatchNorm(batch statistics) + ReLU if the layer has one."""
        L.inputs = inputs
        (a1, k1) = inputs[0]
        (a2, k2) = inputs[1] if len(inputs) > 1 else (None, 0)
        # conv outputs that feed a BatchNorm stay fp32 (x_hat = (z - mean) * rstd cancels); bare convs feed a GEMM: fp16
        z = self._buf(L.conv + ".z", (m, L.cout), torch.float32 if bn else torch.float16)
        wt = self.w16[L.conv]
        bias = None if shape_bias is not None else self.p[L.conv + ".bias"].data_ptr()
        self._gemm(_gemm_desc(a1.data_ptr(), k1, wt.data_ptr(), wt.shape[1], m, L.cout, a2=a2.data_ptr() if a2 is not None else None,
                              k2=k2, bias=bias, shape_bias=shape_bias, rps=rps), z)
        if not bn:
            L.z = L.a = z
            return z
        return self._bn_relu(L, z, m, update_stats)

    def _enc1(self, tbias: torch.Tensor, update_stats: bool) -> torch.Tensor:
        """enc1.conv1 on the xyz columns (K = 3, fp32) plus the per-shape bias tbias [B][64], then BatchNorm + ReLU."""
        z0 = self._buf("enc1.conv1.z", (self.m, 64), torch.float32)
        self._chk(self.lib.pcd_enc1_linear(self.x.data_ptr(), self.m, self.n, self.w_xyz.data_ptr(), 64, tbias.data_ptr(),
                                           z0.data_ptr(), self._st()), "enc1_linear")
        return self._bn_relu(self.enc[0][0], z0, self.m, update_stats)

    def forward(self, x_t: torch.Tensor, t: torch.Tensor, update_stats: bool = True, labels=None) -> torch.Tensor:
        """eps_hat (B, N, 3) fp32 with the network in train() mode; keeps what backward needs.  `labels`: the classes of a
        class-conditional model's shapes (None = the null class); their embedding rows are added to the time embedding."""
        lib, st = self.lib, self._st()
        b, n, _ = x_t.shape
        m = b * n
        if m % 64 != 0:
            raise ValueError("B*N must be a multiple of 64 (reduction length of the backward-weight GEMM)")
        self.b, self.n, self.m = b, n, m
        self.x = x_t.to(torch.float32).contiguous()
        p = self.p
        temb = self._time_embedding(t)
        self.labels = None
        if getattr(self.model, "num_classes", 0):
            # temb_b += class_emb[label_b]: in place on the buffer enc1.conv1's weight gradient reads (time_mlp.2's backward reads its input)
            self.labels = self.model.check_labels(labels, b)
            table = p["class_emb.weight"]
            self._chk(lib.pcd_embed_add_rows(temb.data_ptr(), table.data_ptr(), self.labels.data_ptr(), b, temb.shape[1], table.shape[0], st),
                      "embed_add_rows")
        elif labels is not None:
            raise ValueError("labels were given to a model without classes (num_classes=0)")
        # enc1.conv1: [xyz | temb] -> 64; the time columns give a per-shape bias
        a = self._enc1(self._lin("enc1.conv1", [(temb, 256)], col0=3), update_stats)
        skips = []
        for bi, blk in enumerate(self.enc):
            for li, L in enumerate(blk):
                if bi == 0 and li == 0:
                    continue
                a = self._conv(L, [(a, L.cin)], m, True, update_stats)
            skips.append(a)
        x1, x2, x3, x4 = skips
        a = self._conv(self.gf[0], [(x4, 1024)], m, True, update_stats)
        a = self._conv(self.gf[1], [(a, 2048)], m, True, update_stats)
        # max over the N points of each shape, with the argmax for backward (networks.py:807)
        self.gmax = self._buf("g.max", (b, 4096), torch.float32)
        self.garg = self._buf("g.arg", (b, 4096), torch.int32)
        self._chk(lib.pcd_colmax_argmax_f16(a.data_ptr(), b, n, 4096, self.gmax.data_ptr(), self.garg.data_ptr(), st), "colmax")
        # dec4.conv1 = [global (4096, constant over N) | refine4(x4) (1024)]: the global half is a per-shape bias
        self.gbias = self._lin("dec4.conv1", [(self.gmax, 4096)])
        prev = None
        for blk, xs in zip(self.dec, (x4, x3, x2, x1)):
            c = xs.shape[1]
            r = self._conv(self.refine[c], [(xs, c)], m, False, False)
            if prev is None:
                a = self._conv(blk[0], [(r, 1024)], m, True, update_stats, shape_bias=self.gbias.data_ptr(), rps=n)
            else:
                a = self._conv(blk[0], [(prev, prev.shape[1]), (r, c)], m, True, update_stats)
            a = self._conv(blk[1], [(a, blk[1].cin)], m, True, update_stats)
            prev = a = self._conv(blk[2], [(a, blk[2].cin)], m, True, update_stats)
        a = self._conv(self.out0, [(a, 64)], m, True, update_stats)
        self.pred = self._buf("pred", (b, n, 3), torch.float32)
        self.w_head = p["output.3.weight"].view(3, 64)
        self._chk(lib.pcd_head3(a.data_ptr(), m, 64, self.w_head.data_ptr(), p["output.3.bias"].data_ptr(), self.pred.data_ptr(), st),
                  "head3")
        return self.pred

    # ------------------------------------------------------------------ backward
    def _conv_backward(self, L: _Conv, dz: torch.Tensor, m: int, targets, w_cols0: int = 0):
        """Given dz (M, C): dW, db into the gradient views, and the input gradients.
        targets: per input either None (not needed), ('set', tensor) or ('add', tensor)."""
        c = L.cout
        gw = self.g[L.conv + ".weight"]
        if self.debug is not None:
            self.debug[L.conv + ".dz"] = dz.clone()
        if not L.bn:
            self._chk(self.lib.pcd_colsum_f16(dz.data_ptr(), m, 1, c, self.g[L.conv + ".bias"].data_ptr(), self._st()), "colsum")
        # (a conv bias in front of a BatchNorm: dz is mean-free per channel by construction, its column sum is exactly the
        #  analytic zero - the gradient view keeps the 0 it was allocated with; autograd leaves ~1e-9 rounding noise there)
        self._weight_grad(dz, m, c, L.inputs, gw.data_ptr() + w_cols0 * 4, gw.shape[1])
        wt = self.w16t[L.conv]
        row = 0
        for (a_in, k), tgt in zip(L.inputs, targets):
            if tgt is not None:
                mode, dst = tgt
                # da_in = dz W[:, col:col+k] : the rows [row, row+k) of W^T
                if self.debug is not None and mode == "add":
                    self.debug[f"{L.conv}.in{len(self.debug)}.before_add"] = dst.clone()
                self._gemm(_gemm_desc(dz.data_ptr(), c, wt.data_ptr() + row * c * 2, c, m, k), dst, resid=dst if mode == "add" else None)
                if self.debug is not None:
                    self.debug[f"{L.conv}.din{row}"] = dst.clone()
            row += k

    def _bn_backward(self, L: _Conv, da: torch.Tensor, m: int) -> torch.Tensor:
        """da (grad of the post-ReLU activation) -> dz in place; dgamma, dbeta into the gradient views."""
        if self.debug is not None:
            self.debug[L.conv + ".da"] = da.clone()
        self._chk(self.lib.pcd_bn_backward_f16(da.data_ptr(), L.z.data_ptr(), m, L.cout, L.mean.data_ptr(), L.var.data_ptr(),
                                               self.p[L.bn + ".weight"].data_ptr(), self.p[L.bn + ".bias"].data_ptr(), BN_EPS, 1,
                                               self.g[L.bn + ".weight"].data_ptr(), self.g[L.bn + ".bias"].data_ptr(),
                                               da.data_ptr(), self._st()), "bn_backward")
        return da

    def _chain_backward(self, layers, da: torch.Tensor, m: int, targets=None) -> torch.Tensor:
        """Backward through conv + BatchNorm + ReLU layers, given last first, from da = the gradient of the last one's
        output.  Each layer's input gradient goes to a fresh buffer that feeds the next one; the final layer's go to
        `targets` instead when given.  Returns the last fresh buffer."""
        for i, L in enumerate(layers):
            dz = self._bn_backward(L, da, m)
            if targets is not None and i == len(layers) - 1:
                self._conv_backward(L, dz, m, targets)
            else:
                da = self._buf(f"bwd.{L.conv}", (m, L.cin), torch.float16)
                self._conv_backward(L, dz, m, [("set", da)])
        return da

    def _colsum_shape(self, key: str, d: torch.Tensor) -> torch.Tensor:
        """Per-shape column sums [B][C] of d [B*N][C]: the gradient of a per-shape bias."""
        out = self._buf(key, (self.b, d.shape[1]), torch.float32)
        self._chk(self.lib.pcd_colsum_f16(d.data_ptr(), self.n, self.b, d.shape[1], out.data_ptr(), self._st()), "colsum_shape")
        return out

    def _enc1_backward(self, da: torch.Tensor) -> torch.Tensor:
        """Backward of `_enc1` from da: the xyz columns of enc1.conv1's weight gradient; returns the gradient of tbias."""
        dz0 = self._bn_backward(self.enc[0][0], da, self.m)
        tmp = self._buf("bwd.wxyzT", (3, 64), torch.float32)
        self._chk(self.lib.pcd_vec3_outer(dz0.data_ptr(), self.x.data_ptr(), self.m, 64, tmp.data_ptr(), None, self._st()), "vec3_outer")
        self.g["enc1.conv1.weight"][:, :3, 0].copy_(tmp.t())
        return self._colsum_shape("bwd.dtbias", dz0)

    def backward(self, target: torch.Tensor) -> torch.Tensor:
        """L1 loss against `target` (the noise) and all parameter gradients (scaled by loss_scale) into self.G.
        Returns the loss as a 0-d device tensor."""
        lib, st = self.lib, self._st()
        b, n, m, g = self.b, self.n, self.m, self.g
        loss_sum = self._buf("loss", (1,), torch.float32)
        dpred = self._buf("dpred", (m, 3), torch.float32)
        target = target.to(torch.float32).contiguous()
        self._chk(lib.pcd_l1_loss(self.pred.data_ptr(), target.data_ptr(), m * 3, self.loss_scale, loss_sum.data_ptr(),
                                  dpred.data_ptr(), st), "l1_loss")
        # head 64 -> 3
        a_out = self.out0.a
        self._chk(lib.pcd_vec3_outer(a_out.data_ptr(), dpred.data_ptr(), m, 64, g["output.3.weight"].data_ptr(),
                                     g["output.3.bias"].data_ptr(), st), "vec3_outer")
        da = self._buf("bwd.da0", (m, 64), torch.float16)
        self._chk(lib.pcd_vec3_expand_f16(dpred.data_ptr(), self.w_head.data_ptr(), m, 64, da.data_ptr(), st), "vec3_expand")

        def fresh(key, c):
            return self._buf(key, (m, c), torch.float16)

        da = self._chain_backward([self.out0], da, m)
        dskip: Dict[int, torch.Tensor] = {}
        # decoder, last block first
        for bi in (3, 2, 1, 0):
            blk = self.dec[bi]
            c_skip = (1024, 512, 256, 128)[bi]
            d1 = self._chain_backward(blk[:0:-1], da, m)
            dr = fresh(f"bwd.r{c_skip}", c_skip)
            if bi == 0:
                dz = self._bn_backward(blk[0], d1, m)
                # global half: per-shape sums of dz drive dW[:, :4096] and the max-pool gradient
                S = self._colsum_shape("bwd.S", dz)
                dG = self._buf("bwd.dG", (b, 4096), torch.float32)
                self._lin_backward("dec4.conv1", S, [("set", dG)], bias=False)
                self._conv_backward(blk[0], dz, m, [("set", dr)], w_cols0=4096)
            else:
                da = fresh(f"bwd.prev{bi}", blk[0].inputs[0][1])
                self._chain_backward(blk[:1], d1, m, [("set", da), ("set", dr)])
            # refine_k: bare conv on the skip tensor
            dx = fresh(f"bwd.x{c_skip}", c_skip)
            self._conv_backward(self.refine[c_skip], dr, m, [("set", dx)])
            dskip[c_skip] = dx
        # global_feat: scatter dG through the argmax, then two conv+BN+ReLU stages into dx4
        dgf = self._buf("bwd.dgf", (m, 4096), torch.float16)
        self._chk(lib.pcd_maxpool_backward_f16(dG.data_ptr(), self.garg.data_ptr(), b, n, 4096, dgf.data_ptr(), st), "maxpool_bwd")
        self._chain_backward(self.gf[::-1], dgf, m, [("add", dskip[1024])])
        # encoder: each block ends in a skip tensor whose gradient is already seeded by the decoder side
        for bi in (3, 2, 1):
            blk = self.enc[bi]
            self._chain_backward(blk[::-1], dskip[blk[2].cout], m, [("add", dskip[blk[0].cin])])
        # enc1: K = 3 + 256, all fp32 side products
        dtb = self._enc1_backward(self._chain_backward(self.enc[0][:0:-1], dskip[128], m))
        dtemb = self._buf("bwd.dtemb", (b, 256), torch.float32)
        self._lin_backward("enc1.conv1", dtb, [("set", dtemb)])
        if self.labels is not None:            # class_emb: the ordered sum of dtemb's rows per class
            gt = g["class_emb.weight"]
            self._chk(lib.pcd_embed_rows_backward(dtemb.data_ptr(), self.labels.data_ptr(), b, gt.shape[1], gt.shape[0], gt.data_ptr(), st),
                      "embed_rows_backward")
        self._time_mlp_backward(dtemb)
        return loss_sum[0] / float(m * 3)

    def train_step(self, x_t: torch.Tensor, t: torch.Tensor, noise: torch.Tensor, labels=None) -> torch.Tensor:
        self.forward(x_t, t, update_stats=True, **({} if labels is None else {"labels": labels}))
        loss = self.backward(noise)
        self.micro_step()
        return loss


class LatentTrainer(_Trainer):
    """Forward + backward + AdamW for `SimpleLatentUNetPointNet` (networks.py:963-1086) in train() mode, as used by
    `LatentDiffusion.training_step` (diffusion.py:424-443; the VAE stays frozen).  The batch is 16-32 latent vectors,
    so every product is a few-row fp32 product (`pcd_matmul_f32`: weights read once) and everything stays fp32 (no loss
    scale) - GroupNorm is per sample, so unlike the point denoiser nothing here couples the batch.  Dropout(0.1) after
    `dec1` (networks.py:1035) takes its keep mask from torch's generator, or from the caller (parity tests).  A class-conditional
    model (`num_classes` > 0) adds class_emb[label_b] to the time embedding, as `PointTrainer` does; `class_emb.weight` is the
    last entry of the flat parameter layout."""

    GROUPS = 8
    DROPOUT = 0.1

    def __init__(self, model, lr: float = 1e-4, weight_decay: float = 1e-5, betas=(0.9, 0.999), eps: float = 1e-8):
        super().__init__(model, lr, weight_decay, betas, eps, loss_scale=1.0)

    # ------------------------------------------------------------------ layer helpers
    def _gn(self, name: str, x: torch.Tensor) -> torch.Tensor:
        rows, c = x.shape
        y = self._buf(name + ".y", (rows, c), torch.float32)
        mean = self._buf(name + ".mean", (rows, self.GROUPS), torch.float32)
        rstd = self._buf(name + ".rstd", (rows, self.GROUPS), torch.float32)
        self._chk(self.lib.pcd_groupnorm_f32(x.data_ptr(), rows, c, self.GROUPS, self.p[name + ".weight"].data_ptr(),
                                             self.p[name + ".bias"].data_ptr(), 1e-5, 1, y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                             self._st()), "groupnorm")
        self.saved[name] = (x, mean, rstd)
        return y

    def _gn_backward(self, name: str, dy: torch.Tensor) -> torch.Tensor:
        x, mean, rstd = self.saved[name]
        rows, c = x.shape
        dx = self._buf(name + ".dx", (rows, c), torch.float32)
        self._chk(self.lib.pcd_groupnorm_backward_f32(dy.data_ptr(), x.data_ptr(), rows, c, self.GROUPS, self.p[name + ".weight"].data_ptr(),
                                                      self.p[name + ".bias"].data_ptr(), mean.data_ptr(), rstd.data_ptr(), 1, dx.data_ptr(),
                                                      self.g[name + ".weight"].data_ptr(), self.g[name + ".bias"].data_ptr(), self._st()),
                  "groupnorm_backward")
        return dx

    # ------------------------------------------------------------------ forward / backward
    def forward(self, z_t: torch.Tensor, t: torch.Tensor, dropout_mask: Optional[torch.Tensor] = None, labels=None) -> torch.Tensor:
        """eps_hat (B, 256) fp32 in train() mode; keeps what backward needs.  `labels`: the classes of a class-conditional
        model's shapes (None = the null class)."""
        lib, st = self.lib, self._st()
        b = z_t.shape[0]
        self.z = z_t.to(torch.float32).contiguous()
        te = self._time_embedding(t)
        self.labels = None
        if getattr(self.model, "num_classes", 0):
            # te_b += class_emb[label_b]: in place on the buffer enc1.0's weight gradient reads (time_mlp.2's backward reads its input)
            self.labels = self.model.check_labels(labels, b)
            table = self.p["class_emb.weight"]
            self._chk(lib.pcd_embed_add_rows(te.data_ptr(), table.data_ptr(), self.labels.data_ptr(), b, te.shape[1], table.shape[0], st),
                      "embed_add_rows")
        elif labels is not None:
            raise ValueError("labels were given to a model without classes (num_classes=0)")
        z1 = self._gn("enc1.1", self._lin("enc1.0", [(self.z, 256), (te, 256)]))
        z2 = self._gn("enc2.1", self._lin("enc2.0", [(z1, 128)]))
        z3 = self._gn("enc3.1", self._lin("enc3.0", [(z2, 256)]))
        z4 = self._gn("enc4.1", self._lin("enc4.0", [(z3, 512)]))
        g = self._gn("global_feat.1", self._lin("global_feat.0", [(z4, 1024)]))
        g = self._gn("global_feat.4", self._lin("global_feat.3", [(g, 2048)]))
        h = self._gn("dec4.1", self._lin("dec4.0", [(g, 4096), (self._lin("refine4", [(z4, 1024)]), 1024)]))
        h = self._gn("dec3.1", self._lin("dec3.0", [(h, 1024), (self._lin("refine3", [(z3, 512)]), 512)]))
        h = self._gn("dec2.1", self._lin("dec2.0", [(h, 512), (self._lin("refine2", [(z2, 256)]), 256)]))
        h = self._gn("dec1.1", self._lin("dec1.0", [(h, 256), (self._lin("refine1", [(z1, 128)]), 128)]))
        if dropout_mask is None:
            dropout_mask = (torch.rand(b, 128, device=self.dev) >= self.DROPOUT).to(torch.float32)
        self.mask = dropout_mask.to(self.dev, torch.float32).contiguous()
        hd = self._buf("drop.y", (b, 128), torch.float32)
        self._chk(lib.pcd_mask_scale_f32(h.data_ptr(), self.mask.data_ptr(), 1.0 / (1.0 - self.DROPOUT), h.numel(), hd.data_ptr(), st), "dropout")
        self.o0 = self._lin("output.0", [(hd, 128)])
        o0r = self._buf("o0.relu", (b, 128), torch.float32)
        self._chk(lib.pcd_relu_f32(self.o0.data_ptr(), self.o0.numel(), o0r.data_ptr(), st), "relu")
        self.pred = self._lin("output.2", [(o0r, 128)])
        return self.pred

    def backward(self, target: torch.Tensor) -> torch.Tensor:
        lib, st = self.lib, self._st()
        b = self.pred.shape[0]
        n = self.pred.numel()
        loss_sum = self._buf("loss", (1,), torch.float32)
        d = self._buf("d.pred", (b, 256), torch.float32)
        target = target.to(self.dev, torch.float32).contiguous()
        self._chk(lib.pcd_l1_loss(self.pred.data_ptr(), target.data_ptr(), n, self.loss_scale, loss_sum.data_ptr(), d.data_ptr(), st),
                  "l1_loss")

        def new(key, c):
            return self._buf("d." + key, (b, c), torch.float32)

        d_o0r = new("o0r", 128)
        self._lin_backward("output.2", d, [("set", d_o0r)])
        d_o0 = new("o0", 128)
        self._chk(lib.pcd_relu_backward_f32(self.o0.data_ptr(), d_o0r.data_ptr(), d_o0.numel(), d_o0.data_ptr(), st), "relu_bwd")
        d_hd = new("hd", 128)
        self._lin_backward("output.0", d_o0, [("set", d_hd)])
        d_h = new("h1", 128)
        self._chk(lib.pcd_mask_scale_f32(d_hd.data_ptr(), self.mask.data_ptr(), 1.0 / (1.0 - self.DROPOUT), d_hd.numel(), d_h.data_ptr(), st), "dropout_bwd")
        dz = {}
        for name, kprev, kskip, refine in (("dec1", 256, 128, "refine1"), ("dec2", 512, 256, "refine2"),
                                           ("dec3", 1024, 512, "refine3"), ("dec4", 4096, 1024, "refine4")):
            dx = self._gn_backward(name + ".1", d_h)
            d_prev, d_r = new(name + ".prev", kprev), new(name + ".r", kskip)
            self._lin_backward(name + ".0", dx, [("set", d_prev), ("set", d_r)])
            dz[kskip] = new(f"z{kskip}", kskip)
            self._lin_backward(refine, d_r, [("set", dz[kskip])])
            d_h = d_prev
        dx = self._gn_backward("global_feat.4", d_h)
        d_g0 = new("g0", 2048)
        self._lin_backward("global_feat.3", dx, [("set", d_g0)])
        dx = self._gn_backward("global_feat.1", d_g0)
        self._lin_backward("global_feat.0", dx, [("add", dz[1024])])
        for name, kin, kout in (("enc4", 512, 1024), ("enc3", 256, 512), ("enc2", 128, 256)):
            dx = self._gn_backward(name + ".1", dz[kout])
            self._lin_backward(name + ".0", dx, [("add", dz[kin])])
        dx = self._gn_backward("enc1.1", dz[128])
        d_te = new("te", 256)
        self._lin_backward("enc1.0", dx, [None, ("set", d_te)])
        if self.labels is not None:            # class_emb: the ordered sum of d_te's rows per class
            gt = self.g["class_emb.weight"]
            self._chk(lib.pcd_embed_rows_backward(d_te.data_ptr(), self.labels.data_ptr(), b, gt.shape[1], gt.shape[0], gt.data_ptr(), st),
                      "embed_rows_backward")
        self._time_mlp_backward(d_te)
        return loss_sum[0] / float(n)

    def train_step(self, z_t, t, noise, dropout_mask=None, labels=None) -> torch.Tensor:
        self.forward(z_t, t, dropout_mask, **({} if labels is None else {"labels": labels}))
        loss = self.backward(noise)
        self.micro_step()
        return loss


class _Sab:
    """One SetAttentionBlock (networks.py:51-83) in the training step: its four Linear layers and its saved tensors."""

    def __init__(self, name: str, c: int):
        self.name, self.c = name, c
        self.inp = _Conv(f"{name}.attention.in_proj", None, c, 3 * c)
        self.outp = _Conv(f"{name}.attention.out_proj", None, c, c)
        self.ff0 = _Conv(f"{name}.ff.0", None, c, 4 * c)
        self.ff2 = _Conv(f"{name}.ff.2", None, 4 * c, c)


ATTN_SABS = (("att1", 64), ("att2", 128), ("att3", 256), ("bottleneck", 256), ("att_dec3", 256), ("att_dec2", 128), ("att_dec1", 64))
ATTN_EMBS = (("emb1", 3), ("emb2", 64), ("emb3", 128), ("emb_dec3", 256), ("emb_dec2", 128), ("emb_dec1", 64))
DEC1_PAD = 64          # dec1 = PointNetLayer(128, 3) runs as 64-channel layers with zero rows (GEMM and BatchNorm widths)


class AttentionTrainer(PointTrainer):
    """Forward + backward + AdamW for `UNetAttentionPointExperimental` (networks.py:597-722) in train() mode: the
    counterpart of `PointTrainer` (whose convolution / BatchNorm helpers, optimizer step and surface it shares).
    Each SetAttentionBlock runs unfused and keeps what its backward needs: LN1 -> in_proj -> attention (+ log-sum-exp)
    -> out_proj + residual -> LN2 -> Linear + ReLU -> Linear + residual; the attention backward is the flash-style
    kernel pair of csrc/attn_bwd.hip.  `x.T + emb1(t)` in front of enc1.conv1 (K = 3) is a per-shape bias; dec1's
    3-channel layers run zero-padded to 64 channels in private buffers, their gradients and running statistics are
    copied to the real 3-channel tensors."""

    def _build_layers(self):
        model = self.model
        if model.dim != 256 or model.time_dim != 256:
            raise RuntimeError("AttentionTrainer implements the reference's configuration dim = time_dim = 256")
        self.heads = model.num_heads
        self.enc = [[_Conv(f"{n}.conv{i}", f"{n}.bn{i}", a, b) for i, (a, b) in enumerate([(cin, c), (c, c), (c, c)], start=1)]
                    for n, cin, c in (("enc1", 3, 64), ("enc2", 64, 128), ("enc3", 128, 256))]
        self.dec = [[_Conv(f"{n}.conv{i}", f"{n}.bn{i}", a, b) for i, (a, b) in enumerate([(cin, c), (c, c), (c, c)], start=1)]
                    for n, cin, c in (("dec3", 512, 128), ("dec2", 256, 64), ("dec1p", 128, DEC1_PAD))]
        self.sab = {n: _Sab(n, c) for n, c in ATTN_SABS}
        for s in self.sab.values():              # in_proj's parameters are named in_proj_weight / in_proj_bias
            for d in (self.p, self.g):
                d[s.inp.conv + ".weight"] = d[f"{s.name}.attention.in_proj_weight"]
                d[s.inp.conv + ".bias"] = d[f"{s.name}.attention.in_proj_bias"]
        # dec1 padded: parameters, gradients and running statistics in private 64-channel buffers
        for i, k in ((1, 128), (2, DEC1_PAD), (3, DEC1_PAD)):
            for d in (self.p, self.g):
                d[f"dec1p.conv{i}.weight"] = torch.zeros(DEC1_PAD, k, 1, dtype=torch.float32, device=self.dev)
                d[f"dec1p.conv{i}.bias"] = torch.zeros(DEC1_PAD, dtype=torch.float32, device=self.dev)
                d[f"dec1p.bn{i}.weight"] = torch.zeros(DEC1_PAD, dtype=torch.float32, device=self.dev)
                d[f"dec1p.bn{i}.bias"] = torch.zeros(DEC1_PAD, dtype=torch.float32, device=self.dev)
            self.buf[f"dec1p.bn{i}.running_mean"] = torch.zeros(DEC1_PAD, dtype=torch.float32, device=self.dev)
            self.buf[f"dec1p.bn{i}.running_var"] = torch.ones(DEC1_PAD, dtype=torch.float32, device=self.dev)
            self.buf[f"dec1p.bn{i}.num_batches_tracked"] = self.buf[f"dec1.bn{i}.num_batches_tracked"]
        self.w_head = torch.zeros(3, DEC1_PAD, dtype=torch.float32, device=self.dev)

    def _all_convs(self):
        for blk in self.enc:
            yield from blk[1:] if blk is self.enc[0] else blk
        for blk in self.dec:
            yield from blk
        for s in self.sab.values():
            yield from (s.inp, s.outp, s.ff0, s.ff2)

    def refresh_weights(self):
        """fp16 W / W^T operand copies of the fp32 master weights (dec1 through its zero-padded images); enc1.conv1's
        K = 3 weights stay fp32."""
        with torch.no_grad():
            for i in (1, 2, 3):
                w = self.p[f"dec1.conv{i}.weight"]
                self.p[f"dec1p.conv{i}.weight"][:3, :w.shape[1]].copy_(w)
                self.p[f"dec1p.conv{i}.bias"][:3].copy_(self.p[f"dec1.conv{i}.bias"])
                for s in ("weight", "bias"):
                    self.p[f"dec1p.bn{i}.{s}"][:3].copy_(self.p[f"dec1.bn{i}.{s}"])
            self.w_head[:, :3].copy_(self.p["output.weight"][:, :, 0])
        self.w_xyz = self.p["enc1.conv1.weight"][:, :, 0].contiguous()
        for L in self._all_convs():
            w = self.p[L.conv + ".weight"]
            self._f16_operands(L.conv, w.view(w.shape[0], w.shape[1]))
        self.model.invalidate()        # the sampler's packed (BN-folded) weights are stale now

    # ------------------------------------------------------------------ set-attention block
    def _linear(self, L: _Conv, a: torch.Tensor, out: torch.Tensor, relu: int = 0, resid: Optional[torch.Tensor] = None):
        L.inputs = [(a, L.cin)]
        self._gemm(_gemm_desc(a.data_ptr(), L.cin, self.w16[L.conv].data_ptr(), L.cin, a.shape[0], L.cout,
                              bias=self.p[L.conv + ".bias"].data_ptr(), relu=relu), out, resid)
        return out

    def sab_forward(self, name: str, x: torch.Tensor, b: int, n: int) -> torch.Tensor:
        """SetAttentionBlock `name` on x fp16 [b*n][C] (train-time, unfused); returns y fp16 [b*n][C] and keeps the
        block's saved tensors."""
        lib, st, S = self.lib, self._st(), self.sab[name]
        c, m = S.c, b * n
        f16 = torch.float16
        B = lambda key, shape, dt=f16: self._buf(f"{name}.{key}", shape, dt)
        S.b, S.n, S.x = b, n, x
        S.mu1, S.rs1, S.mu2, S.rs2 = (B(k, (m,), torch.float32) for k in ("mu1", "rs1", "mu2", "rs2"))
        S.h1 = B("h1", (m, c))
        self._chk(lib.pcd_layernorm_train_f16(x.data_ptr(), m, c, self.p[name + ".ln1.weight"].data_ptr(),
                                              self.p[name + ".ln1.bias"].data_ptr(), S.h1.data_ptr(), S.mu1.data_ptr(),
                                              S.rs1.data_ptr(), st), "layernorm_train")
        S.qkv = self._linear(S.inp, S.h1, B("qkv", (m, 3 * c)))
        S.att = B("att", (m, c))
        S.lse = B("lse", (b * self.heads * n,), torch.float32)
        self._chk(lib.pcd_set_attention_lse_f16(S.qkv.data_ptr(), b, n, c, self.heads, S.att.data_ptr(), S.lse.data_ptr(), st),
                  "set_attention_lse")
        S.y1 = self._linear(S.outp, S.att, B("y1", (m, c)), resid=x)
        S.h2 = B("h2", (m, c))
        self._chk(lib.pcd_layernorm_train_f16(S.y1.data_ptr(), m, c, self.p[name + ".ln2.weight"].data_ptr(),
                                              self.p[name + ".ln2.bias"].data_ptr(), S.h2.data_ptr(), S.mu2.data_ptr(),
                                              S.rs2.data_ptr(), st), "layernorm_train")
        S.f1 = self._linear(S.ff0, S.h2, B("f1", (m, 4 * c)), relu=1)
        return self._linear(S.ff2, S.f1, B("y", (m, c)), resid=S.y1)

    def _ln_backward(self, ln: str, dh: torch.Tensor, x: torch.Tensor, mu, rs, dx: torch.Tensor):
        m, c = x.shape
        ws = self._buf("bwd.ln_ws", (self.lib.pcd_layernorm_backward_workspace_bytes(m, c) // 4,), torch.float32)
        self._chk(self.lib.pcd_layernorm_backward_f16(dh.data_ptr(), x.data_ptr(), m, c, mu.data_ptr(), rs.data_ptr(),
                                                      self.p[ln + ".weight"].data_ptr(), 1, dx.data_ptr(),
                                                      self.g[ln + ".weight"].data_ptr(), self.g[ln + ".bias"].data_ptr(),
                                                      ws.data_ptr(), ws.numel() * 4, self._st()), "layernorm_backward")

    def sab_backward(self, name: str, dy: torch.Tensor) -> torch.Tensor:
        """Backward of the last `sab_forward(name, ...)`: dy fp16 [m][C] becomes dx in place; the block's twelve
        parameter gradients go to the gradient buffer."""
        lib, st, S = self.lib, self._st(), self.sab[name]
        c, b, n = S.c, S.b, S.n
        m = b * n
        B = lambda key, shape, dt=torch.float16: self._buf(f"bwd.sab.{key}", shape, dt)
        df1 = B(f"df1.{c}", (m, 4 * c))
        self._conv_backward(S.ff2, dy, m, [("set", df1)])
        self._chk(lib.pcd_relu_mask_f16(df1.data_ptr(), S.f1.data_ptr(), df1.numel(), df1.data_ptr(), st), "relu_mask")
        dh = B(f"dh.{c}", (m, c))
        self._conv_backward(S.ff0, df1, m, [("set", dh)])
        self._ln_backward(name + ".ln2", dh, S.y1, S.mu2, S.rs2, dy)               # dy += LN2^T dh: the first residual's gradient
        datt = B(f"datt.{c}", (m, c))
        self._conv_backward(S.outp, dy, m, [("set", datt)])
        dqkv = B(f"dqkv.{c}", (m, 3 * c))
        ws = B("attn_ws", (lib.pcd_set_attention_backward_workspace_bytes(b, n, c, self.heads) // 4,), torch.float32)
        self._chk(lib.pcd_set_attention_backward_f16(S.qkv.data_ptr(), S.att.data_ptr(), datt.data_ptr(), S.lse.data_ptr(), b, n, c,
                                                     self.heads, dqkv.data_ptr(), ws.data_ptr(), ws.numel() * 4, st), "attention_backward")
        self._conv_backward(S.inp, dqkv, m, [("set", dh)])
        self._ln_backward(name + ".ln1", dh, S.x, S.mu1, S.rs1, dy)
        return dy

    # ------------------------------------------------------------------ forward
    def _layer(self, blk, inputs, m: int, update_stats: bool) -> torch.Tensor:
        a = self._conv(blk[0], inputs, m, True, update_stats)
        a = self._conv(blk[1], [(a, blk[1].cin)], m, True, update_stats)
        return self._conv(blk[2], [(a, blk[2].cin)], m, True, update_stats)

    def _plus_emb(self, key: str, a: torch.Tensor, e: str) -> torch.Tensor:
        out = self._buf(key, tuple(a.shape), torch.float16)
        self._chk(self.lib.pcd_add_shape_bias_f16(a.data_ptr(), self.m, a.shape[1], self.n, self.E[e].data_ptr(), out.data_ptr(),
                                                  self._st()), "add_shape_bias")
        return out

    def forward(self, x_t: torch.Tensor, t: torch.Tensor, update_stats: bool = True) -> torch.Tensor:
        """eps_hat (B, N, 3) fp32 with the network in train() mode; keeps what backward needs."""
        lib, st, p = self.lib, self._st(), self.p
        b, n, _ = x_t.shape
        m = b * n
        if n % 64 != 0:
            raise ValueError("the attention backbone trains on point counts N that are multiples of 64")
        self.b, self.n, self.m = b, n, m
        self.x = x_t.to(torch.float32).contiguous()
        temb = self._time_embedding(t)
        self.E = {name: self._lin(name, [(temb, 256)]) for name, _ in ATTN_EMBS}
        for i in (1, 2, 3):                      # dec1's padded running statistics start from the real ones
            for s in ("running_mean", "running_var"):
                self.buf[f"dec1p.bn{i}.{s}"][:3].copy_(self.buf[f"dec1.bn{i}.{s}"])
        # enc1.conv1 on x + emb1(t): W (x + e) + b = W x + (W e + b), a per-shape bias
        e1 = self.enc[0]
        a = self._enc1(self._lin("enc1.conv1", [(self.E["emb1"], 3)]), update_stats)
        a = self._conv(e1[1], [(a, 64)], m, True, update_stats)
        a = self._conv(e1[2], [(a, 64)], m, True, update_stats)
        self.x1 = self._plus_emb("x1", self.sab_forward("att1", a, b, n), "emb2")
        a = self._layer(self.enc[1], [(self.x1, 64)], m, update_stats)
        self.x2 = self._plus_emb("x2", self.sab_forward("att2", a, b, n), "emb3")
        a = self._layer(self.enc[2], [(self.x2, 128)], m, update_stats)
        self.x3 = self.sab_forward("att3", a, b, n)
        h = self._plus_emb("xb", self.sab_forward("bottleneck", self.x3, b, n), "emb_dec3")
        h = self.sab_forward("att_dec3", h, b, n)
        a = self._layer(self.dec[0], [(h, 256), (self.x3, 256)], m, update_stats)
        h = self.sab_forward("att_dec2", self._plus_emb("h2", a, "emb_dec2"), b, n)
        a = self._layer(self.dec[1], [(h, 128), (self.x2, 128)], m, update_stats)
        h = self.sab_forward("att_dec1", self._plus_emb("h1", a, "emb_dec1"), b, n)
        self.a_out = self._layer(self.dec[2], [(h, 64), (self.x1, 64)], m, update_stats)
        if update_stats:
            for i in (1, 2, 3):
                for s in ("running_mean", "running_var"):
                    self.buf[f"dec1.bn{i}.{s}"].copy_(self.buf[f"dec1p.bn{i}.{s}"][:3])
        self.pred = self._buf("pred", (b, n, 3), torch.float32)
        self._chk(lib.pcd_head3(self.a_out.data_ptr(), m, DEC1_PAD, self.w_head.data_ptr(), p["output.bias"].data_ptr(),
                                self.pred.data_ptr(), st), "head3")
        return self.pred

    # ------------------------------------------------------------------ backward
    def backward(self, target: torch.Tensor) -> torch.Tensor:
        """L1 loss against `target` (the noise) and all parameter gradients (scaled by loss_scale) into self.G.
        Returns the loss as a 0-d device tensor."""
        lib, st = self.lib, self._st()
        b, m, g = self.b, self.m, self.g
        self._chk(lib.pcd_fill_zero(self.G.data_ptr(), self.G.numel() * 4, st), "fill_zero")
        loss_sum = self._buf("loss", (1,), torch.float32)
        dpred = self._buf("dpred", (m, 3), torch.float32)
        target = target.to(torch.float32).contiguous()
        self._chk(lib.pcd_l1_loss(self.pred.data_ptr(), target.data_ptr(), m * 3, self.loss_scale, loss_sum.data_ptr(),
                                  dpred.data_ptr(), st), "l1_loss")
        # output Conv1d(3, 3) on dec1's (padded) activation
        gwh = self._buf("bwd.gw_head", (3, DEC1_PAD), torch.float32)
        self._chk(lib.pcd_vec3_outer(self.a_out.data_ptr(), dpred.data_ptr(), m, DEC1_PAD, gwh.data_ptr(), g["output.bias"].data_ptr(), st),
                  "vec3_outer")
        g["output.weight"][:, :, 0].copy_(gwh[:, :3])
        da = self._buf("bwd.da_out", (m, DEC1_PAD), torch.float16)
        self._chk(lib.pcd_vec3_expand_f16(dpred.data_ptr(), self.w_head.data_ptr(), m, DEC1_PAD, da.data_ptr(), st), "vec3_expand")
        fresh = lambda key, c: self._buf(key, (m, c), torch.float16)
        dE = {}
        # decoder: dec1 <- att_dec1 <- dec2 <- att_dec2 <- dec3 <- att_dec3 <- bottleneck
        dh, dx1 = fresh("bwd.dh64", 64), fresh("bwd.dx1", 64)
        self._chain_backward(self.dec[2][::-1], da, m, [("set", dh), ("set", dx1)])
        for i, k in ((1, 128), (2, 3), (3, 3)):
            g[f"dec1.conv{i}.weight"].copy_(g[f"dec1p.conv{i}.weight"][:3, :k])
            g[f"dec1.bn{i}.weight"].copy_(g[f"dec1p.bn{i}.weight"][:3])
            g[f"dec1.bn{i}.bias"].copy_(g[f"dec1p.bn{i}.bias"][:3])
        dh = self.sab_backward("att_dec1", dh)
        dE["emb_dec1"] = self._colsum_shape("bwd.e_dec1", dh)
        dh2, dx2 = fresh("bwd.dh128", 128), fresh("bwd.dx2", 128)
        self._chain_backward(self.dec[1][::-1], dh, m, [("set", dh2), ("set", dx2)])
        dh2 = self.sab_backward("att_dec2", dh2)
        dE["emb_dec2"] = self._colsum_shape("bwd.e_dec2", dh2)
        dh3, dx3 = fresh("bwd.dh256", 256), fresh("bwd.dx3", 256)
        self._chain_backward(self.dec[0][::-1], dh2, m, [("set", dh3), ("set", dx3)])
        dh3 = self.sab_backward("att_dec3", dh3)
        dE["emb_dec3"] = self._colsum_shape("bwd.e_dec3", dh3)
        dh3 = self.sab_backward("bottleneck", dh3)
        self._chk(lib.pcd_add_relu_f16(dx3.data_ptr(), dh3.data_ptr(), dx3.numel(), 0, dx3.data_ptr(), st), "add")
        # encoder: x3 = att3(enc3(x2)), x2 = att2(enc2(x1)) + emb3, x1 = att1(enc1(x + emb1)) + emb2
        self._chain_backward(self.enc[2][::-1], self.sab_backward("att3", dx3), m, [("add", dx2)])
        dE["emb3"] = self._colsum_shape("bwd.e3", dx2)
        self._chain_backward(self.enc[1][::-1], self.sab_backward("att2", dx2), m, [("add", dx1)])
        dE["emb2"] = self._colsum_shape("bwd.e2", dx1)
        dtb = self._enc1_backward(self._chain_backward(self.enc[0][:0:-1], self.sab_backward("att1", dx1), m))
        dE["emb1"] = self._buf("bwd.e1", (b, 3), torch.float32)
        self._lin_backward("enc1.conv1", dtb, [("set", dE["emb1"])], bias=False, acc=1)
        # the six embedding Linears and time_mlp
        dtemb = self._buf("bwd.dtemb", (b, 256), torch.float32)
        for i, (name, _) in enumerate(ATTN_EMBS):
            self._lin_backward(name, dE[name], [("add" if i else "set", dtemb)])
        self._time_mlp_backward(dtemb)
        return loss_sum[0] / float(m * 3)


class CosineAnnealingLR:
    """torch.optim.lr_scheduler.CosineAnnealingLR(T_max, eta_min) in closed form (diffusion.py:415-419)."""

    def __init__(self, trainer, T_max: int, eta_min: float = 1e-6):
        self.trainer, self.T_max, self.eta_min, self.base, self.epoch = trainer, T_max, eta_min, trainer.lr, 0

    def step(self, metric=None) -> None:
        import math
        self.epoch += 1
        self.trainer.lr = self.eta_min + (self.base - self.eta_min) * (1 + math.cos(math.pi * self.epoch / self.T_max)) / 2

    def state_dict(self) -> dict:
        """torch's field names for what this object has."""
        return {"last_epoch": self.epoch, "base_lrs": [self.base], "T_max": self.T_max, "eta_min": self.eta_min,
                "_last_lr": [self.trainer.lr]}

    def load_state_dict(self, state: dict) -> None:
        self.epoch = int(state.get("last_epoch", self.epoch))
        self.base = float(state.get("base_lrs", [self.base])[0])
        self.T_max, self.eta_min = state.get("T_max", self.T_max), state.get("eta_min", self.eta_min)
        if state.get("_last_lr"):
            self.trainer.lr = float(state["_last_lr"][0])


class ReduceLROnPlateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', factor, patience) as configured at diffusion.py:61,
    restated for the trainer (threshold 1e-4 relative, cooldown 0, min_lr 0: torch's defaults)."""

    def __init__(self, trainer: PointTrainer, factor: float = 0.5, patience: int = 5, threshold: float = 1e-4):
        self.trainer, self.factor, self.patience, self.threshold = trainer, factor, patience, threshold
        self.best, self.bad = float("inf"), 0

    def step(self, metric: float) -> None:
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            self.trainer.lr *= self.factor
            self.bad = 0

    def state_dict(self) -> dict:
        """torch's field names for what this object has."""
        return {"best": self.best, "num_bad_epochs": self.bad, "factor": self.factor, "patience": self.patience,
                "threshold": self.threshold, "_last_lr": [self.trainer.lr]}

    def load_state_dict(self, state: dict) -> None:
        self.best, self.bad = float(state.get("best", self.best)), int(state.get("num_bad_epochs", self.bad))
        self.factor, self.patience = state.get("factor", self.factor), state.get("patience", self.patience)
        self.threshold = state.get("threshold", self.threshold)
        if state.get("_last_lr"):
            self.trainer.lr = float(state["_last_lr"][0])


CKPT_KEY = "shapegen_amd"      # the one private key of a checkpoint: what Lightning's layout has no place for
CKPT_FORMAT = 1
# where a module keeps its position in the on-device Philox streams: the diffusions' noise, the VAE's reparameterisation
# and prior draws (the VAE trainer's own stream position travels in its state dict)
_PHILOX_POSITIONS = ("_philox_offset", "_philox", "_philox_sample")


def adamw_state_to_torch(exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int, layout, order, lr: float, betas, eps: float,
                         weight_decay: float) -> dict:
    """The flat AdamW moments as a `torch.optim.AdamW(...).state_dict()` (what Lightning stores under `optimizer_states`).
    `layout` = (name, shape) of the trained parameters in flat order, `order` = the names of all the module's
    `parameters()`: a parameter's index is its position there, a frozen one takes an index and carries no state.
    A pure function of CPU tensors."""
    index = {name: i for i, name in enumerate(order)}
    state, off = {}, 0
    for name, shape in layout:
        n = 1
        for d in shape:
            n *= int(d)
        state[index[name]] = {"step": torch.tensor(float(step)),
                              "exp_avg": exp_avg[off:off + n].detach().to("cpu", torch.float32).reshape(tuple(shape)).clone(),
                              "exp_avg_sq": exp_avg_sq[off:off + n].detach().to("cpu", torch.float32).reshape(tuple(shape)).clone()}
        off += n
    if off != exp_avg.numel() or off != exp_avg_sq.numel():
        raise ValueError(f"layout covers {off} elements, the moments have {exp_avg.numel()} / {exp_avg_sq.numel()}")
    group = {"lr": float(lr), "betas": tuple(float(b) for b in betas), "eps": float(eps), "weight_decay": float(weight_decay),
             "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "params": list(range(len(order)))}
    return {"state": state, "param_groups": [group]}


def adamw_state_from_torch(opt_state: dict, layout, order):
    """Inverse of `adamw_state_to_torch`: (exp_avg, exp_avg_sq, step, param group) with the moments flat in `layout`'s
    order.  A trained parameter without state (it never received a gradient) reads as zeros."""
    groups = opt_state["param_groups"]
    if len(groups) != 1:
        raise RuntimeError(f"expected one optimizer param group, the file has {len(groups)}")
    ids = list(groups[0]["params"])
    if len(ids) != len(order):
        raise RuntimeError(f"optimizer state is for {len(ids)} parameters, the module has {len(order)}")
    index = {name: ids[i] for i, name in enumerate(order)}
    m1, m2, step = [], [], 0
    for name, shape in layout:
        st = opt_state["state"].get(index[name])
        if st is None:
            m1.append(torch.zeros(tuple(shape)).reshape(-1))
            m2.append(torch.zeros(tuple(shape)).reshape(-1))
            continue
        if tuple(st["exp_avg"].shape) != tuple(shape):
            raise RuntimeError(f"optimizer state of {name}: shape {tuple(st['exp_avg'].shape)}, the parameter is {tuple(shape)}")
        m1.append(st["exp_avg"].detach().to("cpu", torch.float32).reshape(-1))
        m2.append(st["exp_avg_sq"].detach().to("cpu", torch.float32).reshape(-1))
        step = max(step, int(round(float(st["step"]))))
    return torch.cat(m1), torch.cat(m2), step, dict(groups[0])


def _trainer_prefix(model, trainer) -> str:
    """The prefix of the trainer's module inside `model` ('model.' for the diffusions, '' for the VAE)."""
    for name, mod in model.named_modules():
        if mod is trainer.model:
            return name + "." if name else ""
    raise RuntimeError("the trainer's module is not part of the model being saved")


def _trainer_layout(model, trainer):
    pre = _trainer_prefix(model, trainer)
    return pre, [(pre + k, tuple(trainer.p[k].shape)) for k in trainer.names], [n for n, _ in model.named_parameters()]


def split_fingerprint(data_module) -> Optional[str]:
    """A hash of the train / validation index lists of a data module that splits with `random_split` (None otherwise)."""
    import hashlib
    tr = getattr(getattr(data_module, "train_dataset", None), "indices", None)
    va = getattr(getattr(data_module, "val_dataset", None), "indices", None)
    if tr is None or va is None:
        return None
    h = hashlib.sha256()
    for part in (tr, va):
        h.update(torch.as_tensor(list(part), dtype=torch.int64).numpy().tobytes())
        h.update(b"|")
    return h.hexdigest()


def _rng_get(device) -> dict:
    import random
    import numpy as np
    device = torch.device(device)
    return {"torch": torch.get_rng_state(), "device": torch.cuda.get_rng_state(device) if device.type == "cuda" else None,
            "python": random.getstate(), "numpy": np.random.get_state()}


def _rng_set(state: dict, device) -> None:
    import random
    import numpy as np
    device = torch.device(device)
    torch.set_rng_state(state["torch"].cpu())
    if state.get("device") is not None and device.type == "cuda":
        torch.cuda.set_rng_state(state["device"].cpu(), device)
    random.setstate(state["python"])
    np.random.set_state(state["numpy"])


def save_checkpoint(model, path: str, epoch: int, extra: Optional[dict] = None, optimizer=None, scheduler=None,
                    loop: Optional[dict] = None) -> None:
    """A `.ckpt` in the layout the reference's Lightning checkpoints have (`state_dict` + `hyper_parameters`),
    which `PointCloudDiffusion.load_from_checkpoint` of either code base reads back.  With `optimizer` / `scheduler` /
    `loop` it also carries what a run needs to continue: `global_step`, `optimizer_states` (torch.optim.AdamW's own
    layout, indexed like the module's `parameters()`), `lr_schedulers`, `ema_state_dict` and, under the private key
    `shapegen_amd`, the loss scale, EMA decay, gradient-guard settings and counters, loop state, Philox positions and RNG
    states.  `hyper_parameters` is never
    extended: the reference's loader hands it to the constructor.  The file is written to a temporary name in the same
    directory and renamed over `path`."""
    import os
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    payload = {"state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
               "hyper_parameters": dict(model.hparams), "epoch": epoch,
               "pytorch-lightning_version": "2.3.3"}       # the reference's pin; Lightning's loader looks for this key
    private = {"format": CKPT_FORMAT}
    if optimizer is not None and hasattr(optimizer, "state_dict") and hasattr(optimizer, "load_state_dict"):
        st = optimizer.state_dict()
        if isinstance(optimizer, _Trainer):
            pre, layout, order = _trainer_layout(model, optimizer)
            payload["global_step"] = int(st["step"])
            adam_step = st["guard"]["applied"] if "guard" in st else st["step"]     # torch's step: dropped steps do not count
            payload["optimizer_states"] = [adamw_state_to_torch(st["exp_avg"].cpu(), st["exp_avg_sq"].cpu(), adam_step, layout, order,
                                                                st["lr"], st["betas"], st["eps"], st["weight_decay"])]
            private["trainer"] = {k: v for k, v in st.items() if k not in ("exp_avg", "exp_avg_sq", "ema")}
            if st["ema"] is not None:
                ema = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
                trained = set(optimizer.names)
                ema.update({pre + k: v.cpu() for k, v in optimizer.ema_state_dict().items() if k in trained})
                payload["ema_state_dict"] = ema
        else:
            payload["optimizer_states"] = [st]
    if scheduler is not None and hasattr(scheduler, "state_dict") and hasattr(scheduler, "load_state_dict"):
        payload["lr_schedulers"] = [scheduler.state_dict()]
    if loop is not None:
        private.update(loop)
        payload.setdefault("global_step", int(loop.get("steps", 0)))
    if len(private) > 1:
        private["philox"] = {name: {a: int(getattr(mod, a)) for a in _PHILOX_POSITIONS if hasattr(mod, a)}
                             for name, mod in model.named_modules() if any(hasattr(mod, a) for a in _PHILOX_POSITIONS)}
        payload[CKPT_KEY] = private
    payload.update(extra or {})
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        torch.save(payload, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def restore_training_state(ckpt: dict, model, optimizer, scheduler, log=print) -> Optional[dict]:
    """Put a checkpoint dict (`checkpoint.read_checkpoint`) back into the module, the optimizer and the scheduler.  Returns
    the private part of the file, or None for a file without it (one written by Lightning): then weights, moments,
    scheduler, epoch and step are restored and `log` is told what was not."""
    model.load_state_dict(ckpt["state_dict"], strict=True)
    private = ckpt.get(CKPT_KEY)
    if private is not None and private.get("format") != CKPT_FORMAT:
        raise RuntimeError(f"checkpoint training state has format {private.get('format')}, this code reads {CKPT_FORMAT}")
    states = ckpt.get("optimizer_states") or []
    if states and hasattr(optimizer, "load_state_dict"):
        if isinstance(optimizer, _Trainer):
            pre, layout, order = _trainer_layout(model, optimizer)
            m1, m2, step, group = adamw_state_from_torch(states[0], layout, order)
            st = {"layout": optimizer.param_layout(), "exp_avg": m1, "exp_avg_sq": m2, "step": ckpt.get("global_step", step),
                  "lr": group.get("lr", optimizer.lr), "betas": group.get("betas", optimizer.betas), "eps": group.get("eps", optimizer.eps),
                  "weight_decay": group.get("weight_decay", optimizer.wd), "ema": None, "ema_decay": None}
            if private is not None and "trainer" in private:
                st.update(private["trainer"])
                if private["trainer"].get("ema_decay") is not None:
                    src = ckpt["ema_state_dict"]
                    st["ema"] = torch.cat([src[name].reshape(-1).to(torch.float32) for name, _ in layout])
            optimizer.load_state_dict(st)
        else:
            optimizer.load_state_dict(states[0])
    scheds = ckpt.get("lr_schedulers") or []
    if scheds and hasattr(scheduler, "load_state_dict"):
        scheduler.load_state_dict(scheds[0])
    if private is None:
        log("checkpoint has no 'shapegen_amd' training state (a Lightning-written file): weights, optimizer moments, scheduler, epoch "
            "and step are restored; loss scale, EMA weights, top-k list, loss history, Philox positions and RNG states are not")
        return None
    mods = dict(model.named_modules())
    for name, positions in private.get("philox", {}).items():
        for attr, off in positions.items():
            if name in mods and attr in _PHILOX_POSITIONS:
                setattr(mods[name], attr, int(off))
    return private


class _RankRng:
    """Context manager: inside, torch's CPU / device generators (and `torch.initial_seed()`, which seeds the on-device Philox
    stream) are this rank's private stream; outside, the process keeps the RNG state all ranks share."""

    def __init__(self, device, rank: int):
        self.device = torch.device(device)
        shared = self._get()
        torch.manual_seed((torch.initial_seed() + 0x9E3779B1 * (rank + 1)) & 0x7FFFFFFFFFFFFFFF)
        self.mine = self._get()
        self._set(shared)

    def _get(self):
        return torch.get_rng_state(), (torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else None)

    def _set(self, st):
        torch.set_rng_state(st[0])
        if st[1] is not None:
            torch.cuda.set_rng_state(st[1], self.device)

    def __enter__(self):
        self.shared = self._get()
        self._set(self.mine)

    def __exit__(self, *exc):
        self.mine = self._get()
        self._set(self.shared)
        return False


def fit(model, data_module, max_epochs: int = 500, ckpt_dir: Optional[str] = None, log=print, max_steps: Optional[int] = None,
        save_top_k: int = 10, ckpt_name: str = "point_cloud_diffusion", ckpt_path: Optional[str] = None, save_last: bool = False,
        ema_decay: Optional[float] = None, gradient_clip_val: Optional[float] = None, accumulate_grad_batches: int = 1,
        skip_nonfinite: bool = False):
    """What `pl.Trainer(max_epochs=...).fit(model, data_module, ckpt_path=...)` does for the reference's
    train_point_ddpm.py:78-87 and train_point_ldm.py:84-108,144: epochs of training_step + optimizer step, then
    validation_step over the validation loader in eval() mode, the model's scheduler (plateau on `val_loss` / cosine per
    epoch), and the `save_top_k` best checkpoints by val_loss (train_point_ddpm.py:60-66).

    `ckpt_path` continues a run at the epoch after the one the file was written in: module, optimizer, scheduler, loop
    state and RNG states come from the file (after `data_module.setup()` has drawn its split under the caller's seed,
    which must therefore be the first run's; a different split raises).  `save_last` also writes `<ckpt_name>-last.ckpt`
    after every epoch.  `ema_decay` turns on the trainer's moving average of the weights (a resumed run takes the decay
    from the file).  `gradient_clip_val`, `accumulate_grad_batches` and `skip_nonfinite` are Lightning's
    `pl.Trainer(gradient_clip_val=..., accumulate_grad_batches=...)` (norm clipping) and the trainer's non-finite step
    guard (`set_gradient_guard`, `set_accumulation`): an optimizer step every k usable micro-batches and once more at the
    epoch's last one, `max_steps` and `global_step` count optimizer steps.  On resume, a file that carries guard settings
    or an accumulation count (it was written by a run that used them) decides them, like the EMA decay; for a file without
    them the caller's arguments stay in force, and the guard starts with every step of the file counted as applied.
    With several ranks, rank 0 writes: its `ckpt_dir` / `save_last` decide, the other ranks may pass none
    (they only take part in gathering the per-rank random streams and histories when rank 0 saves)."""
    import inspect
    import os
    if "max_epochs" in inspect.signature(model.configure_optimizers).parameters:
        cfg = model.configure_optimizers(max_epochs=max_epochs)
    else:
        cfg = model.configure_optimizers()
    opt = cfg["optimizer"]
    sched = cfg["lr_scheduler"]["scheduler"] if isinstance(cfg["lr_scheduler"], dict) else cfg["lr_scheduler"]
    data_module.setup()
    import torch.distributed as dist
    rank, world = (dist.get_rank(), dist.get_world_size()) if (dist.is_available() and dist.is_initialized()) else (0, 1)
    if world > 1:                              # every rank starts from rank 0's parameters and BatchNorm buffers
        for t in list(model.parameters()) + list(model.buffers()):
            _collective_inplace(dist.broadcast, t.data, 0)
        if hasattr(opt, "refresh_weights"):
            opt.refresh_weights()
        for sub in model.modules():            # packed fp16 weight images (incl. a frozen VAE's handle) were built from the
            inv = getattr(sub, "invalidate", None)      # pre-broadcast values on ranks > 0: rebuild them on next use
            if callable(inv):
                inv()
    # Ranks hold different data batches and must not draw the same (t, noise, dropout) for them, but they MUST enumerate the same
    # shuffled batch sequence (`group[rank]` below deals consecutive batches of ONE permutation out to the ranks; the loaders'
    # RandomSampler seeds itself from the global torch RNG).  So the global RNG stays shared, and only the model's own draws --
    # torch.rand for t, the on-device Philox stream seeded by torch.initial_seed() -- run under a per-rank RNG state that is
    # swapped in around training_step / validation_step and swapped out again (it does not leak out of fit() either).
    if world > 1:
        # ... which only holds if every rank ENTERS with the same global RNG state: nothing upstream enforces that (a caller that seeded per rank,
        # or not at all, would make each rank shuffle differently -- an epoch would no longer partition the dataset, silently).  Rank 0's seed wins.
        seed = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF], dtype=torch.int64, device=model.device if dist.get_backend() == "nccl" else "cpu")
        _collective_inplace(dist.broadcast, seed, 0)
        torch.manual_seed(int(seed.item()))
    rank_rng = _RankRng(model.device, rank) if world > 1 else contextlib.nullcontext()
    if ema_decay is not None and hasattr(opt, "enable_ema"):
        opt.enable_ema(ema_decay)              # after the broadcast: the average starts from rank 0's weights on every rank
    if gradient_clip_val is not None or skip_nonfinite or accumulate_grad_batches != 1:
        if not isinstance(opt, _Trainer):
            raise RuntimeError("gradient_clip_val / accumulate_grad_batches / skip_nonfinite need the model's optimizer to be a HIP trainer")
        opt.set_gradient_guard(gradient_clip_val, skip_nonfinite)
        opt.set_accumulation(accumulate_grad_batches)
    micro_step = opt.micro_step if isinstance(opt, _Trainer) else (lambda: opt.step() or True)
    flush = opt.flush if isinstance(opt, _Trainer) else (lambda: False)
    kept: List[Tuple[float, str]] = []
    steps = 0
    history = []
    first_epoch = 0
    split = split_fingerprint(data_module)
    if ckpt_path is not None:
        from .checkpoint import read_checkpoint
        ckpt = read_checkpoint(ckpt_path)
        private = restore_training_state(ckpt, model, opt, sched, log)
        first_epoch = int(ckpt.get("epoch", -1)) + 1
        steps = int(ckpt.get("global_step", 0))
        if ckpt_dir is None:
            ckpt_dir = os.path.dirname(os.path.abspath(ckpt_path))
        if private is not None:
            if split is not None and private.get("split") is not None and private["split"] != split:
                raise RuntimeError(f"{ckpt_path}: the train / validation split of this data module differs from the one the checkpoint "
                                   "was trained on (seed the process as the first run did before fit()): validation samples would "
                                   "move into the training set")
            kept = [(float(v), os.path.join(ckpt_dir, name)) for v, name in private.get("kept", [])]
            steps, history = int(private.get("steps", steps)), [tuple(h) for h in private.get("history", [])]
            if private.get("rng") is not None:
                _rng_set(private["rng"], model.device)                # after setup(): the split above came from the caller's seed
            streams = private.get("rank_rng") or []
            if world > 1:
                if len(streams) == world:
                    rank_rng.mine = (streams[rank][0].cpu(), None if streams[rank][1] is None else streams[rank][1].cpu())
                    history = [tuple(h) for h in private["rank_history"][rank]]
                else:
                    rank_rng = _RankRng(model.device, rank)       # reseeded from the restored shared stream
                    log(f"resuming on {world} ranks a run saved on {max(len(streams), 1)}: the per-rank random streams are reseeded, "
                        "the continuation is not bitwise the uninterrupted run")
            elif len(streams) > 1:
                log(f"resuming on 1 rank a run saved on {len(streams)}: the continuation is not bitwise the uninterrupted run")
        if ema_decay is not None and hasattr(opt, "enable_ema") and getattr(opt, "EMA", None) is None:
            opt.enable_ema(ema_decay)
            log(f"{ckpt_path} holds no EMA weights: the average starts from the restored weights with decay {ema_decay}")
        log(f"resumed from {ckpt_path}: continuing at epoch {first_epoch}, step {steps}, lr {getattr(opt, 'lr', float('nan')):.2e}")

    saving = ckpt_dir is not None
    if world > 1:                              # rank 0 writes, so its settings decide on every rank whether the gather below runs
        flags = torch.tensor([int(saving), int(save_last)], dtype=torch.int64, device=model.device if dist.get_backend() == "nccl" else "cpu")
        _collective_inplace(dist.broadcast, flags, 0)
        saving, save_last = bool(flags[0].item()), bool(flags[1].item())

    def loop_state():
        """What the private checkpoint key records about this loop (every rank calls it: the rank streams are gathered)."""
        streams = histories = None
        if world > 1:                          # per rank: its private random stream and its own train losses
            per_rank = [None] * world
            dist.all_gather_object(per_rank, (tuple(None if t is None else t.cpu() for t in rank_rng.mine), list(history)))
            streams, histories = [r[0] for r in per_rank], [r[1] for r in per_rank]
        return {"kept": [(v, os.path.basename(p)) for v, p in kept], "steps": steps, "history": list(history), "max_epochs": max_epochs,
                "world": world, "rng": _rng_get(model.device), "rank_rng": streams, "rank_history": histories, "split": split}

    for epoch in range(first_epoch, max_epochs):
        if hasattr(model, "current_epoch"):
            model.current_epoch, model._max_epochs = epoch, max_epochs      # VAE3DLarge.get_kl_weight reads these
        model.train()
        tl = []
        group = []                             # data parallel: consecutive usable batches are dealt out `world` at a time
        for i, batch in enumerate(data_module.train_dataloader()):
            clouds = batch[0] if isinstance(batch, (tuple, list)) else batch       # a labelled batch is (clouds, labels)
            if clouds.dim() == 3 and clouds.shape[0] * clouds.shape[1] % 64:
                continue                       # ragged last point-cloud batch: the backward-weight GEMM reduces over B*N in 64s
            group.append((i, batch))
            if len(group) < world:
                continue                       # an incomplete last group is dropped: every rank takes the same number of
            i, batch = group[rank]             # steps, so each optimizer all-reduce pairs the same step on all ranks
            group = []
            with rank_rng:
                loss = model.training_step(batch, i)
            tl.append(loss)
            if not micro_step():
                continue                       # accumulating: the optimizer steps at the k-th micro-batch
            steps += 1
            if max_steps is not None and steps >= max_steps:
                break
        if flush():                            # the epoch's last micro-batches, fewer than k; validation comes after it
            steps += 1
        model.eval()
        vl = []
        for i, b in enumerate(data_module.val_dataloader()):
            with rank_rng:
                vl.append(model.validation_step(b, i))
        train_loss = float(torch.stack(tl).mean()) if tl else float("nan")
        val_loss = float(torch.stack(vl).mean()) if vl else train_loss
        if world > 1:                          # one val_loss for the scheduler and the top-k logic on every rank
            v = torch.tensor([val_loss], dtype=torch.float64, device=model.device)
            _collective_inplace(dist.all_reduce, v)
            val_loss = float(v.item()) / world
        sched.step(val_loss)
        history.append((epoch, train_loss, val_loss, opt.lr))
        line = f"epoch {epoch}: train_loss {train_loss:.4f} val_loss {val_loss:.4f} lr {opt.lr:.2e}"
        if getattr(opt, "guard", False):
            gs = opt.guard_stats()
            line += f" grad_norm {gs['last_norm']:.3e} clipped {gs['clipped']} skipped {gs['skipped']}"
        log(line)
        if saving:
            # every rank keeps the top-k list (val_loss is the same everywhere) and takes part in gathering the rank streams; rank 0 writes
            path = os.path.join(ckpt_dir or "", f"{ckpt_name}-epoch={epoch:02d}-val_loss={val_loss:.2f}.ckpt")
            enters = len(kept) < save_top_k or val_loss < max(kept)[0]
            dropped = []
            if enters:
                kept.append((val_loss, path))
                kept.sort()
                dropped, kept = [old for _, old in kept[save_top_k:] if old != path], kept[:save_top_k]
            if enters or save_last:
                state = loop_state()
                if rank == 0:
                    if enters:
                        save_checkpoint(model, path, epoch, optimizer=opt, scheduler=sched, loop=state)
                    if save_last:
                        save_checkpoint(model, os.path.join(ckpt_dir, f"{ckpt_name}-last.ckpt"), epoch, optimizer=opt, scheduler=sched,
                                        loop=state)
            if rank == 0:
                for old in dropped:
                    if os.path.exists(old):
                        os.remove(old)
        if max_steps is not None and steps >= max_steps:
            break
    return history
