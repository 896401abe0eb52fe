"""The float64 statement of "clip, then AdamW, with skips" that the gradient-guard tests compare against: what
`torch.nn.utils.clip_grad_norm_(params, max_norm)` followed by `torch.optim.AdamW.step()` computes on one flat tensor,
plus the rule torch's AMP path has for a non-finite gradient (`found_inf`: the step is dropped and AdamW's own step
count does not advance).  tests/test_grad_guard_cpu.py pins it against torch on the CPU."""
import math

import torch


def grad_norm(g: torch.Tensor) -> float:
    """The L2 norm of g in float64."""
    return float(torch.sqrt((g.double() ** 2).sum()))


class GuardedAdamW:
    """State (p, m1, m2, optional ema) in float64 and the counters; `step(g)` takes the unscaled gradient."""

    def __init__(self, p, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, m1=None, m2=None, ema=None,
                 ema_decay=None, t=0):
        self.p = p.detach().double().clone()
        self.m1 = torch.zeros_like(self.p) if m1 is None else m1.detach().double().clone()
        self.m2 = torch.zeros_like(self.p) if m2 is None else m2.detach().double().clone()
        self.ema = None if ema is None else ema.detach().double().clone()
        self.lr, self.betas, self.eps, self.wd, self.max_norm, self.decay = lr, betas, eps, weight_decay, max_norm, ema_decay
        self.t = t                      # AdamW's step: the applied count
        self.applied = self.skipped = self.clipped = 0
        self.norms = []

    def step(self, g: torch.Tensor, t: int = None) -> bool:
        """One guarded step; `t` overrides AdamW's step number for this update (to state what a wrong count would give)."""
        g = g.detach().double()
        if not bool(torch.isfinite(g).all()):
            self.skipped += 1
            self.norms.append(float("nan"))
            return False
        norm = grad_norm(g)
        self.norms.append(norm)
        if self.max_norm is not None and self.max_norm > 0:
            coef = self.max_norm / (norm + 1e-6)
            if coef < 1.0:
                g = g * coef
                self.clipped += 1
        self.applied += 1
        self.t = self.t + 1 if t is None else t
        b1, b2 = self.betas
        self.p = self.p * (1.0 - self.lr * self.wd)
        self.m1 = b1 * self.m1 + (1.0 - b1) * g
        self.m2 = b2 * self.m2 + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        self.p = self.p - (self.lr / bc1) * self.m1 / (torch.sqrt(self.m2) / math.sqrt(bc2) + self.eps)
        if self.ema is not None:
            self.ema = self.decay * self.ema + (1.0 - self.decay) * self.p
        return True
