"""The gradient guard's kernels on the device: norm + non-finite scan (`pcd_grad_norm_f32`), the guarded AdamW launch
(`pcd_adamw_guarded_step`) and the accumulation kernel (`pcd_grad_accumulate_f32`), against the float64 statement of
tests/grad_guard_statement.py and bitwise against the plain launches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_guard_statement as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = 1024.0
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
# 1024 blocks x 256 lanes x 4 floats is one pass of the 16-byte form: at 5_000_011 a block's loop runs five times (once
# through its four-deep unrolled body, then singly); the one-element form loops from 262_145 elements on
N_LOOP = 5_000_011


def _L():
    from shapegen_amd import _lib as L
    L.require_gpu()
    return L, L.load()


def shifted(t):
    """The same values 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    buf[1:].copy_(t)
    return buf[1:]


def place(t, shift):
    t = t.to(DEV)
    out = shifted(t) if shift else t.clone()
    assert out.data_ptr() % 16 == (4 if shift else 0)
    return out


class Guard:
    """A device state block and the two launches around it."""

    def __init__(self, max_norm=0.0, scale=SCALE):
        self.L, self.lib = _L()
        self.state = torch.zeros(16, dtype=torch.int32, device=DEV)
        self.max_norm, self.scale, self.step = max_norm, scale, 0

    def norm(self, g):
        self.step += 1
        self.L.check(self.lib.pcd_grad_norm_f32(g.data_ptr(), g.numel(), self.scale, self.max_norm, self.step, *HYPER["betas"],
                                                self.state.data_ptr(), self.L.stream_ptr()), "grad_norm")
        return self.read()

    def adamw(self, p, m1, m2, g, ema=None, decay=0.0):
        self.L.check(self.lib.pcd_adamw_guarded_step(p.data_ptr(), g.data_ptr(), m1.data_ptr(), m2.data_ptr(),
                                                     None if ema is None else ema.data_ptr(), p.numel(), HYPER["lr"], *HYPER["betas"],
                                                     HYPER["eps"], HYPER["weight_decay"], decay, self.state.data_ptr(),
                                                     self.L.stream_ptr()), "adamw_guarded")

    def read(self):
        h = self.state.cpu()
        f = h.view(torch.float32)
        return {"norm": f[0].numpy().copy(), "apply": int(h[1]), "coef": float(f[2]), "inv_scale": float(f[3]), "bc1": float(f[4]),
                "bc2": float(f[5]), "applied": int(h[6]), "skipped": int(h[7]), "clipped": int(h[8])}


def plain_adamw(p, m1, m2, g, step, scale=SCALE, ema=None, decay=0.0):
    L, lib = _L()
    hyper = (HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], step, scale)
    if ema is None:
        L.check(lib.pcd_adamw_step(p.data_ptr(), g.data_ptr(), m1.data_ptr(), m2.data_ptr(), p.numel(), *hyper, L.stream_ptr()), "adamw")
    else:
        L.check(lib.pcd_adamw_ema_step(p.data_ptr(), g.data_ptr(), m1.data_ptr(), m2.data_ptr(), ema.data_ptr(), p.numel(), *hyper, decay,
                                       L.stream_ptr()), "adamw_ema")


def ulps(a, b) -> int:
    """Distance of two positive fp32 values in units in the last place."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def want_norm(g, scale=SCALE):
    """float32(sqrt(sum(g.double() ** 2)) / scale)"""
    return np.float32(float(torch.sqrt((g.double() ** 2).sum())) / scale)


# ---------------------------------------------------------------------------------------------- 1. the norm
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 255, 1000, 1_000_003, N_LOOP])
def test_norm_within_two_ulp_and_repeatable(n, shift):
    """The device norm against float32(sqrt(sum(g.double()**2)) / scale) for randn * 1024 * 10**j: 2 ulp (squares of
    fp32 values are exact in double, a double sum of at most 2^26 terms errs by at most 2^-27 relative, one rounding to
    fp32 remains).  Two launches give the same bits."""
    gen = torch.Generator().manual_seed(n)
    for j in (-1, 0, 1):
        g = place(torch.randn(n, generator=gen) * 1024 * 10.0 ** j, shift)
        guard = Guard()
        a = guard.norm(g)
        b = guard.norm(g)
        want = want_norm(g)
        print(f"n {n} shift {shift} j {j}: device {a['norm']!r} want {want!r} ulps {ulps(a['norm'], want)}")
        assert ulps(a["norm"], want) <= 2
        assert a["norm"].tobytes() == b["norm"].tobytes()
        assert (a["apply"], b["apply"], b["applied"], b["skipped"], b["clipped"]) == (1, 1, 2, 0, 0)
        assert a["coef"] == 1.0 and a["inv_scale"] == float(np.float32(1.0) / np.float32(SCALE))


def test_values_whose_squares_overflow_fp32_are_finite():
    """1e25 squared is beyond fp32 but every element is finite: the step is not skipped and the norm is right (what the
    double accumulation buys)."""
    for n, shift in ((1000, 0), (1003, 1)):
        g = place(torch.randn(n, generator=torch.Generator().manual_seed(5)) * 1e25, shift)
        assert bool(torch.isinf(g * g).any())
        r = Guard(max_norm=1.0).norm(g)
        want = want_norm(g)
        assert r["apply"] == 1 and r["skipped"] == 0 and np.isfinite(r["norm"]) and ulps(r["norm"], want) <= 2
        assert r["clipped"] == 1 and 0.0 < r["coef"] < 1e-20


# ---------------------------------------------------------------------------------------------- 2. the scan
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 255, 1000, 1003, 300_001])
def test_scan_finds_one_nonfinite_value(n, shift):
    """One NaN, +inf or -inf at the first element, a middle one and the last one (in the n % 4 tail of the 16-byte form
    when n is no multiple of 4) drops the step; the all-finite buffer does not."""
    base = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 1024
    assert Guard().norm(place(base, shift))["apply"] == 1
    for poison in (float("nan"), float("inf"), float("-inf")):
        for pos in sorted({0, n // 2, n - 1}):
            g = place(base, shift)
            g[pos] = poison
            r = Guard(max_norm=1.0).norm(g)
            assert (r["apply"], r["applied"], r["skipped"], r["clipped"]) == (0, 0, 1, 0), (poison, pos)
            assert r["inv_scale"] == 0.0


# ---------------------------------------------------------------------------------------------- 3. armed and idle
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [1000, 1_000_003])
def test_armed_and_idle_is_the_plain_launch(n, shift):
    """Three chained steps on the inputs of test_adamw_ema_step_against_adamw_step, max_norm 0 (no clipping) and 1e30
    (never reached): parameters, both moments and the EMA are bitwise those of pcd_adamw_step / pcd_adamw_ema_step."""
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    e0 = torch.randn(n, generator=gen) * 0.5
    grads = [place(torch.randn(n, generator=gen) * 1024 * 10 ** (k - 1), shift) for k in range(3)]
    zeros = torch.zeros(n)
    new = lambda ema: tuple(place(t, shift) for t in ((p0, zeros, zeros, e0) if ema else (p0, zeros, zeros)))
    plain, plain_ema = new(False), new(True)
    runs = [(Guard(max_norm=mx), new(False), new(True)) for mx in (0.0, 1e30)]
    guards_ema = [Guard(max_norm=mx) for mx in (0.0, 1e30)]
    for k, g in enumerate(grads, start=1):
        plain_adamw(*plain, g=g, step=k)
        plain_adamw(*plain_ema[:3], g=g, step=k, ema=plain_ema[3], decay=0.999)
        for (guard, bufs, bufs_ema), guard_ema in zip(runs, guards_ema):
            r = guard.norm(g)
            assert (r["apply"], r["coef"], r["clipped"]) == (1, 1.0, 0)
            guard.adamw(*bufs, g=g)
            guard_ema.norm(g)
            guard_ema.adamw(*bufs_ema[:3], g=g, ema=bufs_ema[3], decay=0.999)
            for a, b in zip(plain, bufs):
                assert torch.equal(a, b), k
            for a, b in zip(plain_ema, bufs_ema):
                assert torch.equal(a, b), k
    assert not torch.equal(plain[0], p0.to(DEV)) and torch.equal(plain[0], plain_ema[0])


# ---------------------------------------------------------------------------------------------- 4. clipping
@pytest.mark.parametrize("shift", [0, 1])
def test_clipped_steps_match_the_statement(shift):
    """AdamW's first step does not see the gradient's scale, so: four steps with gradient magnitudes 1, 10, 0.1, 10 and a
    max_norm (3 sqrt(n); the norms are about sqrt(n) times the magnitude) that clips steps 2 and 4 only.  The parameters
    follow the statement to the 2e-6 tests/test_gpu_train.py holds pcd_adamw_step to at this lr, and are more than a
    hundred times that away from the statement without clipping."""
    n = 1003
    gen = torch.Generator().manual_seed(21)
    p0 = torch.randn(n, generator=gen)
    e0 = p0.clone()
    max_norm = 3.0 * n ** 0.5
    clipped, unclipped = S.GuardedAdamW(p0, max_norm=max_norm, ema=e0, ema_decay=0.9, **HYPER), S.GuardedAdamW(p0, **HYPER)
    guard = Guard(max_norm=max_norm)
    bufs = tuple(place(t, shift) for t in (p0, torch.zeros(n), torch.zeros(n), e0))
    for mag in (1.0, 10.0, 0.1, 10.0):
        g = torch.randn(n, generator=gen) * mag
        clipped.step(g)
        unclipped.step(g)
        gs = place(g * SCALE, shift)
        r = guard.norm(gs)
        guard.adamw(*bufs[:3], g=gs, ema=bufs[3], decay=0.9)
        assert abs(float(r["norm"]) - clipped.norms[-1]) <= 1e-6 * clipped.norms[-1]
    err = float((bufs[0].cpu().double() - clipped.p).abs().max())
    away = float((bufs[0].cpu().double() - unclipped.p).abs().max())
    print(f"clip: against the statement {err:.3e}, against the unclipped statement {away:.3e}")
    assert err <= 2e-6 and away > 100 * 2e-6
    assert float((bufs[3].cpu().double() - clipped.ema).abs().max()) <= 2e-6
    r = guard.read()
    assert (r["applied"], r["clipped"], r["skipped"]) == (4, 2, 0) == (clipped.applied, clipped.clipped, clipped.skipped)


# ---------------------------------------------------------------------------------------------- 5. skipping
@pytest.mark.parametrize("shift", [0, 1])
def test_skipped_step_changes_nothing_and_does_not_count(shift):
    """A normal step, a step whose gradient buffer holds one NaN (written by the test: a poisoned buffer), a normal step.
    The middle one leaves parameters, moments and EMA bitwise as they were; the third is AdamW's step t = 2 (2e-6 against
    the statement), not t = 3: the two differ by the factor (bc1(2) / bc1(3)) sqrt(bc2(3) / bc2(2)) = 0.859 on an update
    of up to lr = 1e-3, about 1e-4 at the largest element, so the t = 3 statement is held to be more than 4e-5 (twenty
    times the tolerance) away."""
    n = 1003
    gen = torch.Generator().manual_seed(22)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(3)]
    right = S.GuardedAdamW(p0, ema=p0, ema_decay=0.9, **HYPER)
    wrong = S.GuardedAdamW(p0, **HYPER)
    guard = Guard(max_norm=0.0)
    bufs = tuple(place(t, shift) for t in (p0, torch.zeros(n), torch.zeros(n), p0))

    def device_step(g):
        gs = place(g * SCALE, shift)
        r = guard.norm(gs)
        guard.adamw(*bufs[:3], g=gs, ema=bufs[3], decay=0.9)
        return r

    device_step(grads[0])
    right.step(grads[0]); wrong.step(grads[0])
    before = [t.clone() for t in bufs]
    bad = grads[1].clone()
    bad[n - 2] = float("nan")
    r = device_step(bad)
    assert (r["apply"], r["applied"], r["skipped"]) == (0, 1, 1)
    assert all(torch.equal(a, b) for a, b in zip(before, bufs))
    assert not right.step(bad)
    r = device_step(grads[2])
    right.step(grads[2]); wrong.step(grads[2], t=3)
    assert (r["apply"], r["applied"], r["skipped"]) == (1, 2, 1) == (1, right.applied, right.skipped)
    # 1 - beta^2 for the fp32 betas: the power is a value just below 1 rounded to fp32 (a few 2^-24), the subtraction exact
    b1, b2 = (float(np.float32(b)) for b in HYPER["betas"])
    assert abs(r["bc1"] - (1 - b1 ** 2)) < 2.0 ** -22 and abs(r["bc2"] - (1 - b2 ** 2)) < 2.0 ** -22
    err = float((bufs[0].cpu().double() - right.p).abs().max())
    away = float((bufs[0].cpu().double() - wrong.p).abs().max())
    print(f"skip: against the t = 2 statement {err:.3e}, against the t = 3 statement {away:.3e}")
    assert err <= 2e-6 and away > 4e-5
    assert float((bufs[3].cpu().double() - right.ema).abs().max()) <= 2e-6


# ---------------------------------------------------------------------------------------------- 6. accumulation
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [3, 1003, 1_000_003])
def test_accumulate_is_the_ordered_fp32_sum(n, shift):
    """k = 3: A is bitwise torch's (g1 + g2) + g3 in fp32 (whatever it held before), and the plain step on A with the
    scale S * k is bitwise pcd_adamw_step on that sum."""
    L, lib = _L()
    gen = torch.Generator().manual_seed(n)
    gs = [place(torch.randn(n, generator=gen) * SCALE, shift) for _ in range(3)]
    A = place(torch.full((n,), float("nan")), shift)
    for i, g in enumerate(gs):
        L.check(lib.pcd_grad_accumulate_f32(A.data_ptr(), g.data_ptr(), n, int(i == 0), L.stream_ptr()), "accumulate")
    want = place(((gs[0] + gs[1]) + gs[2]).cpu(), shift)
    assert torch.equal(A, want)
    p0 = torch.randn(n, generator=gen)
    a = tuple(place(t, shift) for t in (p0, torch.zeros(n), torch.zeros(n)))
    b = tuple(place(t, shift) for t in (p0, torch.zeros(n), torch.zeros(n)))
    plain_adamw(*a, g=A, step=1, scale=SCALE * 3)
    plain_adamw(*b, g=want, step=1, scale=SCALE * 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], p0.to(DEV))
