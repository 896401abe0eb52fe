"""The float statement of `sample_dpm`: DPM-Solver++ 2M (second-order multistep, data-prediction form) on a grid uniform in
log-SNR, written with the CPU oracle's schedule and broadcast helpers.  The step table is formed in float64 from the fp32 rates
and rounded once; the update is torch-CPU fp32 in the kernel's operation order.  The HIP path is checked against this
(tests/test_dpm_cpu.py, tests/test_gpu_dpm.py); with order 1 and the uniform grid it is `oracle.torch_oracle.ddim_sample`."""
import math

import torch

from oracle import torch_oracle as O

MIN_SIGNAL, MAX_SIGNAL = 0.02, 0.95          # the offset cosine schedule's end points (oracle.torch_oracle.offset_cosine_schedule)


def _f32(v):
    return torch.tensor(v, dtype=torch.float64).to(torch.float32)


def grid(K, spacing="logsnr", t_last=1e-3):
    """The K network times as a (K,) fp32 tensor, and whether the last row updates the state."""
    if spacing == "uniform":                                     # `sample`: t_k = 1 - k / K
        step = 1.0 / K
        return torch.cat([torch.ones(1) - k * step for k in range(K)]), True
    a0, a1 = math.acos(MAX_SIGNAL), math.acos(MIN_SIGNAL)

    def lam(t):
        ang = a0 + t * (a1 - a0)
        return math.log(math.cos(ang) / math.sin(ang))

    l0, l1 = lam(1.0), lam(t_last)
    ts = []
    for k in range(K):
        if k == 0:
            ts.append(1.0)
        elif k == K - 1:
            ts.append(t_last)
        else:
            ts.append((math.atan(math.exp(-(l0 + (l1 - l0) * k / (K - 1)))) - a0) / (a1 - a0))
    return _f32(ts), False


def table(K, order=2, spacing="logsnr", t_last=1e-3):
    """One dict of fp32 scalars per network evaluation: t, n, s, n2, s2, c, q and `update` (False: the row only predicts x_0)."""
    t, last_updates = grid(K, spacing, t_last)
    rows, h_prev = [], None
    for k in range(K):
        n, s = O.offset_cosine_schedule(t[k:k + 1])
        update = k < K - 1 or last_updates
        if not update:
            rows.append(dict(t=t[k], n=n[0], s=s[0], n2=torch.zeros(()), s2=torch.zeros(()), c=torch.zeros(()), q=torch.zeros(()),
                             update=False))
            continue
        n2, s2 = O.offset_cosine_schedule(t[k:k + 1] - 1.0 / K) if spacing == "uniform" else O.offset_cosine_schedule(t[k + 1:k + 2])
        nk, sk, n2k, s2k = float(n[0]), float(s[0]), float(n2[0]), float(s2[0])       # fp32 rates promoted to float64
        h = math.log(s2k / n2k) - math.log(sk / nk)
        c = h / (2.0 * h_prev) if (order == 2 and k > 0) else 0.0
        h_prev = h
        rows.append(dict(t=t[k], n=n[0], s=s[0], n2=n2[0], s2=s2[0], c=_f32(c), q=_f32(sk / nk), update=True))
    return rows


def update(x, eps, hist, n, s, n2, s2, c, q):
    """One step in the kernel's operation order; the rates are (R,) tensors, R = 1 or the batch.  -> (x0, x_next).
    c = 0 reads no history (it may hold anything) and is the DDIM update."""
    ne = O._bc(n, x) * eps
    x0 = (x - ne) / O._bc(s, x)
    w = O._bc(c, x) * (x0 - hist)
    use = O._bc(c != 0, x)
    D = torch.where(use, x0 + w, x0)
    qw = O._bc(q, x) * w
    eD = torch.where(use, eps - qw, eps)
    a = O._bc(s2, x) * D
    cc = O._bc(n2, x) * eD
    return x0, a + cc


def sample_dpm(model, x_T, K, order=2, spacing="logsnr", t_last=1e-3):
    """Returns the last x_0."""
    b = x_T.shape[0]
    x, hist = x_T, torch.full_like(x_T, float("nan"))
    for r in table(K, order, spacing, t_last):
        eps = model(x, r["t"].expand(b))
        one = lambda v: v.reshape(1)
        x0, xn = update(x, eps, hist, *(one(r[k]) for k in ("n", "s", "n2", "s2", "c", "q")))
        hist = x0
        if r["update"]:
            x = xn
    return hist
