"""The float statement of `PointCloudDiffusion.complete`: shape completion from partial clouds with RePaint-style
resampling, written with the CPU oracle's schedule and broadcast helpers.  The HIP path is checked against this
(tests/test_completion_cpu.py, tests/test_gpu_completion.py); with counts = 0 and resample = 1 it is
`oracle.torch_oracle.ddpm_sample`."""
import torch

from oracle import torch_oracle as O


def completion_rows(T, jump, resample):
    """One (i, to) per network evaluation: the step from index i to i - 1, then (to is not None) the forward jump to index `to`."""
    left = {k: resample - 1 for k in range(0, T - jump, jump)} if resample > 1 else {}
    rows, i = [], T - 1
    while i > 0:
        lands = i - 1
        if left.get(lands, 0) > 0:
            left[lands] -= 1; rows.append((i, lands + jump)); i = lands + jump
        else:
            rows.append((i, None)); i = lands
    rows.append((0, None))
    return rows


def complete(model, partial, counts, x_T, T, noises, jump=1, resample=1, sched=O.offset_cosine_schedule):
    b, n_pts, _ = x_T.shape
    known = (torch.arange(n_pts)[None, :] < counts[:, None])[:, :, None]
    p = torch.zeros_like(x_T); p[:, :partial.shape[1]] = partial
    rows = completion_rows(T, jump, resample)
    n, s = sched(torch.ones(b) * rows[0][0] / T)
    x = torch.where(known, O._bc(s, x_T) * p + O._bc(n, x_T) * x_T, x_T)
    j = 0
    for i, to in rows:
        t = torch.ones(b) * i / T
        n, s = sched(t)
        eps = model(x, t)
        x0 = O.remove_noise(x, eps, n, s)
        if i == 0:
            return torch.where(known, p, x0)
        npv, sp = sched(torch.ones(b) * (i - 1) / T)
        z = noises[j]; j += 1
        unk = O._bc(sp, x) * x0 + O._bc(torch.sqrt(npv / n), x) * O._bc(n, x) * z      # sample2's update
        kn = O._bc(sp, x) * p + O._bc(npv, x) * z
        x = torch.where(known, kn, unk)
        if to is not None:
            _, sb = sched(torch.ones(b) * to / T)
            ja = sb.double() / sp.double(); jb = torch.sqrt(1 - ja * ja)                # float64, rounded to fp32 once
            z2 = noises[j]; j += 1
            x = O._bc(ja.float(), x) * x + O._bc(jb.float(), x) * z2
