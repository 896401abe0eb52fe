"""The per-step statement of the samplers' step tables: the literal transcription of the reference's loops -- `sample2`
(diffusion.py:241-255), `sample` (:277-286), `sample3` (:323-335) -- and of `complete`'s walk (tests/completion_statement.py),
one schedule call per step on the (width,) vector the reference forms there, written with the CPU oracle's schedule functions.
`ddim_table`, `ddpm_table`, `from_state_table` and `completion_table` of `shapegen_amd.diffusion` form the same numbers for all
steps at once as (T, width) matrices and are checked against these bit for bit (tests/test_abi_cpu.py,
tests/test_completion_cpu.py).  Each function returns the table's fields: t (T,), the rest (T, width)."""
import torch

from completion_statement import completion_rows
from oracle import torch_oracle as O


def _table(**cols):
    out = {f: torch.stack([v.reshape(-1) for v in rows]) for f, rows in cols.items()}
    out["t"] = out["t"][:, 0]
    return out


def ddim(T, width, sched=O.offset_cosine_schedule):
    ts, ns, ss, n2, s2 = [], [], [], [], []
    step = 1.0 / T
    for k in range(T):
        t = torch.ones(width) - k * step
        n, s = sched(t)
        nn_, sn = sched(t - step)
        ts.append(t); ns.append(n); ss.append(s); n2.append(nn_); s2.append(sn)
    return _table(t=ts, n=ns, s=ss, a=n2, b=s2)


def ddpm(T, width, sched=O.offset_cosine_schedule):
    ts, ns, ss, co, s2 = [], [], [], [], []
    for i in reversed(range(T)):
        t = torch.ones(width) * i / T
        n, s = sched(t)
        ts.append(t); ns.append(n); ss.append(s)
        if i > 0:
            npv, sp = sched(torch.ones(width) * (i - 1) / T)
            co.append(torch.sqrt(npv / n)); s2.append(sp)
        else:                                                       # x_t = x_0, no update
            co.append(torch.zeros(width)); s2.append(torch.zeros(width))
    return _table(t=ts, n=ns, s=ss, a=co, b=s2)


def from_state(start_t0, T, sched=O.offset_cosine_schedule):
    """Only start_t[0] is used and the schedule sees a 0-d t: width 1 for both schedules."""
    steps = torch.linspace(torch.as_tensor(start_t0, dtype=torch.float32), torch.zeros(1)[0], T)
    ts, ns, ss, n2, s2 = [], [], [], [], []
    for i in range(T):
        n, s = sched(steps[i])
        ts.append(steps[i]); ns.append(n); ss.append(s)
        if i < T - 1:
            nn_, sn = sched(steps[i + 1])
            n2.append(nn_); s2.append(sn)
        else:
            n2.append(torch.zeros(())); s2.append(torch.zeros(()))
    return _table(t=ts, n=ns, s=ss, a=n2, b=s2)


def completion(T, jump, resample, width, sched=O.offset_cosine_schedule):
    """The scalars `completion_statement.complete` forms at each row of its walk; zeros where a row has no update or no jump."""
    ts, ns, ss, co, s2, n2, jas, jbs = [], [], [], [], [], [], [], []
    for i, to in completion_rows(T, jump, resample):
        t = torch.ones(width) * i / T
        n, s = sched(t)
        ts.append(t); ns.append(n); ss.append(s)
        ja, jb = torch.zeros(width), torch.zeros(width)
        if i > 0:
            npv, sp = sched(torch.ones(width) * (i - 1) / T)
            co.append(torch.sqrt(npv / n)); s2.append(sp); n2.append(npv)
            if to is not None:
                _, sb = sched(torch.ones(width) * to / T)
                ja = sb.double() / sp.double()
                jb = torch.sqrt(1 - ja * ja).float()
                ja = ja.float()
        else:
            co.append(torch.zeros(width)); s2.append(torch.zeros(width)); n2.append(torch.zeros(width))
        jas.append(ja); jbs.append(jb)
    return _table(t=ts, n=ns, s=ss, a=co, b=s2, n2=n2, ja=jas, jb=jbs)
