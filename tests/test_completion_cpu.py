"""Shape completion, the parts that need no GPU: the RePaint walk, the float statement against the DDPM oracle, the step
table `complete` uploads, the C ABI of the new kernels and the argument checks of `PointCloudDiffusion.complete`."""
import os
import re

import pytest
import torch

import completion_statement as S
from oracle import torch_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pcd_step_select_cols", "pcd_complete_start", "pcd_complete_update", "pcd_complete_update_philox")


def _toy(x, t):
    """A set function like the denoisers: pointwise terms plus a per-shape max."""
    return torch.tanh(x * 1.7 + t[:, None, None]) * 0.8 + 0.1 * x.max(dim=1, keepdim=True).values


def _unit_clouds(b, m, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(b, m, 3, generator=g)
    return c / c.norm(dim=2).max(dim=1).values[:, None, None]


def _n_draws(rows):
    return sum(1 if to is None else 2 for _, to in rows[:-1])


@pytest.mark.parametrize("T,jump,resample,want", [(20, 5, 3, 50), (16, 4, 2, 28), (1000, 10, 10, 9910), (12, 4, 2, 20),
                                                  (12, 4, 1, 12), (1, 1, 1, 1)])
def test_row_counts_and_index_range(T, jump, resample, want):
    from shapegen_amd.diffusion import completion_rows
    rows = S.completion_rows(T, jump, resample)
    assert rows == completion_rows(T, jump, resample)
    jumps = sum(to is not None for _, to in rows)
    assert len(rows) == want == T + jump * jumps
    assert rows[0][0] == T - 1 and rows[-1] == (0, None)
    assert all(0 <= i <= T - 1 and (to is None or i - 1 + jump == to <= T - 1) for i, to in rows)
    for (i, to), (nxt, _) in zip(rows, rows[1:]):                     # a walk: each row starts where the last one ended
        assert nxt == (i - 1 if to is None else to)
    if resample > 1:                                                  # every jump index is left resample - 1 times by a jump
        for k in range(0, T - jump, jump):
            assert sum(1 for i, to in rows if to is not None and i - 1 == k) == resample - 1


def test_statement_without_known_rows_is_the_ddpm_oracle():
    g = torch.Generator().manual_seed(5)
    B, N, T = 3, 128, 12
    x_T = torch.randn(B, N, 3, generator=g)
    noises = [torch.randn(B, N, 3, generator=g) for _ in range(T - 1)]
    got = S.complete(_toy, _unit_clouds(B, 50, 1), torch.zeros(B, dtype=torch.int64), x_T, T, noises)
    assert torch.equal(got, O.ddpm_sample(_toy, x_T, T, noises))


@pytest.mark.parametrize("jump,resample", [(1, 1), (4, 2)])
def test_statement_returns_known_rows_bitwise(jump, resample):
    g = torch.Generator().manual_seed(6)
    B, N, T = 3, 128, 12
    counts = torch.tensor([0, 37, 128])
    partial = _unit_clouds(B, N, 2)
    x_T = torch.randn(B, N, 3, generator=g)
    noises = [torch.randn(B, N, 3, generator=g) for _ in range(_n_draws(S.completion_rows(T, jump, resample)))]
    out = S.complete(_toy, partial, counts, x_T, T, noises, jump, resample)
    assert torch.isfinite(out).all()
    for b, c in enumerate(counts.tolist()):
        assert torch.equal(out[b, :c], partial[b, :c])
    assert torch.equal(out[2], partial[2])
    assert not torch.equal(out[1, 37:], partial[1, 37:])


@pytest.mark.parametrize("T,jump,resample", [(12, 4, 2), (20, 5, 3), (7, 1, 1)])
def test_completion_table_holds_the_statements_scalars(T, jump, resample):
    """Every column of the uploaded table is, bit for bit, the scalar the statement forms at that row."""
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=8)
    tab = m.completion_table(T, jump, resample, batch=3)
    rows = S.completion_rows(T, jump, resample)
    assert tab.steps == len(rows) and tab.width == 1 and tab.stride == 0 and tab.rows == rows
    assert tab.jumps == (resample > 1) and len(tab.columns()) == 7
    j = 0
    for k, (i, to) in enumerate(rows):
        assert tab.draws[k] == j
        n, s = O.offset_cosine_schedule(torch.ones(3) * i / T)
        assert tab.t[k] == (torch.ones(3) * i / T)[0] and tab.n[k, 0] == n[0] and tab.s[k, 0] == s[0]
        if i == 0:
            assert [float(c[k, 0]) for c in tab.columns()[2:]] == [0.0] * 5
            continue
        npv, sp = O.offset_cosine_schedule(torch.ones(3) * (i - 1) / T)
        assert tab.a[k, 0] == torch.sqrt(npv / n)[0] and tab.b[k, 0] == sp[0] and tab.n2[k, 0] == npv[0]
        j += 1
        if to is None:
            assert tab.ja[k, 0] == 0 and tab.jb[k, 0] == 0
        else:
            _, sb = O.offset_cosine_schedule(torch.ones(3) * to / T)
            ja = sb.double() / sp.double()
            assert tab.ja[k, 0] == ja.float()[0] and tab.jb[k, 0] == torch.sqrt(1 - ja * ja).float()[0]
            assert 0 < float(tab.ja[k, 0]) < 1
            j += 1


def test_completion_table_linear_schedule_has_batch_width():
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=8, noise_schedule="linear")
    tab, ref = m.completion_table(5, 10, 1, batch=3), m.ddpm_table(5, 3)
    assert tab.width == 3 and tab.stride == 1 and not tab.jumps
    for a, b in zip(tab.columns()[:4], ref.columns()):
        assert torch.equal(a, b)
    n_prev, _ = O.linear_schedule(torch.ones(3) * 2 / 5)
    assert torch.equal(tab.n2[1], n_prev)


@pytest.mark.parametrize("schedule,args,batch", [("linear", (5, 10, 1), 3), ("cosine", (12, 4, 2), 3)])
def test_completion_table_equals_the_per_step_loop(schedule, args, batch):
    """The table is built for all rows and the whole width at once; the statement's walk, one schedule call per row on the
    (width,) vector (tests/table_statement.py), gives the same bits -- on the linear schedule each row is its own batch-axis
    cumprod."""
    import table_statement as TS
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=8, noise_schedule=schedule)
    tab = m.completion_table(*args, batch=batch)
    want = TS.completion(*args, tab.width, O.schedule_fn(schedule))
    assert tab.width == (batch if schedule == "linear" else 1) and tab.steps == len(want["t"]) and tab.skip_last_update
    for f in ("t", "n", "s", "a", "b", "n2", "ja", "jb"):
        assert torch.equal(getattr(tab, f), want[f]), f


def test_new_symbols_declared_exported_and_bound():
    from shapegen_amd import _lib
    _lib.build()
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcd_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/pcd_hip.h"
        assert hasattr(lib, name) and name in _lib._SIGS
    assert lib.pcd_abi_version() == _lib.ABI_VERSION == 2
    # argument errors come back before any device work
    assert lib.pcd_complete_start(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == -1
    assert lib.pcd_complete_update(64, 64, 64, 0, 64, 64, 64, 1, 0, 12, 6, 3, 0, 0, 0) == -1       # neither x0 nor x_next
    assert lib.pcd_complete_update(64, 64, 0, 0, 64, 64, 64, 1, 0, 12, 6, 3, 64, 64, 0) == -1      # x_next without z
    assert lib.pcd_complete_update(64, 64, 64, 0, 64, 64, 64, 1, 0, 12, 5, 3, 64, 64, 0) == -1     # ragged shapes
    assert lib.pcd_complete_update_philox(64, 64, 64, 64, 64, 3, 1, 12, 6, 3, 0, 64, 64, 0, 0, 0, 0, 64, 0) == -1   # width != shapes
    assert lib.pcd_step_select_cols(64, 4, 64, 8, 64, 64, 0, 1, 64, 0) == -1


def test_complete_on_a_cpu_module_and_argument_checks():
    from shapegen_amd.diffusion import PointCloudDiffusion
    m = PointCloudDiffusion(num_points=16)
    part = _unit_clouds(2, 10, 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.complete(part, 16, num_steps=4)                                   # no CPU path: fail loudly
    with pytest.raises(RuntimeError, match="MI355X"):
        m.complete(part, 16, num_steps=8, known_counts=torch.tensor([0, 10]), resample=2, jump=2)
    bad = [dict(known_counts=torch.tensor([0, 11])),                        # above M
           dict(known_counts=torch.tensor([-1, 3])),
           dict(known_counts=torch.tensor([1, 2, 3])),                      # not (B,)
           dict(known_counts=torch.tensor([1.0, 2.0])),                     # not integers
           dict(resample=2, jump=0), dict(resample=2, jump=4), dict(resample=2, jump=9),     # jump outside [1, T)
           dict(resample=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            m.complete(part, 16, num_steps=4, **kw)
    with pytest.raises(ValueError):
        m.complete(_unit_clouds(2, 17, 3), 16, num_steps=4)                 # M > num_points
    with pytest.raises(ValueError):
        m.complete(_unit_clouds(2, 17, 3), 16, num_steps=4, known_counts=torch.tensor([17, 0]))
    for v in (float("nan"), float("inf")):
        p2 = part.clone()
        p2[1, 9, 2] = v
        with pytest.raises(ValueError, match="finite"):
            m.complete(p2, 16, num_steps=4)
    lin = PointCloudDiffusion(num_points=16, noise_schedule="linear")
    with pytest.raises(ValueError, match="cosine"):
        lin.complete(part, 16, num_steps=8, resample=2, jump=2)
    with pytest.raises(RuntimeError, match="MI355X"):
        lin.complete(part, 16, num_steps=8, resample=1)                     # resample = 1 is legal with the linear schedule
