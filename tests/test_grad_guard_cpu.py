"""Host-side checks of the gradient guard (clipping, accumulation, non-finite step guard): the boundary, the argument
checks, the float64 statement the GPU tests compare against, and `fit`'s surface."""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_guard_statement as S  # noqa: E402

NEW = ("pcd_grad_norm_f32", "pcd_adamw_guarded_step", "pcd_grad_accumulate_f32")


def _lib():
    from shapegen_amd import _lib as L
    L.build()
    return L, L.load()


def test_new_symbols_are_exported_and_bound():
    L, lib = _lib()
    for name in NEW:
        assert name in L._SIGS, f"{name} has no ctypes prototype"
        assert getattr(lib, name).argtypes == L._SIGS[name][1]
    assert lib.pcd_abi_version() == L.ABI_VERSION == 2          # additive: the version does not move


P = 64          # a non-null pointer that an argument check never dereferences


@pytest.mark.parametrize("call", [
    lambda lib: lib.pcd_grad_norm_f32(None, 8, 1024.0, 1.0, 1, 0.9, 0.999, P, None),
    lambda lib: lib.pcd_grad_norm_f32(P, 8, 1024.0, 1.0, 1, 0.9, 0.999, None, None),
    lambda lib: lib.pcd_grad_norm_f32(P, 0, 1024.0, 1.0, 1, 0.9, 0.999, P, None),
    lambda lib: lib.pcd_grad_norm_f32(P, -3, 1024.0, 1.0, 1, 0.9, 0.999, P, None),
    lambda lib: lib.pcd_grad_norm_f32(P, 8, 0.0, 1.0, 1, 0.9, 0.999, P, None),
    lambda lib: lib.pcd_grad_norm_f32(P, 8, -1.0, 1.0, 1, 0.9, 0.999, P, None),
    lambda lib: lib.pcd_grad_norm_f32(P, 8, 1024.0, 1.0, 0, 0.9, 0.999, P, None),
    lambda lib: lib.pcd_adamw_guarded_step(None, P, P, P, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, P, None),
    lambda lib: lib.pcd_adamw_guarded_step(P, None, P, P, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, P, None),
    lambda lib: lib.pcd_adamw_guarded_step(P, P, None, P, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, P, None),
    lambda lib: lib.pcd_adamw_guarded_step(P, P, P, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, P, None),
    lambda lib: lib.pcd_adamw_guarded_step(P, P, P, P, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, None, None),
    lambda lib: lib.pcd_adamw_guarded_step(P, P, P, P, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, P, None),
    lambda lib: lib.pcd_adamw_guarded_step(P, P, P, P, P, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, P, None),
    lambda lib: lib.pcd_grad_accumulate_f32(None, P, 8, 1, None),
    lambda lib: lib.pcd_grad_accumulate_f32(P, None, 8, 0, None),
    lambda lib: lib.pcd_grad_accumulate_f32(P, P, 0, 1, None),
])
def test_argument_checks(call):
    """Every bad argument is refused on the host, before any device work."""
    _, lib = _lib()
    assert call(lib) == -1
    assert b"bad argument" in lib.pcd_last_error()


def test_statement_against_torch_clip_and_adamw():
    """Five steps with gradient magnitudes 1, 10, 0.1, 10, 1 and a max_norm that clips the second and fourth only:
    the statement against clip_grad_norm_ + AdamW in fp32, to the 2e-6 tests/test_resume_cpu.py holds adamw_step to."""
    n, hyper = 1000, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    g = torch.Generator().manual_seed(3)
    w = torch.nn.Parameter(torch.randn(n, generator=g))
    opt = torch.optim.AdamW([w], **hyper)
    max_norm = 3.0 * n ** 0.5                    # norms are about sqrt(n) * magnitude
    st = S.GuardedAdamW(w.data, max_norm=max_norm, **hyper)
    for k, mag in enumerate((1.0, 10.0, 0.1, 10.0, 1.0), start=1):
        gr = torch.randn(n, generator=g) * mag
        w.grad = gr.clone()
        total = torch.nn.utils.clip_grad_norm_([w], max_norm)
        opt.step()
        assert st.step(gr)
        assert abs(st.norms[-1] - float(total)) <= 1e-6 * float(total)
        assert (w.detach().double() - st.p).abs().max() <= 2e-6, k
        state = opt.state[w]
        assert (state["exp_avg"].double() - st.m1).abs().max() <= 2e-6
        assert (state["exp_avg_sq"].double() - st.m2).abs().max() <= 2e-6
    assert (st.applied, st.clipped, st.skipped, st.t) == (5, 2, 0, 5)


def test_statement_skips_like_found_inf():
    """A non-finite gradient changes nothing and does not advance AdamW's step: the run with a poisoned step in the
    middle is the run without that step."""
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(100, generator=g)
    grads = [torch.randn(100, generator=g) for _ in range(3)]
    bad = grads[1].clone()
    bad[17] = float("nan")
    a, b = S.GuardedAdamW(p0), S.GuardedAdamW(p0)
    a.step(grads[0]); a.step(grads[2])
    b.step(grads[0])
    before = b.p.clone()
    assert not b.step(bad) and torch.equal(b.p, before)
    b.step(grads[2])
    assert torch.equal(a.p, b.p) and torch.equal(a.m2, b.m2)
    assert (b.applied, b.skipped, b.t) == (2, 1, 2)
    for poison in (float("inf"), float("-inf")):
        bad[17] = poison
        assert not S.GuardedAdamW(p0).step(bad)


def test_fit_signature_has_the_three_keywords():
    from shapegen_amd.training import fit
    prm = inspect.signature(fit).parameters
    assert prm["gradient_clip_val"].default is None
    assert prm["accumulate_grad_batches"].default == 1
    assert prm["skip_nonfinite"].default is False
