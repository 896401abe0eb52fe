"""VAE3DLarge training step on the HIP kernels (shapegen_amd.training_vae.VAETrainer).  Three layers of evidence:
  1. every one of the 9 + 9 ops of the encoder and decoder programs driven through the trainer's own routines at its real
     grid and compared, link by link, with the float64 statement of that layer (tests/vae_train_statement.py, pinned to
     the oracle by tests/test_train_vae_statement_cpu.py) on the operands the kernels see (tight);
  2. the whole step against the oracle's autograd (oracle.torch_oracle.vae_training_step, pinned to the reference by
     tests/golden/train_vae.npz): with fp16 operands through ~30 conv layers this is a direction / magnitude check
     (measured: cosine >= 0.99, norm ratio 0.99..1.02 on every weight tensor), every 1-D tensor included, then two Adam
     steps against the oracle's;
  3. a change of batch size on one trainer against a fresh trainer per batch, bitwise.
The small kernels of the step have their own tests in test_gpu_train.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_train_statement as S
from helpers import rel_l2, as_torch
from oracle import torch_oracle as O
from oracle import make_golden as MG
from shapegen_amd import specs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():
        yield


def _vae_sd():
    return as_torch(specs.synth_state_dict(specs.vae3d_large_spec(prefix="vae."), seed=0, gain=1.3))


def _step_and_oracle():
    from shapegen_amd.training_vae import VAETrainer
    from shapegen_amd.vae import VAE3DLarge
    sd = _vae_sd()
    vae = VAE3DLarge()
    vae.load_state_dict({k[len("vae."):]: v for k, v in sd.items()}, strict=True)
    vae = vae.to("cuda")
    x = torch.from_numpy(MG.synth_voxels(2, 5))
    eps = torch.randn(2, 256, generator=torch.Generator().manual_seed(1))
    tr = VAETrainer(vae, lr=1e-4)
    tr.forward(x.cuda(), eps.cuda())
    losses = tr.backward(0.01)
    sd_ref = {k: v.clone() for k, v in sd.items()}
    ref = O.vae_training_step(sd_ref, "vae.", x, eps, 0.01, specs.VAE_ENC, specs.VAE_DEC)
    return sd, vae, x, eps, tr, losses, sd_ref, ref


def test_vae_training_step_against_oracle():
    sd, vae, x, eps, tr, (loss, recon_loss, kl), sd_ref, ref = _step_and_oracle()
    l_ref, r_ref, k_ref, recon_ref, mu_ref, lv_ref, grads_ref = ref
    # measured: mu / logvar 2e-3, loss 3e-4, reconstruction 1.5e-3, gradient cosines min 0.992 / median 0.997
    assert rel_l2(tr.mu.cpu(), mu_ref) < 1e-2 and rel_l2(tr.logvar.cpu(), lv_ref) < 1e-2
    assert abs(kl.item() - k_ref.item()) < 1e-2 * abs(k_ref.item())
    assert abs(recon_loss.item() - r_ref.item()) < 5e-3 * r_ref.item() and abs(loss.item() - l_ref.item()) < 5e-3 * l_ref.item()
    assert rel_l2(tr.recon.cpu(), recon_ref) < 1e-2
    grads = tr.grads()
    cos = {}
    n_zero = 0
    for k, gr in grads_ref.items():
        mine = grads[k[len("vae."):]].cpu()
        assert mine.shape == gr.shape and torch.isfinite(mine).all(), k
        if gr.dim() > 1 and gr.norm() > 0:
            cos[k] = F.cosine_similarity(mine.reshape(1, -1), gr.reshape(1, -1)).item()
            assert 0.9 < mine.norm().item() / gr.norm().item() < 1.1, (k, mine.norm().item(), gr.norm().item())
        if S.is_bias_before_batchnorm(k):
            wnorm = grads_ref[k[:-len("bias")] + "weight"].norm().item()
            # analytic zero (the batch mean removes the bias): the oracle holds fp32 residue, at most 1.1e-5 of the layer's
            # weight gradient; the trainer must not put anything larger there (the other 1-D tensors: next test)
            assert gr.norm().item() < 1e-4 * wnorm and mine.norm().item() < 1e-4 * wnorm, (k, mine.norm().item(), wnorm)
            n_zero += 1
    assert n_zero == 16
    low = sorted(cos.items(), key=lambda kv: kv[1])[:5]
    assert min(cos.values()) > 0.95 and np.median(list(cos.values())) > 0.98, low
    for k, v in vae.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            assert torch.allclose(v.cpu(), sd_ref["vae." + k], rtol=3e-2, atol=3e-2), k
    # Adam (AdamW with zero decay) on the trainer's own gradients, twice: the second step carries the moments
    params = {k: v.detach().cpu().clone() for k, v in vae.named_parameters()}
    state = {}
    for step in (1, 2):
        if step == 2:
            tr.forward(x.cuda(), eps.cuda())
            tr.backward(0.01)
            grads = tr.grads()
        tr.optimizer_step()
        O.adamw_step(params, {k: v.cpu() for k, v in grads.items()}, state, lr=1e-4, weight_decay=0.0)
        moved = 0
        for k, v in vae.named_parameters():
            assert torch.allclose(v.detach().cpu(), params[k], rtol=0, atol=2e-6), (step, k)
            moved += int(not torch.equal(params[k], sd["vae." + k]))
        assert moved >= len(params) - 16, moved                # all but (at most) the analytic-zero biases have moved
        shown = vae.state_dict()
        for k in ("encoder.12.weight", "decoder.0.bias", "fc_mu.bias", "decoder.11.bn2.weight"):
            assert torch.allclose(shown[k].cpu(), params[k], rtol=0, atol=2e-6) and not torch.equal(shown[k].cpu(), sd["vae." + k]), k


def test_vae_one_dimensional_gradients_against_oracle():
    """Every 1-D gradient of the step (conv / conv-transpose / downsample biases, BatchNorm gamma and beta, the three
    linear biases; not the analytic zeros in front of a BatchNorm) against the oracle's, by cosine and norm ratio.
    The bound is the reference side's own sensitivity with a margin of two: S.FP16_OPERAND_FLOOR is, per class, the worst
    1 - cosine and |log norm ratio| between the oracle's gradients as is and with fp16 conv / linear operands (measured on
    the CPU by test_train_vae_statement_cpu.py); the HIP path adds fp16 storage of activations and gradients on top.
        class       floor (1 - cos, |log ratio|)   bound              MI355X, worst tensor
        conv_bias   3.95e-3, 2.28e-2               7.90e-3, 4.56e-2   3.76e-3, 1.20e-2
        bn_gamma    4.55e-3, 2.72e-2               9.10e-3, 5.44e-2   4.98e-3, 1.53e-2
        bn_beta     4.52e-3, 1.64e-2               9.04e-3, 3.28e-2   5.01e-3, 1.63e-2
        fc_bias     3.53e-3, 2.74e-3               7.06e-3, 5.48e-3   3.77e-3, 1.72e-3
    The step is reproducible (every cross-block sum but the two loss sums adds its partials in a fixed order; see
    test_vae_batch_size_change_on_one_trainer), so these figures are the same in every run."""
    sd, vae, x, eps, tr, losses, sd_ref, ref = _step_and_oracle()
    grads, grads_ref = tr.grads(), ref[6]
    worst, misses = {}, []
    for k, gr in grads_ref.items():
        if gr.dim() != 1 or S.is_bias_before_batchnorm(k):
            continue
        c, lr = S.cos_and_log_ratio(grads[k[len("vae."):]].cpu(), gr)
        cls = S.tensor_class(k)
        floor_cos, floor_lr = S.FP16_OPERAND_FLOOR[cls]
        w = worst.setdefault(cls, [0.0, 0.0, 0])
        w[0], w[1], w[2] = max(w[0], 1 - c), max(w[1], abs(lr)), w[2] + 1
        if not (1 - c < 2 * floor_cos and abs(lr) < 2 * floor_lr):
            misses.append((k, cls, f"1 - cos {1 - c:.2e} (< {2 * floor_cos:.2e})", f"|log ratio| {abs(lr):.2e} (< {2 * floor_lr:.2e})"))
    print("1-D gradients, worst per class (1 - cos, |log norm ratio|, tensors):", worst)
    print("misses:", misses)
    assert {c: w[2] for c, w in worst.items()} == {"conv_bias": 14, "bn_gamma": 16, "bn_beta": 16, "fc_bias": 3}
    assert not misses, misses


def test_vae_training_reduces_the_loss():
    from shapegen_amd.training_vae import VAETrainer
    from shapegen_amd.vae import VAE3DLarge
    torch.manual_seed(0)
    vae = VAE3DLarge().to("cuda")                       # the reference's own initialisation
    tr = VAETrainer(vae, lr=1e-3)
    x = torch.from_numpy(MG.synth_voxels(4, 7)).cuda()
    eps = torch.randn(4, 256, device="cuda")
    losses = [float(tr.train_step(x, 0.01, eps)[0]) for _ in range(8)]
    assert np.isfinite(losses).all() and losses[-1] < 0.85 * losses[0], losses
    vae.eval()
    rec, mu, logvar = vae(x)
    assert torch.isfinite(rec).all() and rec.shape == x.shape


# ------------------------------------------------------------------ every op of the two programs, link by link
ACT, GRAD, DX_TWO_PATHS = 2e-3, 2e-3, 3e-3        # test_gpu_train.py::test_layerwise_backward_consistency's bounds
STATS = 2e-4                                      # batch mean / variance: see _check_block


def _trainer():
    from shapegen_amd.training_vae import VAETrainer
    from shapegen_amd.vae import VAE3DLarge
    sd = _vae_sd()
    vae = VAE3DLarge()
    vae.load_state_dict({k[len("vae."):]: v for k, v in sd.items()}, strict=True)
    vae = vae.to("cuda")
    return VAETrainer(vae, lr=1e-4), vae, sd


def _up64(v):
    return (v + 63) // 64 * 64


def _rows_input(g, rows, c):
    """fp16 activations [rows][c]: unit normal around a per-channel offset (E[x^2] - E[x]^2 would lose digits)."""
    off = torch.linspace(-1.5, 1.5, c) if c > 1 else torch.tensor([0.5])
    return (torch.randn(rows, c, generator=g) + off).half()


def _leaf(t):
    return t.detach().cpu().double().clone().requires_grad_(True)


def _close(name, got, want, bound):
    err = rel_l2(got, want)
    print(f"    {name:42s} {err:.2e}  (< {bound:.0e})")
    assert err < bound, (name, err, bound)


def _convT_rounding_emulation(a_in, w, bias, d_out, L, b, rounded=True):
    """ConvTranspose3d + bias + ReLU and its backward in torch on the CPU with the trainer's rounding points: fp16 operands,
    fp32 sums, fp16 stores, in the trainer's order of operations - the per-tap products P = x W[:, :, tap] stored in fp16,
    the taps that reach an output voxel (8 of 64 for k 4, s 2) summed in fp32 and stored in fp16, then + bias, ReLU, fp16;
    backward from the mask of that activation with fp32 sums and an fp16 input gradient.  With `rounded` False and float64
    operands it is the exact function (checked against the statement, so the fold below is right).
    -> (activation rows, input gradient rows, weight gradient, bias gradient)"""
    dt = torch.float32 if rounded else torch.float64
    r16 = (lambda t: t.half().to(dt)) if rounded else (lambda t: t)
    k, s, p, din, dout, cin, cout = L.k, L.s, L.p, L.din, L.dout, L.cin, L.cout
    P = r16(a_in.to(dt) @ w.to(dt).reshape(cin, cout * k ** 3)).reshape(b, din, din, din, cout, k, k, k)
    y = torch.zeros(b, dout, dout, dout, cout, dtype=dt)
    for kd in range(k):
        for kh in range(k):
            for kw in range(k):
                sl_in, sl_out = [], []
                for t in (kd, kh, kw):                    # output index o = i * s - p + t, kept where 0 <= o < dout
                    i0 = max(0, -((t - p) // s))
                    i1 = min(din - 1, (dout - 1 + p - t) // s)
                    sl_in.append(slice(i0, i1 + 1))
                    sl_out.append(slice(i0 * s - p + t, i1 * s - p + t + 1, s))
                y[:, sl_out[0], sl_out[1], sl_out[2]] += P[:, sl_in[0], sl_in[1], sl_in[2], :, kd, kh, kw]
    a = r16(r16(y).reshape(-1, cout) + bias.to(dt))
    a = r16(a.clamp_min(0)) if L.relu else a
    dz = torch.where(a > 0, d_out[:a.shape[0], :cout].to(dt), torch.zeros((), dtype=dt)) if L.relu else d_out[:a.shape[0], :cout].to(dt)
    x5 = S.rows_to_ncdhw(a_in, b, din, cin).to(dt).requires_grad_(True)
    w5 = w.to(dt).clone().requires_grad_(True)
    with torch.enable_grad():
        F.conv_transpose3d(x5, w5, None, stride=s, padding=p).backward(S.rows_to_ncdhw(dz, b, dout, cout))
    return a, r16(S.ncdhw_to_rows(x5.grad)), w5.grad, dz.sum(0)


def _check_single(tr, L, b, g):
    """One Conv3d / ConvTranspose3d + bias [+ ReLU] through `_conv_fwd` / `_conv_bwd`.

    The three ConvTranspose3d layers cannot meet the 2e-3 gradient bound against the unbranched statement, and it is a
    property of how they are computed, not a defect: the per-tap products are stored in fp16 before the 8 taps of an
    output voxel are added, so the pre-activation carries ~3e-4 of fp16 noise (a Conv3d's is an fp32 sum) and ~1e-4 of
    the ReLU decisions near zero fall on the other side; each flip moves a whole element of d_out in or out of dz.
    `_convT_rounding_emulation` shows the same on the CPU.  Against the float64 statement (input / weight / bias gradient):
        decoder.0   emulation 9.03e-3 / 9.10e-3 / 8.57e-3   MI355X 9.03e-3 / 9.10e-3 / 8.57e-3
        decoder.3   emulation 1.15e-2 / 1.16e-2 / 1.13e-2   MI355X 1.15e-2 / 1.16e-2 / 1.13e-2
        decoder.6   emulation 1.17e-2 / 1.18e-2 / 1.01e-2   MI355X 1.17e-2 / 1.18e-2 / 1.01e-2
    (the emulation reproduces the kernels' flips element for element).  For these layers the unbranched bound is
    twice the emulation's error, computed here on the same inputs (never
    below the project's 2e-3), and in addition the statement is branched at the mask of the stored activation (itself
    compared above at 2e-3), which holds the three gradients to the project's 2e-3 link by link."""
    m_in, m = b * L.din ** 3, b * L.dout ** 3
    assert m_in % 64 == 0                                   # the input rows need no padding at any layer
    a_in = _rows_input(g, m_in, L.cin)
    d_out = torch.zeros(_up64(m), L.cout if L.transposed else L.cp, dtype=torch.float16)
    d_out[:m, :L.cout] = torch.randn(m, L.cout, generator=g).half()
    a = tr._conv_fwd(L, a_in.cuda(), b, False).cpu()
    dx = tr._conv_bwd(L, d_out.cuda(), b, True).cpu()
    got = {"input": dx, "weight": tr.g[L.key + ".weight"].cpu(), "bias": tr.g[L.key + ".bias"].cpu()}
    w16 = tr.p[L.key + ".weight"].half()

    def statement(mask_from=None):
        x = _leaf(S.rows_to_ncdhw(a_in, b, L.din, L.cin))
        w, bias = _leaf(w16), _leaf(tr.p[L.key + ".bias"])
        ref = S.vconv(x, w, bias, bool(L.transposed), L.s, L.p, relu=L.relu and mask_from is None)
        assert ref["a"].shape == (b, L.cout, L.dout, L.dout, L.dout)
        d = d_out[:m, :L.cout]
        if mask_from is not None:
            d = torch.where(mask_from > 0, d, torch.zeros_like(d))
        ref["a"].backward(S.rows_to_ncdhw(d.double(), b, L.dout, L.cout))
        return ref["a"].detach(), {"input": S.ncdhw_to_rows(x.grad), "weight": w.grad, "bias": bias.grad}

    act, want = statement()
    assert a.shape == d_out.shape and not a[m:].any() and not a[:, L.cout:].any(), L.key      # padding rows / channels: exactly 0
    _close(L.key + " activation", a[:m, :L.cout], S.ncdhw_to_rows(act), ACT)
    assert dx.shape == (m_in, L.cin)
    bound = {"input": GRAD, "weight": GRAD, "bias": GRAD}
    if L.transposed:
        w64, b64 = w16.cpu().double(), tr.p[L.key + ".bias"].detach().cpu().double()
        exact = _convT_rounding_emulation(a_in.double(), w64, b64, d_out.double(), L, b, rounded=False)
        for e, r in zip(exact, (S.ncdhw_to_rows(act), want["input"], want["weight"], want["bias"])):
            assert rel_l2(e, r) < 1e-12
        emu = _convT_rounding_emulation(a_in, w16.cpu(), b64, d_out, L, b)
        for n, e in zip(("input", "weight", "bias"), emu[1:]):
            err = rel_l2(e, want[n])
            print(f"    {L.key} {n} gradient, CPU emulation of the rounding points vs statement: {err:.2e}")
            bound[n] = max(GRAD, 2 * err)
        _, branched = statement(mask_from=a[:m, :L.cout])
        for n in ("input", "weight", "bias"):
            _close(f"{L.key} {n} gradient (mask of the stored activation)", got[n], branched[n], GRAD)
    for n in ("input", "weight", "bias"):
        _close(f"{L.key} {n} gradient", got[n], want[n], bound[n])


def _check_block(tr, op, b, g):
    """One residual block through the one-op program [op] of `_run_fwd` / `_run_bwd`.  The statement branches at the
    fp16 tensors the trainer stored in forward (conv1's activation for conv2; conv2's BatchNorm output and the identity
    path for the tail, which is then exact), each of which is compared with its own statement first.  The backward
    statement does not branch: conv1's gradients come from the float64 gradient of conv2's link.
    Batch mean / variance (STATS): the BatchNorm kernel's own bound on fp32 input is 1e-4
    (test_train_kernels_against_torch); z here is an fp32-accumulated sum of up to 13824 fp16 products, whose rounding
    (sqrt(K) * 2^-24 ~ 7e-6 of z, twice that in z^2) doubles it at most.  MI355X: mean <= 4.1e-7, variance <= 1.0e-6."""
    _, c1, c2, dn = op
    key = c1.key[:-len(".conv1")]
    d, cin, cout = c1.din, c1.cin, c1.cout
    m = b * d ** 3
    assert m % 64 == 0
    a_in = _rows_input(g, m, cin)
    d_out = torch.randn(m, cout, generator=g).half()
    out = tr._run_fwd([op], a_in.cuda(), b, False).cpu()
    layers = [("conv1", c1), ("conv2", c2)] + ([("downsample", dn)] if dn is not None else [])
    st = {n: {"z": L.z.cpu().clone(), "a": L.a.cpu().clone(),
              "mean": L.mean.cpu().clone() if L.bn else None, "var": L.var.cpu().clone() if L.bn else None} for n, L in layers}
    blk_out = c2.out.cpu().clone()
    dx = tr._run_bwd([op], d_out.cuda(), b, True).cpu()
    names = ["conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias", "conv2.weight", "conv2.bias", "bn2.weight", "bn2.bias"]
    names += ["downsample.weight", "downsample.bias"] if dn is not None else []
    P = {n: _leaf(tr.p[f"{key}.{n}"].half() if n in ("conv1.weight", "conv2.weight", "downsample.weight") else tr.p[f"{key}.{n}"])
         for n in names}
    x = _leaf(S.rows_to_ncdhw(a_in, b, d, cin))
    # ---- forward links
    r1 = S.vconv(x, P["conv1.weight"], P["conv1.bias"], False, 1, 1, P["bn1.weight"], P["bn1.bias"], relu=True)
    h = _leaf(S.rows_to_ncdhw(st["conv1"]["a"], b, d, cout))                  # branch: conv2 reads what conv1 stored
    r2 = S.vconv(h, P["conv2.weight"], P["conv2.bias"], False, 1, 1, P["bn2.weight"], P["bn2.bias"], relu=False)
    for n, r in (("conv1", r1), ("conv2", r2)):
        s = st[n]
        assert s["z"].dtype == torch.float32 and s["a"].dtype == torch.float16
        _close(f"{key}.{n} z", s["z"][:, :cout], S.ncdhw_to_rows(r["z"].detach()), ACT)
        _close(f"{key}.{n} batch mean", s["mean"][:cout], r["mean"].detach(), STATS)
        _close(f"{key}.{n} batch variance", s["var"][:cout], r["var"].detach(), STATS)
        _close(f"{key}.{n} activation", s["a"][:, :cout], S.ncdhw_to_rows(r["a"].detach()), ACT)
        assert not s["a"][:, cout:].any() and not s["z"][:, cout:].any(), (key, n)        # padding channels: exactly 0
    if dn is not None:
        r = S.conv(x, P["downsample.weight"], P["downsample.bias"], False, 1, 0)
        _close(f"{key}.downsample activation", st["downsample"]["a"][:, :cout], S.ncdhw_to_rows(r.detach()), ACT)
        assert not st["downsample"]["a"][:, cout:].any()
        ident = st["downsample"]["a"]
    else:
        r = x
        ident = torch.zeros(m, c2.cp, dtype=torch.float16)
        ident[:, :cin] = a_in
    # the tail on the stored fp16 operands is one fp32 add and one rounding: exact
    want_out = (st["conv2"]["a"].float() + ident.float()).clamp_min(0).half()
    assert torch.equal(blk_out, want_out) and torch.equal(out, blk_out[:, :cout]), key
    assert S.res_block(x.detach(), {k: v.detach() for k, v in P.items()})["out"].shape == (b, cout, d, d, d)
    # ---- backward: the shared mask is the stored block output's
    dm = S.rows_to_ncdhw(torch.where(blk_out[:, :cout] > 0, d_out, torch.zeros_like(d_out)).double(), b, d, cout)
    r2["a"].backward(dm)
    r1["a"].backward(h.grad)
    if dn is not None:
        r.backward(dm)
        want_dx = x.grad
    else:
        want_dx = x.grad + dm
    for n in names:
        if S.is_bias_before_batchnorm(f"{key}.{n}"):
            continue                              # analytic zero: the trainer never writes it (checked in the whole step)
        _close(f"{key}.{n} gradient", tr.g[f"{key}.{n}"].cpu(), P[n].grad, GRAD)
    assert dx.shape == (m, cin)
    _close(f"{key} input gradient", dx, S.ncdhw_to_rows(want_dx), DX_TWO_PATHS)


def test_vae_layers_against_statement():
    """All 9 + 9 ops of VAE_ENC / VAE_DEC at their real grids (32 / 16 / 8 / 4 / 1 cubed), batch 2, through the trainer's
    own `_conv_fwd` / `_conv_bwd` (single layers) and `_run_fwd` / `_run_bwd` (residual blocks, with and without
    `downsample`), against the float64 statement on the operands the kernels see: fp16 input rows, the fp16 image of the
    weights, fp32 bias / gamma / beta, a dense fp16 output gradient (unscaled, so `tr.g` is the gradient itself)."""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    tr, vae, sd = _trainer()
    checked, kinds = 0, set()
    for ops in (tr.enc, tr.dec):
        for op in ops:
            g = torch.Generator().manual_seed(1000 + checked)
            print(f"  {op[1].key}  ({op[0]}, {op[1].cin} -> {op[1].cout}, grid {op[1].din} -> {op[1].dout})")
            if op[0] == "conv":
                _check_single(tr, op[1], 2, g)
                kinds.add("convT" if op[1].transposed else "conv")
            else:
                _check_block(tr, op, 2, g)
                kinds.add("res+downsample" if op[3] is not None else "res")
            checked += 1
    assert checked == 18 and kinds == {"conv", "convT", "res", "res+downsample"}


# ------------------------------------------------------------------ one trainer, several batch sizes
def _fixed_step(tr, x, eps):
    tr.forward(x.cuda(), eps.cuda(), update_stats=False)
    loss, recon_loss, kl = tr.backward(0.01)
    out = {"loss": loss.item(), "recon_loss": recon_loss.item(), "kl": kl.item(), "mu": tr.mu.clone(), "logvar": tr.logvar.clone(),
           "recon": tr.recon.clone()}
    out.update({"grad " + k: v.clone() for k, v in tr.g.items()})
    return out


def _enc12_step(tr, a_in, d_out, b):
    op = tr.enc[-1]
    L = op[1]
    out = tr._run_fwd([op], a_in[:b * 64].cuda(), b, False)
    dx = tr._run_bwd([op], d_out[:b].cuda(), b, True)
    return {"activation": out.clone(), "input gradient": dx.clone(), "weight gradient": tr.g[L.key + ".weight"].clone(),
            "bias gradient": tr.g[L.key + ".bias"].clone()}


def test_encoder12_across_batch_size_changes_bitwise():
    """encoder.12 (Conv3d 512 -> 512, k 4, 4 cubed -> 1) is the one layer with fewer output rows (M = B) than its 64-row
    buffers, and its weight-gradient product reduces over all 64 rows: rows a larger batch wrote must not reach a
    smaller one.  Its one-op program (`_run_fwd` / `_run_bwd`: gather, GEMMs, mask, `_widen`, col2im) on one trainer at
    batch 4, 2, 3, 2, 4 equals a fresh trainer per batch size bitwise.  Before `_rows_buf` cleared the tail rows the
    step at batch 2 after batch 4 summed the weight gradient of both batches (this layer's own figure on the parent's
    trainer: the first assertion to fail is the activation with its padding rows, 9.6e-1 rel-L2 at 4 -> 2;
    in the whole step encoder.12.weight's gradient is 5.8e-1 off)."""
    g = torch.Generator().manual_seed(21)
    a_in, d_out = _rows_input(g, 4 * 64, 512), torch.randn(4, 512, generator=g).half()
    fresh = {}
    for b in (4, 2, 3):
        tr, vae, sd = _trainer()
        fresh[b] = _enc12_step(tr, a_in, d_out, b)
    tr, vae, sd = _trainer()
    for n, b in enumerate((4, 2, 3, 2, 4)):
        got = _enc12_step(tr, a_in, d_out, b)
        for k, want in fresh[b].items():
            assert torch.equal(got[k], want), (n, b, k, rel_l2(got[k], want))
        assert not got["activation"][b:].any()


def test_vae_batch_size_change_on_one_trainer():
    """Whole steps at batch 4, 2, 3, 2, 4 on one trainer (forward + backward, fixed eps, running statistics untouched)
    against a fresh trainer per batch size: mu, logvar, recon and all 98 gradients bitwise; loss, recon_loss and kl, whose
    sums are atomicAdd-ed per block, at 1e-6 relative.  Every other cross-block sum of the step (BatchNorm statistics
    and their backward, column sums, the few-row fp32 products) adds its per-block partials in a fixed order, so a step
    is reproducible and anything a batch leaves behind in the workspace shows.  On the parent's trainer the stale rows
    of encoder.12 gave its weight gradient 5.8e-1 rel-L2 off at 4 -> 2 and 3.4e-1 at 2 -> 3."""
    xs = torch.from_numpy(MG.synth_voxels(4, 9))
    eps = torch.randn(4, 256, generator=torch.Generator().manual_seed(3))
    fresh = {}
    for b in (4, 2, 3):
        tr, vae, sd = _trainer()
        fresh[b] = _fixed_step(tr, xs[:b], eps[:b])
        del tr, vae
    tr, vae, sd = _trainer()
    for n, b in enumerate((4, 2, 3, 2, 4)):
        got = _fixed_step(tr, xs[:b], eps[:b])
        assert sorted(got) == sorted(fresh[b]) and len(got) == 6 + 98
        for k, want in fresh[b].items():
            if isinstance(want, float):
                assert abs(got[k] - want) <= 1e-6 * abs(want), (n, b, k, got[k], want)
            else:
                assert torch.equal(got[k], want), (n, b, k, rel_l2(got[k], want))
    for k, v in vae.state_dict().items():          # update_stats=False: the module is as loaded
        assert torch.equal(v.cpu(), sd["vae." + k]), k
