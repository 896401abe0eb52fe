"""Training step on the HIP kernels (shapegen_amd.training.PointTrainer, csrc/train.hip).

Three layers of evidence, because the network itself is ill-conditioned for end-to-end gradient comparison: in
train() mode (batch statistics, ReLU masks, max-pool argmax, sign() of the L1 loss) the ORACLE's own gradients
move by ~25 % relative L2 when the input is perturbed by 3e-4 (measured with the reference's own initialisation
too), so no reduced-precision implementation can match them tightly through 28 layers.
  1. every kernel of csrc/train.hip against a torch fp32 statement of the same op (tight);
  2. layer-wise consistency: each layer's BatchNorm/conv backward recomputed in torch fp32 from the tensors the
     HIP path saved and the gradient it received (tight) - proves the arithmetic of the chain link by link;
  3. the whole step against the oracle's autograd (tests/golden/train.npz pins the oracle to the reference):
     prediction and loss close, gradient directions aligned (a wiring mistake gives cosine ~0), BatchNorm
     running statistics, one exact AdamW update, and the loss going down over a few steps."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import point_sd, rel_l2
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _autograd_on():
    # other test modules switch autograd off process-wide; the torch references below need it
    with torch.enable_grad():
        yield


def _lib():
    from shapegen_amd import _lib
    return _lib, _lib.load(), _lib.stream_ptr()


def test_train_kernels_against_torch():
    L, lib, st = _lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    m, c = 2304, 200                                    # ragged column count: 200 = 3 * 64 + 8
    z = torch.randn(m, c, device="cuda", generator=g) * 0.7 + torch.linspace(-30, 30, c, device="cuda")   # |mean| >> std
    gamma = torch.rand(c, device="cuda", generator=g) + 0.5
    beta = torch.randn(c, device="cuda", generator=g) * 0.3
    mean, var = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    scratch = torch.empty(2 * c, device="cuda")
    L.check(lib.pcd_bn_batch_stats(z.data_ptr(), m, c, 0.1, mean.data_ptr(), var.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                   scratch.data_ptr(), st))
    assert torch.allclose(mean, z.mean(0), rtol=1e-5, atol=1e-5)
    assert torch.allclose(var, z.var(0, unbiased=False), rtol=1e-4)
    assert torch.allclose(rm, 0.1 * z.mean(0), rtol=1e-5, atol=1e-6) and torch.allclose(rv, 0.9 + 0.1 * z.var(0), rtol=1e-4)
    a = torch.empty(m, c, dtype=torch.float16, device="cuda")
    L.check(lib.pcd_bn_apply_f16(z.data_ptr(), m, c, mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, 1,
                                 a.data_ptr(), st))
    zr = z.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ar = F.relu(F.batch_norm(zr, None, None, gr, br, True, 0.1, 1e-5))
    assert rel_l2(a.float(), ar.detach()) < 5e-4
    da = (torch.randn(m, c, device="cuda", generator=g) * 3).half()
    ar.backward(da.float())
    dg, db = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    dz = torch.empty(m, c, dtype=torch.float16, device="cuda")
    L.check(lib.pcd_bn_backward_f16(da.data_ptr(), z.data_ptr(), m, c, mean.data_ptr(), var.data_ptr(), gamma.data_ptr(),
                                    beta.data_ptr(), 1e-5, 1, dg.data_ptr(), db.data_ptr(), dz.data_ptr(), st))
    # borderline ReLU-mask elements (bn(z) ~ 0) may fall on either side: a handful of flips in 2304 x 200
    assert rel_l2(dg, gr.grad) < 2e-3 and rel_l2(db, br.grad) < 2e-3
    assert rel_l2(dz.float(), zr.grad) < 3e-3
    # column sums per group, transpose
    x = torch.randn(6 * 500, 72, device="cuda", generator=g).half()
    out = torch.empty(6, 72, device="cuda")
    L.check(lib.pcd_colsum_f16(x.data_ptr(), 500, 6, 72, out.data_ptr(), st))
    assert torch.allclose(out, x.float().reshape(6, 500, 72).sum(1), rtol=1e-4, atol=1e-3)
    xt = torch.empty(72, 3000, dtype=torch.float16, device="cuda")
    L.check(lib.pcd_transpose_f16(x.data_ptr(), 3000, 72, xt.data_ptr(), st))
    assert torch.equal(xt, x.t().contiguous())
    xo = torch.randn(1001, 37, device="cuda", generator=g).half()                      # odd sizes: scalar edge path
    xot = torch.empty(37, 1001, dtype=torch.float16, device="cuda")
    L.check(lib.pcd_transpose_f16(xo.data_ptr(), 1001, 37, xot.data_ptr(), st))
    assert torch.equal(xot, xo.t().contiguous())
    # max-pool with first-index argmax (ties included) and its scatter
    b, n, cc = 3, 257, 130
    act = torch.randint(0, 5, (b * n, cc), device="cuda", generator=g).half()          # many exact ties
    mx, arg = torch.empty(b, cc, device="cuda"), torch.empty(b, cc, dtype=torch.int32, device="cuda")
    L.check(lib.pcd_colmax_argmax_f16(act.data_ptr(), b, n, cc, mx.data_ptr(), arg.data_ptr(), st))
    v, i = act.float().reshape(b, n, cc).cpu().max(1)                                 # CPU torch.max: first index on ties
    assert torch.equal(mx.cpu(), v) and torch.equal(arg.cpu().long(), i)
    dgm = torch.randn(b, cc, device="cuda", generator=g)
    dact = torch.empty(b * n, cc, dtype=torch.float16, device="cuda")
    L.check(lib.pcd_maxpool_backward_f16(dgm.data_ptr(), arg.data_ptr(), b, n, cc, dact.data_ptr(), st))
    want = torch.zeros(b, n, cc, device="cuda").scatter_(1, arg.long().unsqueeze(1), dgm.unsqueeze(1)).reshape(b * n, cc)
    assert torch.equal(dact, want.half())
    # K = 3 / C = 3 edge layers
    mm = 4096
    xyz = torch.randn(mm, 3, device="cuda", generator=g)
    w3 = torch.randn(64, 3, device="cuda", generator=g)
    tb = torch.randn(4, 64, device="cuda", generator=g)
    z0 = torch.empty(mm, 64, device="cuda")
    L.check(lib.pcd_enc1_linear(xyz.data_ptr(), mm, 1024, w3.data_ptr(), 64, tb.data_ptr(), z0.data_ptr(), st))
    assert torch.allclose(z0, xyz @ w3.t() + tb.repeat_interleave(1024, 0), rtol=1e-5, atol=1e-5)
    mat = torch.randn(mm, 64, device="cuda", generator=g).half()
    o3, vs = torch.empty(3, 64, device="cuda"), torch.empty(3, device="cuda")
    L.check(lib.pcd_vec3_outer(mat.data_ptr(), xyz.data_ptr(), mm, 64, o3.data_ptr(), vs.data_ptr(), st))
    assert torch.allclose(o3, xyz.t() @ mat.float(), rtol=1e-4, atol=1e-3) and torch.allclose(vs, xyz.sum(0), rtol=1e-4, atol=1e-3)
    wh = torch.randn(3, 64, device="cuda", generator=g)
    ex = torch.empty(mm, 64, dtype=torch.float16, device="cuda")
    L.check(lib.pcd_vec3_expand_f16(xyz.data_ptr(), wh.data_ptr(), mm, 64, ex.data_ptr(), st))
    assert rel_l2(ex.float(), xyz @ wh) < 5e-4
    # L1 loss and its gradient, small fp32 products, SiLU, AdamW
    pred, tgt = torch.randn(3000, device="cuda", generator=g), torch.randn(3000, device="cuda", generator=g)
    pred[:7] = tgt[:7]                                                                  # sign(0) = 0
    ls, dp = torch.empty(1, device="cuda"), torch.empty(3000, device="cuda")
    L.check(lib.pcd_l1_loss(pred.data_ptr(), tgt.data_ptr(), 3000, 8.0, ls.data_ptr(), dp.data_ptr(), st))
    assert abs(ls.item() / 3000 - F.l1_loss(tgt, pred).item()) < 1e-5
    assert torch.equal(dp, 8.0 * torch.sign(pred - tgt) / 3000)
    A, Bm = torch.randn(7, 33, device="cuda", generator=g), torch.randn(33, 19, device="cuda", generator=g)
    bias = torch.randn(19, device="cuda", generator=g)
    Cm = torch.empty(7, 19, device="cuda")
    L.check(lib.pcd_matmul_f32(A.data_ptr(), 33, 0, Bm.data_ptr(), 19, 0, 7, 19, 33, bias.data_ptr(), 0, Cm.data_ptr(), 19, st))
    assert torch.allclose(Cm, A @ Bm + bias, rtol=1e-5, atol=1e-5)
    At, Bt = A.t().contiguous(), Bm.t().contiguous()
    L.check(lib.pcd_matmul_f32(At.data_ptr(), 7, 1, Bt.data_ptr(), 33, 1, 7, 19, 33, None, 1, Cm.data_ptr(), 19, st))
    assert torch.allclose(Cm, 2 * (A @ Bm) + bias, rtol=1e-5, atol=1e-4)
    for (mr, nr, kr) in ((16, 1024, 4096), (5, 70, 300), (32, 4096, 1024)):          # few-row fast paths, both B layouts
        Af = torch.randn(mr, kr, device="cuda", generator=g)
        Bn, bb = torch.randn(kr, nr + 3, device="cuda", generator=g), torch.randn(nr, device="cuda", generator=g)
        Cf = torch.zeros(mr, nr, device="cuda")
        L.check(lib.pcd_matmul_f32(Af.data_ptr(), kr, 0, Bn.data_ptr(), nr + 3, 0, mr, nr, kr, bb.data_ptr(), 0, Cf.data_ptr(), nr, st))
        assert rel_l2(Cf, Af @ Bn[:, :nr] + bb) < 1e-5
        Bt = Bn[:, :nr].t().contiguous()
        L.check(lib.pcd_matmul_f32(Af.data_ptr(), kr, 0, Bt.data_ptr(), kr, 1, mr, nr, kr, None, 1, Cf.data_ptr(), nr, st))
        assert rel_l2(Cf, 2 * (Af @ Bn[:, :nr]) + bb) < 1e-5
    xs = torch.randn(500, device="cuda", generator=g).requires_grad_(True)
    y, dy, dx = torch.empty(500, device="cuda"), torch.randn(500, device="cuda", generator=g), torch.empty(500, device="cuda")
    L.check(lib.pcd_silu_f32(xs.data_ptr(), 500, y.data_ptr(), st))
    L.check(lib.pcd_silu_backward_f32(xs.data_ptr(), dy.data_ptr(), 500, dx.data_ptr(), st))
    F.silu(xs).backward(dy)
    assert torch.allclose(y, F.silu(xs.detach()), rtol=1e-5, atol=1e-6) and torch.allclose(dx, xs.grad, rtol=1e-4, atol=1e-6)
    w = torch.randn(1000, device="cuda", generator=g)
    wr = torch.nn.Parameter(w.clone())
    opt = torch.optim.AdamW([wr], lr=1e-3, weight_decay=1e-2)
    m1, m2 = torch.zeros_like(w), torch.zeros_like(w)
    for step in (1, 2, 3):
        gr_ = torch.randn(1000, device="cuda", generator=g)
        wr.grad = gr_.clone()
        opt.step()
        gs = gr_ * 64.0
        L.check(lib.pcd_adamw_step(w.data_ptr(), gs.data_ptr(), m1.data_ptr(), m2.data_ptr(), 1000, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step,
                                   64.0, st))
        assert torch.allclose(w, wr.detach(), rtol=0, atol=2e-6)


def _setup(golden):
    from shapegen_amd.diffusion import PointCloudDiffusion
    g = golden("train.npz")
    sd = point_sd()
    model = PointCloudDiffusion(num_points=128)
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda")
    x_t, t, noise = (torch.from_numpy(g[k]) for k in ("x_t", "t", "noise"))
    return model, sd, x_t, t, noise, g


def test_layerwise_backward_consistency(golden):
    """Every conv+BN+ReLU link of the backward chain, recomputed by torch autograd (fp32) from the tensors the HIP
    path saved in forward and the gradient it fed into the link."""
    from shapegen_amd.training import PointTrainer
    model, sd, x_t, t, noise, g = _setup(golden)
    tr = PointTrainer(model.model)
    tr.debug = {}
    tr.forward(x_t.cuda(), t.cuda(), update_stats=False)
    tr.backward(noise.cuda())
    grads = tr.g
    checked = 0
    for L in tr._all_convs():
        if L.conv == "enc1.conv1" or not L.bn:
            continue
        a_in = torch.cat([a.float() for a, _ in L.inputs], dim=1)
        w = tr.p[L.conv + ".weight"].detach()
        w2 = (w[:, 4096:, 0] if L.conv == "dec4.conv1" else w.view(w.shape[0], -1)).clone().requires_grad_(True)
        a_in = a_in.clone().requires_grad_(True)
        gam = tr.p[L.bn + ".weight"].detach().clone().requires_grad_(True)
        bet = tr.p[L.bn + ".bias"].detach().clone().requires_grad_(True)
        z = a_in @ w2.half().float().t()
        z = z + (tr.gbias.repeat_interleave(tr.n, 0) if L.conv == "dec4.conv1" else tr.p[L.conv + ".bias"].detach())
        assert rel_l2(L.z, z.detach()) < 2e-3, L.conv
        zz = L.z.clone().requires_grad_(True)                       # branch the graph at the saved z
        a = F.relu(F.batch_norm(zz, None, None, gam, bet, True, 0.1, 1e-5))
        assert rel_l2(L.a.float(), a.detach()) < 1e-3, L.conv
        da = tr.debug[L.conv + ".da"].float()
        a.backward(da)
        dz = tr.debug[L.conv + ".dz"].float()
        assert rel_l2(dz, zz.grad) < 2e-3, L.conv
        assert rel_l2(grads[L.bn + ".weight"], gam.grad) < 2e-3 and rel_l2(grads[L.bn + ".bias"], bet.grad) < 2e-3, L.conv
        (a_in @ w2.t()).backward(dz)
        gw = grads[L.conv + ".weight"]
        gw2 = gw[:, 4096:, 0] if L.conv == "dec4.conv1" else gw.view(gw.shape[0], -1)
        assert rel_l2(gw2, w2.grad) < 2e-3, L.conv
        k0 = 0
        for a_src, k in L.inputs:
            key = f"{L.conv}.din{k0}"
            if key in tr.debug:
                got = tr.debug[key].float()
                before = [v for kk, v in tr.debug.items() if kk.startswith(L.conv + ".in") and kk.endswith("before_add")]
                want = a_in.grad[:, k0:k0 + k] + (before[0].float() if before and got.shape == before[0].shape else 0)
                assert rel_l2(got, want) < 3e-3, (L.conv, k0)
            k0 += k
        checked += 1
    assert checked == 26          # 11 encoder + 2 global + 12 decoder + output.0 (enc1.conv1 is the K = 3 + 256 special case)


def test_training_step_against_oracle(golden):
    from shapegen_amd.training import PointTrainer
    model, sd, x_t, t, noise, g = _setup(golden)
    tr = PointTrainer(model.model, lr=1e-4)
    pred = tr.forward(x_t.cuda(), t.cuda())
    loss = tr.backward(noise.cuda())
    sd_ref = {k: v.clone() for k, v in sd.items()}
    loss_ref, grads_ref = O.point_training_step(sd_ref, "model.", x_t, t, noise)
    assert rel_l2(pred.cpu(), torch.from_numpy(g["pred"])) < 6e-2          # the oracle itself: 1.1e-2 for a 3e-4 input change
    assert abs(loss.item() - loss_ref.item()) <= 1e-2 * loss_ref.item()
    grads = tr.grads()
    cos = {}
    for k, gr in grads_ref.items():
        mine = grads[k[len("model."):]].cpu()
        assert mine.shape == gr.shape and torch.isfinite(mine).all(), k
        if gr.dim() > 1 and gr.norm() > 0:
            cos[k] = F.cosine_similarity(mine.reshape(1, -1), gr.reshape(1, -1)).item()
            assert 0.8 < mine.norm().item() / gr.norm().item() < 1.25, k
    # measured: cosine min 0.94 / median 0.95, norm ratios 0.94..1.01, prediction 2.5e-2, loss 1e-3
    assert min(cos.values()) > 0.85 and np.median(list(cos.values())) > 0.9, sorted(cos.items(), key=lambda kv: kv[1])[:5]
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            assert torch.allclose(v.cpu(), sd_ref[k], rtol=2e-2, atol=2e-2), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(sd_ref[k])


def test_adamw_update_and_loss_decreases(golden):
    from shapegen_amd.training import PointTrainer
    model, sd, x_t, t, noise, g = _setup(golden)
    tr = PointTrainer(model.model, lr=1e-4)
    # one step against the oracle's AdamW on the HIP gradients (isolates the optimizer kernel)
    tr.forward(x_t.cuda(), t.cuda())
    tr.backward(noise.cuda())
    grads = {k: v.cpu() for k, v in tr.grads().items()}
    params = {k: v.detach().cpu().clone() for k, v in model.model.named_parameters()}
    tr.optimizer_step()
    O.adamw_step(params, grads, {}, lr=1e-4, weight_decay=1e-5)
    for k, v in model.model.named_parameters():
        assert torch.allclose(v.detach().cpu(), params[k], rtol=0, atol=3e-7), k
    # the state_dict is the trained weights (parameters are views of the flat buffer) and the sampler sees them
    assert torch.allclose(model.state_dict()["model.output.3.weight"].cpu(), params["output.3.weight"], rtol=0, atol=3e-7)
    # loading weights after the trainer exists refreshes its fp16 operand copies (the flat buffer is written in place)
    w16_before = tr.w16["enc2.conv1"].clone()
    model.load_state_dict(sd, strict=True)
    assert torch.equal(model.state_dict()["model.enc2.conv1.weight"].cpu(), sd["model.enc2.conv1.weight"])
    assert not torch.equal(tr.w16["enc2.conv1"], w16_before)
    assert torch.equal(tr.w16["enc2.conv1"].cpu(), sd["model.enc2.conv1.weight"][:, :, 0].half())
    # a few more steps on the same batch: the L1 loss must go down
    tr2 = PointTrainer(model.model, lr=2e-3)
    losses = [tr2.train_step(x_t.cuda(), t.cuda(), noise.cuda()).item() for _ in range(12)]
    assert all(np.isfinite(losses)) and losses[-1] < 0.8 * losses[0], losses
    model.eval()
    out = model.sample(2, 128, num_steps=3)
    assert torch.isfinite(out).all()


def test_groupnorm_f32_kernels_against_torch():
    L, lib, st = _lib()
    g = torch.Generator(device="cuda").manual_seed(2)
    for rows, c in ((16, 128), (5, 4096), (32, 1024)):
        x = torch.randn(rows, c, device="cuda", generator=g) * 2 + 1
        gam, bet = torch.rand(c, device="cuda", generator=g) + 0.5, torch.randn(c, device="cuda", generator=g) * 0.3
        y, mean, rstd = torch.empty_like(x), torch.empty(rows, 8, device="cuda"), torch.empty(rows, 8, device="cuda")
        L.check(lib.pcd_groupnorm_f32(x.data_ptr(), rows, c, 8, gam.data_ptr(), bet.data_ptr(), 1e-5, 1, y.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), st))
        xr, gr, br = x.clone().requires_grad_(True), gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
        yr = F.relu(F.group_norm(xr, 8, gr, br, 1e-5))
        assert torch.allclose(y, yr.detach(), rtol=1e-5, atol=1e-5)
        dy = torch.randn(rows, c, device="cuda", generator=g)
        yr.backward(dy)
        dx, dg, db = torch.empty_like(x), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        L.check(lib.pcd_groupnorm_backward_f32(dy.data_ptr(), x.data_ptr(), rows, c, 8, gam.data_ptr(), bet.data_ptr(), mean.data_ptr(),
                                               rstd.data_ptr(), 1, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), st))
        assert rel_l2(dx, xr.grad) < 1e-5 and rel_l2(dg, gr.grad) < 1e-5 and rel_l2(db, br.grad) < 1e-5
    m = (torch.rand(300, device="cuda", generator=g) > 0.1).float()
    v, o = torch.randn(300, device="cuda", generator=g), torch.empty(300, device="cuda")
    L.check(lib.pcd_mask_scale_f32(v.data_ptr(), m.data_ptr(), 1 / 0.9, 300, o.data_ptr(), st))
    assert torch.equal(o, v * m * (1 / 0.9))
    L.check(lib.pcd_relu_f32(v.data_ptr(), 300, o.data_ptr(), st))
    assert torch.equal(o, v.clamp_min(0))
    L.check(lib.pcd_relu_backward_f32(v.data_ptr(), m.data_ptr(), 300, o.data_ptr(), st))
    assert torch.equal(o, m * (v > 0))


def test_latent_training_step_against_oracle(golden):
    """LatentTrainer (all fp32, per-sample GroupNorm: well conditioned) against the oracle's autograd on the golden
    batch: prediction, loss and EVERY parameter gradient tight, then AdamW, then the loss going down."""
    from helpers import latent_sd
    from shapegen_amd.diffusion import LatentDiffusion
    from shapegen_amd.training import LatentTrainer
    from shapegen_amd.vae import VAE3DLarge
    g = golden("train_latent.npz")
    sd = latent_sd()
    m = LatentDiffusion(VAE3DLarge())
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda")
    z_t, t, noise, mask = (torch.from_numpy(g[k]) for k in ("z_t", "t", "noise", "mask"))
    tr = LatentTrainer(m.model, lr=1e-4)
    pred = tr.forward(z_t.cuda(), t.cuda(), mask.cuda())
    loss = tr.backward(noise.cuda())
    msd = {k: v for k, v in sd.items() if k.startswith("model.")}
    loss_ref, pred_ref, grads_ref = O.latent_training_step(msd, "model.", z_t, t, noise, mask)
    assert rel_l2(pred.cpu(), pred_ref) < 1e-5 and abs(loss.item() - loss_ref.item()) < 1e-6
    assert np.abs(pred.cpu().numpy() - g["pred"]).max() < 1e-4
    grads = tr.grads()
    for k, gr in grads_ref.items():
        mine = grads[k[len("model."):]].cpu()
        # sign(pred - noise) may flip where |pred - noise| ~ 1e-6; none of the 1024 elements is that close here
        assert rel_l2(mine, gr) < 2e-4, (k, rel_l2(mine, gr))
    params = {k[len("model."):]: v.clone() for k, v in msd.items()}
    tr.optimizer_step()
    # (the optimizer kernel is checked on the HIP gradients: the first Adam step is lr * g / (|g| + eps), which turns a
    # 1e-4 relative difference of a ~1e-8 gradient element into a visible difference of the update)
    O.adamw_step(params, {k: v.cpu() for k, v in grads.items()}, {}, lr=1e-4, weight_decay=1e-5)
    for k, v in m.model.named_parameters():
        assert torch.allclose(v.detach().cpu(), params[k], rtol=0, atol=2e-6), k
    assert not any(p.requires_grad for p in m.vae.parameters())
    # the reference's training_step surface: frozen VAE encode -> reparameterize -> loss; loss decreases on a fixed batch
    m.train()
    vox = (torch.rand(4, 1, 32, 32, 32, device="cuda") > 0.9).float()
    cfg = m.configure_optimizers(max_epochs=10)
    cfg["optimizer"].lr = 1e-3
    torch.manual_seed(0)
    losses = []
    for _ in range(15):
        torch.manual_seed(1)                                   # same t, noise and dropout draw every step
        losses.append(float(m.training_step(vox)))
        cfg["optimizer"].step()
    assert np.isfinite(losses).all() and losses[-1] < 0.9 * losses[0], losses
    cfg["lr_scheduler"].step()
    assert cfg["optimizer"].lr < 1e-3
    m.eval()
    clouds = m.sample(num_samples=2, num_steps=3)
    assert len(clouds) == 2


def _im2col(L, lib, st, x_cl, b, cin, din, dout, k, s, p, tr, kp):
    col = torch.empty(b * dout ** 3, kp, dtype=torch.float16, device="cuda")
    L.check(lib.pcd_im2col_f16(x_cl.data_ptr(), b, cin, din, din, din, dout, dout, dout, k, s, p, tr, kp, col.data_ptr(), st))
    return col


def test_im2col_col2im_against_torch_convs():
    """Conv3d / ConvTranspose3d as gather + product, for every geometry VAE3DLarge uses (networks.py:2225-2264), and
    col2im as the exact adjoint of im2col (that is what backward-data needs)."""
    L, lib, st = _lib()
    g = torch.Generator(device="cuda").manual_seed(4)
    cases = [(0, 3, 1, 1, 8, 8, 1, 16), (0, 3, 1, 1, 8, 8, 16, 8), (0, 4, 2, 1, 8, 4, 8, 16), (0, 4, 1, 0, 4, 1, 16, 8),
             (0, 1, 1, 0, 8, 8, 8, 16), (1, 4, 2, 1, 4, 8, 16, 8)]
    for tr, k, s, p, din, dout, cin, cout in cases:
        b = 2
        x = torch.randint(-3, 4, (b, cin, din, din, din), device="cuda", generator=g).float()
        w = (torch.randint(-2, 3, (cin, cout, k, k, k) if tr else (cout, cin, k, k, k), device="cuda", generator=g)).float()
        want = F.conv_transpose3d(x, w, stride=s, padding=p) if tr else F.conv3d(x, w, stride=s, padding=p)
        assert want.shape[-1] == dout
        x_cl = x.permute(0, 2, 3, 4, 1).reshape(-1, cin).half().contiguous()
        kk = k ** 3 * cin
        kp = (kk + 63) // 64 * 64
        col = _im2col(L, lib, st, x_cl, b, cin, din, dout, k, s, p, tr, kp)
        assert bool((col[:, kk:] == 0).all())
        wm = (w.permute(1, 2, 3, 4, 0) if tr else w.permute(0, 2, 3, 4, 1)).reshape(cout, kk)      # [cout][tap][cin]
        got = col[:, :kk].float() @ wm.t()
        assert torch.equal(got, want.permute(0, 2, 3, 4, 1).reshape(-1, cout)), (tr, k, s, p)       # small integers: exact
        # adjoint: <im2col(x), y> == <x, col2im(y)>
        y = torch.randint(-2, 3, (b * dout ** 3, kp), device="cuda", generator=g).half()
        y[:, kk:] = 0
        dx = torch.empty(b * din ** 3, cin, dtype=torch.float16, device="cuda")
        L.check(lib.pcd_col2im_f16(y.data_ptr(), b, cin, din, din, din, dout, dout, dout, k, s, p, tr, kp, dx.data_ptr(), st))
        lhs = (col.double() * y.double()).sum()
        rhs = (x_cl.double() * dx.double()).sum()
        assert lhs == rhs, (tr, k, s, p, float(lhs), float(rhs))
    # residual tail and fused sigmoid + BCE
    a, bb = torch.randn(1000, device="cuda", generator=g).half(), torch.randn(1000, device="cuda", generator=g).half()
    o = torch.empty_like(a)
    L.check(lib.pcd_add_relu_f16(a.data_ptr(), bb.data_ptr(), 1000, 1, o.data_ptr(), st))
    assert torch.equal(o, (a.float() + bb.float()).clamp_min(0).half())
    d = torch.empty_like(a)
    L.check(lib.pcd_relu_mask_f16(bb.data_ptr(), o.data_ptr(), 1000, d.data_ptr(), st))
    assert torch.equal(d, torch.where(o > 0, bb, torch.zeros_like(bb)))
    logit = (torch.randn(777, 8, device="cuda", generator=g) * 4).half()
    tgt = (torch.rand(777, device="cuda", generator=g) > 0.7).float()
    ls, rec, dl = torch.empty(1, device="cuda"), torch.empty(777, device="cuda"), torch.zeros(777, 8, dtype=torch.float16, device="cuda")
    L.check(lib.pcd_sigmoid_bce(logit.data_ptr(), 8, tgt.data_ptr(), 777, 64.0, ls.data_ptr(), rec.data_ptr(), dl.data_ptr(), st))
    z = logit[:, 0].float().clone().requires_grad_(True)
    r = torch.sigmoid(z)
    loss = F.binary_cross_entropy(r, tgt)
    loss.backward()
    assert abs(ls.item() / 777 - loss.item()) < 1e-5 and torch.allclose(rec, r.detach(), atol=1e-6)
    assert rel_l2(dl[:, 0].float() / 64.0, z.grad) < 2e-3


# ------------------------------------------------------------------ the VAE step's small kernels, each against CPU torch
def test_bias_act_f16_kernel():
    """out = half_sat(float(x) + bias[col]) [ReLU]: one fp32 add and one rounding, so the result is exact."""
    L, lib, st = _lib()
    g = torch.Generator().manual_seed(11)
    rows = 37                                            # 37 * c is no multiple of the 256-thread block for any c below
    for c in (1, 32, 64, 200):
        for relu in (0, 1):
            x = (torch.randn(rows, c, generator=g) * 3).half()
            bias = torch.randn(c, generator=g) + torch.arange(c) * 0.25          # distinct per column: bias[i % c]
            x[0, 0], x[rows - 1, c - 1] = 65504.0, -65504.0                         # the sum leaves fp16's range: saturates
            if c > 1:
                bias[c - 1] = -100.0 - bias[c - 1].abs()
            bias[0] = 100.0 + bias[0].abs()
            out = torch.full((rows, c), float("nan"), dtype=torch.float16, device="cuda")
            xd, bd = x.cuda(), bias.cuda()
            L.check(lib.pcd_bias_act_f16(xd.data_ptr(), bd.data_ptr(), rows, c, relu, out.data_ptr(), st))
            want = x.float() + bias                                                 # fp32, as the kernel adds
            assert want[0, 0] > 65504.0
            if relu:
                want = want.clamp_min(0)
            want = want.clamp(-65504.0, 65504.0).half()
            assert torch.equal(out.cpu(), want), (c, relu)
            assert out[0, 0].item() == 65504.0 and (relu or c == 1 or out[rows - 1, c - 1].item() == -65504.0)
            # and the fp32 add loses nothing that matters: within half an fp16 ulp of the float64 sum
            w64 = x.double() + bias.double()
            w64 = (w64.clamp_min(0) if relu else w64).clamp(-65504.0, 65504.0)
            assert ((out.cpu().double() - w64).abs() <= w64.abs().clamp_min(2.0 ** -14) * 2.0 ** -11 * 1.001).all()


def _latent_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(n, generator=g) * 2
    lv = torch.linspace(-20, 10, n)[torch.randperm(n, generator=g)].float()
    eps, dz = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.3
    return mu, lv, eps, dz


def test_reparameterize_and_latent_backward_kernels():
    """z = mu + eps exp(logvar / 2); the gradients of <z, dz> + kl_scale * KL by float64 autograd; the KL sum.  The
    vectors are fp32 results of a few operations and one expf (a few ulp): 2e-6 rel-L2; kl_sum is an fp32 atomic sum
    of n terms: 1e-5 relative.  MI355X: z 4.3e-8, dmu 4.4e-8, dlogvar 5.6e-8, kl_sum 1.1e-8 (the worse of the two n);
    the element-wise rtol 1e-5 / atol 1e-6 (terms of order 1, a few fp32 roundings each) is an allclose and has no figure."""
    L, lib, st = _lib()
    for n, seed in ((2 * 256, 5), (777, 6)):
        mu, lv, eps, dz = _latent_inputs(n, seed)
        d = [t.cuda() for t in (mu, lv, eps, dz)]
        z = torch.full((n,), float("nan"), device="cuda")
        L.check(lib.pcd_reparameterize(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), z.data_ptr(), n, st))
        mu64, lv64 = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
        z64 = mu64 + eps.double() * torch.exp(lv64 / 2)
        print(f"n {n}: z {rel_l2(z.cpu(), z64.detach()):.2e}")
        assert rel_l2(z.cpu(), z64.detach()) < 2e-6
        kl_scale = 0.37 * 1024.0
        kl_terms = 1 + lv64 - mu64 ** 2 - torch.exp(lv64)
        ((z64 * dz.double()).sum() + kl_scale * (-0.5 * kl_terms.mean())).backward()
        dmu, dlv = torch.full((n,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        kl_sum = torch.full((1,), float("nan"), device="cuda")
        L.check(lib.pcd_vae_latent_backward(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, kl_scale,
                                            dmu.data_ptr(), dlv.data_ptr(), kl_sum.data_ptr(), st))
        print(f"n {n}: dmu {rel_l2(dmu.cpu(), mu64.grad):.2e} dlogvar {rel_l2(dlv.cpu(), lv64.grad):.2e} "
              f"kl_sum {abs(kl_sum.item() - kl_terms.sum().item()) / abs(kl_terms.sum().item()):.2e}")
        assert rel_l2(dmu.cpu(), mu64.grad) < 2e-6, rel_l2(dmu.cpu(), mu64.grad)
        assert rel_l2(dlv.cpu(), lv64.grad) < 2e-6, rel_l2(dlv.cpu(), lv64.grad)
        # element-wise too: the large exp(logvar) terms must not hide the small ones
        assert torch.allclose(dlv.cpu().double(), lv64.grad, rtol=1e-5, atol=1e-6)
        assert torch.allclose(dmu.cpu().double(), mu64.grad, rtol=1e-5, atol=1e-6)
        want = kl_terms.sum().item()
        assert abs(kl_sum.item() - want) < 1e-5 * abs(want), (kl_sum.item(), want)
        # the call VAE3DLarge.calculate_loss makes in eval mode: zero eps / dz (one tensor), scale 0, both outputs aliased
        zero, scratch = torch.zeros(n, device="cuda"), torch.empty(n, device="cuda")
        out = torch.full((2,), float("nan"), device="cuda")
        L.check(lib.pcd_vae_latent_backward(d[0].data_ptr(), d[1].data_ptr(), zero.data_ptr(), zero.data_ptr(), n, 0.0,
                                            scratch.data_ptr(), scratch.data_ptr(), out[1:].data_ptr(), st))
        assert abs(out[1].item() - want) < 1e-5 * abs(want) and torch.isnan(out[0])
        assert torch.equal(d[0].cpu(), mu) and torch.equal(d[1].cpu(), lv) and not zero.any()


def test_f16_to_f32_kernel_is_exact():
    """Every fp16 bit pattern that is not a NaN (subnormals, +-0, +-65504, +-inf): 63490 elements, 2 past a block."""
    L, lib, st = _lib()
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    h = bits.view(torch.float16)
    h = h[~torch.isnan(h)]
    n = h.numel()
    assert n == 63490 and n % 256 == 2 and (h == 65504).any() and (h == -65504).any() and (h.abs() == 2.0 ** -24).sum() == 2
    src = h.cuda()
    dst = torch.full((n + 8,), 7.0, device="cuda")
    L.check(lib.pcd_f16_to_f32(src.data_ptr(), dst.data_ptr(), n, st))
    got = dst.cpu()
    assert torch.equal(got[:n].view(torch.int32), h.float().view(torch.int32))          # bitwise: the sign of zero too
    assert bool((got[n:] == 7.0).all())
    for m in (1, 255, 257):
        dst.fill_(7.0)
        L.check(lib.pcd_f16_to_f32(src.data_ptr(), dst.data_ptr(), m, st))
        assert torch.equal(dst.cpu()[:m], h.float()[:m]) and bool((dst[m:] == 7.0).all())


def test_sigmoid_bce_kernel_strided_grid_stride():
    """The trainer's call shape: logits in column 0 of an [n][64] fp16 matrix, n = 600000 > 2048 blocks * 256 threads,
    so the grid-stride loop runs.  The loss reference is float32 on the CPU (the reference project's arithmetic):
    for a logit z > 16.64 float32 gives 1 + exp(-z) == 1, sigmoid == 1 and log(1 - sigmoid) = -inf, clamped to -100 by
    torch's BCE, so a target 0 there costs exactly 100 (float64 would say z).  Those elements (z >= 18, target 0) are
    also run on their own, where the sum is exact.  On the negative side nothing saturates (sigmoid(-30) = 9.4e-14)."""
    L, lib, st = _lib()
    g = torch.Generator().manual_seed(13)
    n, ld, scale = 600000, 64, 32768.0
    z = torch.randn(n, generator=g) * 4
    z[:4000] = torch.linspace(18, 30, 4000)
    z[4000:8000] = torch.linspace(-30, -18, 4000)
    z[(z > 16.0) & (z < 18.0)] = 16.0          # keep the full run off the band where 1 + exp(-z) rounds to 1 (z ~ 16.64): one
    #                                            logit judged differently by expf and the CPU would move a term from ~17 to 100
    z = z[torch.randperm(n, generator=g)].half()
    x = (torch.rand(n, generator=g) > 0.7).float()
    logit = (torch.randn(n, ld, generator=g) * 4).half()              # columns 1.. hold other numbers: must not be read
    logit[:, 0] = z
    dl0 = torch.randn(n, ld, generator=g).half()
    sat = (z.float() >= 18) & (x == 0)
    assert z.float().max() == 30 and z.float().min() == -30 and 500 < int(sat.sum()) < 160000

    def run(zm, xt, dl):
        ls, rec = torch.full((1,), float("nan"), device="cuda"), torch.full((xt.numel(),), float("nan"), device="cuda")
        L.check(lib.pcd_sigmoid_bce(zm.data_ptr(), ld, xt.data_ptr(), xt.numel(), scale, ls.data_ptr(), rec.data_ptr(), dl.data_ptr(), st))
        return ls.item(), rec.cpu()

    dl = dl0.cuda()
    ls, rec = run(logit.cuda(), x.cuda(), dl)
    assert torch.allclose(rec.double(), torch.sigmoid(z.double()), rtol=0, atol=1e-6)
    r32 = torch.sigmoid(z.float())
    per = F.binary_cross_entropy(r32, x, reduction="none")
    assert bool((per[sat] == 100.0).all())                                 # the regime the docstring describes
    want = per.double().sum().item()
    assert abs(ls - want) < 1e-5 * want, (ls, want)
    dl = dl.cpu()
    assert torch.equal(dl[:, 1:], dl0[:, 1:])                              # only column 0 is written
    want_d = scale * (torch.sigmoid(z.double()) - x.double()) / n
    assert rel_l2(dl[:, 0], want_d) < 2e-3
    # the clamp regime alone: every term is exactly 100, and sums of those are exact in fp32
    ns = int(sat.sum())
    ls_sat, rec_sat = run(logit[sat].contiguous().cuda(), x[sat].contiguous().cuda(), torch.zeros(ns, ld, dtype=torch.float16, device="cuda"))
    assert ls_sat == 100.0 * ns and bool((rec_sat == 1.0).all())
    # and the rest against float64, where float32's sigmoid is accurate
    rest = z.float().abs() < 8
    nr = int(rest.sum())
    ls_r, _ = run(logit[rest].contiguous().cuda(), x[rest].contiguous().cuda(), torch.zeros(nr, ld, dtype=torch.float16, device="cuda"))
    want_r = F.binary_cross_entropy(torch.sigmoid(z[rest].double()), x[rest].double(), reduction="sum").item()
    assert abs(ls_r - want_r) < 1e-5 * want_r, (ls_r, want_r)



def test_point_and_latent_trainers_across_a_batch_size_change(golden):
    """One trainer stepped at the golden batch and then at half of it, and one stepped twice at the half, against a
    fresh trainer at the half: nothing an earlier step left in the workspace may reach a later one.  Gradients bitwise,
    except the three that `pcd_vec3_outer` still adds atomically per block (1e-6 rel-L2, their norms are ~1e2); the
    atomically summed loss at 1e-6 relative.  (The VAE trainer's version is in test_gpu_train_vae.py.)"""
    from helpers import latent_sd
    from shapegen_amd.diffusion import LatentDiffusion
    from shapegen_amd.training import LatentTrainer, PointTrainer
    from shapegen_amd.vae import VAE3DLarge
    atomic = ("output.3.weight", "output.3.bias", "enc1.conv1.weight")

    def point(sizes):
        model, sd, x_t, t, noise, g = _setup(golden)
        tr = PointTrainer(model.model)
        for b in sizes:
            tr.forward(x_t[:b].cuda(), t[:b].cuda(), update_stats=False)
            loss = tr.backward(noise[:b].cuda())
        return loss.item(), {k: v.clone() for k, v in tr.g.items()}

    def latent(sizes):
        g = golden("train_latent.npz")
        m = LatentDiffusion(VAE3DLarge())
        m.load_state_dict(latent_sd(), strict=True)
        m = m.to("cuda")
        z_t, t, noise, mask = (torch.from_numpy(g[k]) for k in ("z_t", "t", "noise", "mask"))
        tr = LatentTrainer(m.model)
        for b in sizes:
            tr.forward(z_t[:b].cuda(), t[:b].cuda(), mask[:b].cuda())
            loss = tr.backward(noise[:b].cuda())
        return loss.item(), {k: v.clone() for k, v in tr.g.items()}

    for step, full, half in ((point, 2, 1), (latent, 4, 2)):
        loss_ref, grads_ref = step((half,))
        for sizes in ((full, half), (half, half)):
            loss, grads = step(sizes)
            assert abs(loss - loss_ref) <= 1e-6 * abs(loss_ref), (step.__name__, sizes, loss, loss_ref)
            assert sorted(grads) == sorted(grads_ref)
            for k, v in grads_ref.items():
                if step is point and k in atomic:
                    assert v.norm() > 1 and rel_l2(grads[k], v) < 1e-6, (sizes, k, rel_l2(grads[k], v))
                else:
                    assert torch.equal(grads[k], v), (step.__name__, sizes, k, rel_l2(grads[k], v))
