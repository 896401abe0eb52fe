"""Class-conditional latent diffusion on the device: the hoisted class bias, the guided samplers on the per-layer launches and
inside the persistent launch (csrc/latent_persist.hip, paired rows), the labelled latent trainer and the entry scripts, against
the float statement tests/latent_cfg_statement.py.  Weights: helpers.latent_sd(); class table: torch.randn(K + 1, 256) from a
fixed seed, K = 3.  Bounds are the project's own for the same paths without classes (cited where they are used)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import latent_cfg_statement as S
import resume_runs as R
from helpers import counted_replays, latent_sd, rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
K, NULL = 3, 3
B, T = 3, 8
LABELS = (0, 2, NULL)
SCALES = {"one": 2.0, "per_shape": (1.0, 2.0, 3.5)}
# fp16: test_latent_ddim's bound; fp32 mode: DESIGN section 4 (rel-L2 5e-5, max-abs 1e-3 * max(1, max|x| / 100))
TOL = {"fp16": {"rel": 5e-3, "maxabs": None}, "fp32": {"rel": 5e-5, "maxabs": 1e-3}}


def class_table():
    return torch.randn(K + 1, 256, generator=torch.Generator().manual_seed(31))


def class_sd():
    sd = latent_sd()
    sd["model.class_emb.weight"] = class_table()
    return sd


def model_sd():
    return {k: v for k, v in latent_sd().items() if k.startswith("model.")}


_MODELS = {}


def model_of(prec="fp16"):
    """The class-conditional latent model in one precision (built once per module run)."""
    if prec not in _MODELS:
        from shapegen_amd.diffusion import ConditionalLatentDiffusion
        from shapegen_amd.vae import VAE3DLarge
        m = ConditionalLatentDiffusion(VAE3DLarge(), K)
        m.load_state_dict(class_sd(), strict=True)
        m.model.set_precision(prec)
        _MODELS[prec] = m.to(DEV).eval()
    return _MODELS[prec]


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _MODELS.clear()


def per_layer(m):
    """Context: the module samples on the per-layer launches."""
    import contextlib

    @contextlib.contextmanager
    def ctx():
        m.use_persistent = False
        try:
            yield
        finally:
            del m.use_persistent
    return ctx()


def inputs(b=B):
    g = torch.Generator().manual_seed(17)
    return torch.randn(b, 256, generator=g), [torch.randn(b, 256, generator=g) for _ in range(T)]


def run_sampler(m, kind, scale, z_T, noises, labels=LABELS):
    kw = dict(labels=torch.tensor(labels), guidance_scale=scale if isinstance(scale, float) else torch.tensor(scale), return_latent=True)
    b = z_T.shape[0]
    if kind == "ddim":
        return m.sample(b, num_steps=T, z_T=z_T.to(DEV), **kw)[1]
    if kind == "ddpm":
        return m.sample2(b, num_steps=T, z_T=z_T.to(DEV), noises=noises, **kw)[1]
    if kind == "state":
        return m.sample3(b, z=z_T.to(DEV), start_t=torch.ones(b) * 0.4, num_steps=9, **kw)[1]
    return m.sample_dpm(b, num_steps=12, z_T=z_T.to(DEV), **kw)[1]


_REF = {}


def reference(kind, scale_key):
    """The statement's result for (kind, scale), computed once and shared."""
    if (kind, scale_key) not in _REF:
        z_T, noises = inputs()
        steps = {"ddim": T, "ddpm": T, "state": 9, "dpm": 12}[kind]
        _REF[kind, scale_key] = S.sample(kind, model_sd(), "model.", class_table(), LABELS, SCALES[scale_key], z_T, steps, noises=noises,
                                         start_t=torch.ones(B) * 0.4)
    return _REF[kind, scale_key]


# ------------------------------------------------------------------ 1. the hoisted class bias and the module forward
def test_class_bias_goes_through_the_packed_time_columns():
    from shapegen_amd import packing
    _, _, ex = packing.pack_latent_unet(latent_sd(), "model.")
    want = class_table().double().numpy() @ np.asarray(ex["e1w_t"], dtype=np.float64).T
    for prec in ("fp16", "fp32"):
        cb = model_of(prec).model.class_bias()
        assert cb.shape == (K + 1, 128) and cb.dtype == torch.float32 and rel_l2(cb.cpu(), want) < 1e-6
        assert model_of(prec).model.class_bias() is cb
    m = model_of("fp16")
    try:
        with torch.no_grad():
            m.model.class_emb.weight[1] += 1.0
        m.model.invalidate()
        cb2 = m.model.class_bias()
        assert not torch.equal(cb2[1], cb[1]) and rel_l2(cb2[0].cpu(), want[0]) < 1e-6
    finally:
        m.load_state_dict(class_sd(), strict=True)                               # loading invalidates too
    assert rel_l2(m.model.class_bias().cpu(), want) < 1e-6
    # the module's own forward adds the same rows
    g = torch.Generator().manual_seed(4)
    z, t = torch.randn(B, 256, generator=g), torch.tensor([0.2, 0.5, 0.9])
    ref = S.eps_of(model_sd(), "model.", class_table(), LABELS, z, t)
    f32 = model_of("fp32").model
    got = f32(z.to(DEV), t.to(DEV), torch.tensor(LABELS))
    print(f"module forward with labels [fp32]: rel-L2 {rel_l2(got.cpu(), ref):.3e}")
    assert rel_l2(got.cpu(), ref) < 1e-4                                         # the fp32 mode's eps bound (networks._Denoiser)
    none, null = f32(z.to(DEV), t.to(DEV)), f32(z.to(DEV), t.to(DEV), torch.tensor([NULL] * B))
    assert torch.equal(none, null) and torch.equal(none[2], got[2]) and not torch.equal(none[0], got[0])
    from shapegen_amd.networks import SimpleLatentUNetPointNet
    with pytest.raises(ValueError, match="without classes"):
        SimpleLatentUNetPointNet(256).to(DEV)(z.to(DEV), t.to(DEV), torch.tensor(LABELS))


# ------------------------------------------------------------------ 2. per-layer samplers against the statement
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("scale_key", ["one", "per_shape"])
@pytest.mark.parametrize("kind", ["ddim", "ddpm", "dpm", "state"])
def test_guided_samplers_against_the_statement(kind, scale_key, prec):
    """B = 3, labels (0, 2, null), scale 2.0 and per-shape scales (1.0, 2.0, 3.5): DDIM and DDPM (injected noises) at T = 8,
    sample_dpm at 12 steps, sample3 from t = 0.4 over 9 steps, all on the per-layer launches.  Figures (one MI355X), printed
    before the assertions: see DESIGN section 4."""
    z_T, noises = inputs()
    want = reference(kind, scale_key)
    assert torch.isfinite(want).all()
    m = model_of(prec)
    with per_layer(m):
        got = run_sampler(m, kind, SCALES[scale_key], z_T, noises).cpu()
    tol = TOL[prec]
    r, mx = rel_l2(got, want), float((got - want).abs().max())
    print(f"latent cfg {kind} scale {scale_key} [{prec}]: rel-L2 {r:.3e}  max-abs {mx:.3e}  max|x| {float(want.abs().max()):.3g}")
    assert r <= tol["rel"], (kind, scale_key, prec, r)
    if tol["maxabs"] is not None:
        assert mx <= tol["maxabs"] * max(1.0, float(want.abs().max()) / 100.0), (kind, scale_key, prec, mx)


def test_scale_one_runs_one_forward_and_is_the_conditional_run():
    m = model_of("fp16")
    z_T, noises = inputs()
    calls, inner = [], m.model.forward_with_bias
    m.model.forward_with_bias = lambda x, tb, stride, out=None: (calls.append(stride), inner(x, tb, stride, out=out))[1]
    try:
        with per_layer(m):
            one = run_sampler(m, "ddim", 1.0, z_T, noises)
            assert calls == [1] * T                                              # no second forward
            del calls[:]
            ones = run_sampler(m, "ddim", (1.0, 1.0, 1.0), z_T, noises)
            assert calls == [1] * T
            del calls[:]
            two = run_sampler(m, "ddim", 2.0, z_T, noises)
            assert calls == [1, 0] * T
    finally:
        del m.model.forward_with_bias
    assert torch.equal(one, ones) and not torch.equal(one, two)
    want = S.sample("ddim", model_sd(), "model.", class_table(), LABELS, 1.0, z_T, T)
    assert rel_l2(one.cpu(), want) <= TOL["fp16"]["rel"]
    with per_layer(m):                                                           # labels=None on a class model is the null class
        a = m.sample(B, num_steps=T, z_T=z_T.to(DEV), return_latent=True)[1]
        b = m.sample(B, num_steps=T, z_T=z_T.to(DEV), labels=[NULL] * B, return_latent=True)[1]
    assert torch.equal(a, b)


def test_graph_replay_equals_eager_stepping():
    """(2 shapes, 20 steps) on the per-layer launches: one eager step, two graphs of 8, the rest eager."""
    m = model_of("fp16")
    z_T = torch.randn(2, 256, generator=torch.Generator().manual_seed(13)).to(DEV)
    outs = []
    with per_layer(m):
        for graphs in (True, False):
            with counted_replays(m, graphs) as seen:
                outs.append(m.sample(2, num_steps=20, z_T=z_T, labels=[1, NULL], guidance_scale=torch.tensor([2.0, 1.5]), return_latent=True)[1])
                assert len(seen) == (2 if graphs else 0)
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    meshes = m.sample_dpm(2, num_steps=12, z_T=z_T, labels=[1, NULL], guidance_scale=2.0, output="mesh")        # the surfaces leave as before
    assert len(meshes) == 2 and all(torch.isfinite(mesh.vertices).all() for mesh in meshes)


# ------------------------------------------------------------------ 3. the persistent launch, forward mode
def _persist_labels(b, g):
    """(raw int32 labels with a null and an out-of-range value where the batch has room, what they mean)."""
    raw = torch.randint(0, K, (b,), generator=g, dtype=torch.int32)
    if b > 1:
        raw[b // 2] = NULL
    if b > 2:
        raw[1] = 7                                                               # outside [0, class_rows): reads the null row
    if b > 3:
        raw[b - 1] = -2
    meant = torch.where((raw < 0) | (raw > K), torch.full_like(raw, NULL), raw)
    return raw, meant


def _per_layer_eps(m, z, tb_row, meant, w):
    """The guided eps on the per-layer launches: the Stepper's select, two forwards and combine, with torch's fp32 elementwise ops."""
    cb = m.model.class_bias()
    ec = m.model.forward_with_bias(z, (tb_row[None, :] + cb[meant.to(DEV).long()]).contiguous(), 1)
    if w is None:
        return ec
    eu = m.model.forward_with_bias(z, (tb_row + cb[NULL]).contiguous(), 0)
    return eu + w.to(DEV).expand(z.shape[0])[:, None] * (ec - eu)


@pytest.mark.parametrize("b,guided", [(1, True), (16, True), (17, True), (32, True), (5, False), (33, False), (64, False)])
def test_persistent_forward_guided(b, guided):
    """One launch against the per-layer guided eps (<= 2e-3) and the statement (<= 3e-3), test_latent_persistent_forward's bounds;
    rows of a null label at scale 1 are bitwise the unguided launch's over the same bias row; a second launch is bitwise the first."""
    m = model_of("fp16")
    if not m.model.persist_supported(32):
        pytest.skip("needs a 256-CU device")
    g = torch.Generator().manual_seed(100 + b)
    z = (torch.randn(b, 256, generator=g) * 1.2).to(DEV)
    tval = 0.1 + 0.8 * float(torch.rand(1, generator=g))
    raw, meant = _persist_labels(b, g)
    w = None
    if guided:
        w = 1.0 + 2.5 * torch.rand(b, generator=g)
        w[meant == NULL] = 1.0
        w[0] = 3.5 if b > 1 else 2.0
    tb = m.model.time_bias(torch.full((1,), tval).to(DEV))[0]
    eps = m.model.forward_persist_guided(z, tb, raw.to(DEV), None if w is None else w.to(DEV))
    m.model.check_persist_status()
    assert torch.isfinite(eps).all()
    want_layers = _per_layer_eps(m, z, tb, meant, w)
    want = S.guided_model(model_sd(), "model.", class_table(), meant.long(), 1.0 if w is None else w)(z.cpu(), torch.full((b,), tval))
    r1, r2 = rel_l2(eps.cpu(), want_layers.cpu()), rel_l2(eps.cpu(), want)
    print(f"persistent forward B = {b} {'guided' if guided else 'labelled'}: v. per-layer {r1:.3e}, v. statement {r2:.3e}")
    assert r1 <= 2e-3 and r2 <= 3e-3
    again = m.model.forward_persist_guided(z, tb, raw.to(DEV), None if w is None else w.to(DEV))
    assert torch.equal(again, eps)
    # null label (and scale 1): the unguided launch over the null bias row
    plain = m.model.forward_persist(z, (tb + m.model.class_bias()[NULL]).contiguous())
    m.model.check_persist_status()
    rows = meant == NULL
    assert int(rows.sum()) >= (1 if b > 1 else 0) and torch.equal(eps[rows.to(DEV)], plain[rows.to(DEV)])
    if b > 1:
        assert not torch.equal(eps[~rows.to(DEV)], plain[~rows.to(DEV)])
    if guided and b > 1:                                                         # one shared scale (stride 0) is the vector of that scale
        shared = m.model.forward_persist_guided(z, tb, raw.to(DEV), torch.full((1,), 2.0, device=DEV))
        each = m.model.forward_persist_guided(z, tb, raw.to(DEV), torch.full((b,), 2.0, device=DEV))
        assert torch.equal(shared, each)


# ------------------------------------------------------------------ 4. the persistent launch, DDIM
def _both_routes(m, b, steps, z_T, labels, scale, counted=None):
    """(persistent, per-layer) latents of one guided DDIM call; the persistent call must have stayed on its launch."""
    kw = dict(num_steps=steps, z_T=z_T, labels=labels, guidance_scale=scale, return_latent=True)
    keep = z_T.clone()
    m.use_persistent = True
    try:
        a = m.sample(b, **kw)[1]
        assert m.use_persistent and m.model.persist_status() == 0
        m.use_persistent = False
        want = m.sample(b, **kw)[1]
    finally:
        del m.use_persistent
    assert torch.equal(z_T, keep)                                                # the caller's z_T is untouched
    return a, want


@pytest.mark.parametrize("b,guided,bound", [(1, True, 2e-3), (16, True, 2e-3), (17, True, 2e-3), (32, True, 2e-3), (5, False, 2e-3),
                                            (33, False, 2e-3), (45, False, 2e-3), (64, False, 3e-3)])
def test_persistent_ddim_guided_20_steps(b, guided, bound):
    """20 steps in ONE launch against the per-layer guided run, the forward test's B set (33 labelled: the second stream carries one
    row) and B = 45; the bounds are test_latent_persistent_ddim_steps' at these shapes."""
    m = model_of("fp16")
    if not m.model.persist_supported(32):
        pytest.skip("needs a 256-CU device")
    g = torch.Generator().manual_seed(200 + b)
    z_T = torch.randn(b, 256, generator=g).to(DEV)
    labels = torch.randint(0, K + 1, (b,), generator=g)
    scale = (1.0 + 2.5 * torch.rand(b, generator=g)) if guided else 1.0
    launches, inner = [], m.model.ddim_steps_persist_guided
    m.model.ddim_steps_persist_guided = lambda *a: (launches.append(a[-1] is not None), inner(*a))[1]
    try:
        a, want = _both_routes(m, b, 20, z_T, labels, scale)
    finally:
        del m.model.ddim_steps_persist_guided
    assert launches == [guided]                                                  # one launch, with or without a scale
    r = rel_l2(a.cpu(), want.cpu())
    print(f"persistent DDIM, 20 steps, B = {b} {'guided' if guided else 'labelled'}: rel-L2 v. per-layer {r:.3e}")
    assert torch.isfinite(a).all() and r <= bound


def test_persistent_ddim_guided_long_runs_and_streams():
    """200 guided steps at B = 32 twice: bitwise equal (a stale exchange read would show); shapes 0..15 equal the B = 16 run bitwise (a
    stream does not depend on the other); 1000 steps against the per-layer launches <= 5e-3; sample3 guided at B = 5 <= 2e-3; the
    unlabelled LatentDiffusion on the same build still takes its launch and agrees with its per-layer run (<= 2e-3)."""
    m = model_of("fp16")
    if not m.model.persist_supported(32):
        pytest.skip("needs a 256-CU device")
    g = torch.Generator().manual_seed(12)
    z_T = torch.randn(32, 256, generator=g).to(DEV)
    labels = torch.randint(0, K + 1, (32,), generator=g)
    scale = 1.0 + 2.5 * torch.rand(32, generator=g)
    kw = dict(num_steps=200, return_latent=True)
    m.use_persistent = True
    try:
        a = m.sample(32, z_T=z_T, labels=labels, guidance_scale=scale, **kw)[1]
        assert m.model.persist_status() == 0
        b = m.sample(32, z_T=z_T, labels=labels, guidance_scale=scale, **kw)[1]
        assert m.model.persist_status() == 0
        half = m.sample(16, z_T=z_T[:16], labels=labels[:16], guidance_scale=scale[:16], **kw)[1]
        assert m.model.persist_status() == 0 and m.use_persistent
    finally:
        del m.use_persistent
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a[:16], half)
    a1000, want1000 = _both_routes(m, 32, 1000, z_T, labels, scale)
    r = rel_l2(a1000.cpu(), want1000.cpu())
    print(f"persistent guided DDIM, 1000 steps, B = 32: rel-L2 v. per-layer {r:.3e}")
    assert r <= 5e-3
    kw3 = dict(z=z_T[:5], start_t=torch.ones(5) * 0.4, num_steps=9, labels=labels[:5], guidance_scale=2.0, return_latent=True)
    m.use_persistent = True
    try:
        a5 = m.sample3(5, **kw3)[1]
        assert m.model.persist_status() == 0 and m.use_persistent
        m.use_persistent = False
        want5 = m.sample3(5, **kw3)[1]
    finally:
        del m.use_persistent
    print(f"persistent guided sample3, B = 5: rel-L2 v. per-layer {rel_l2(a5.cpu(), want5.cpu()):.3e}")
    assert rel_l2(a5.cpu(), want5.cpu()) <= 2e-3
    # more than 32 guided shapes: the per-layer launches
    launches, inner = [], m.model.ddim_steps_persist_guided
    m.model.ddim_steps_persist_guided = lambda *args: (launches.append(1), inner(*args))[1]
    try:
        z40 = torch.randn(40, 256, generator=g).to(DEV)
        out = m.sample(40, num_steps=4, z_T=z40, labels=torch.arange(40) % 4, guidance_scale=2.0, return_latent=True)[1]
    finally:
        del m.model.ddim_steps_persist_guided
    assert launches == [] and torch.isfinite(out).all()
    # the unlabelled model
    from shapegen_amd.diffusion import LatentDiffusion
    from shapegen_amd.vae import VAE3DLarge
    plain = LatentDiffusion(VAE3DLarge())
    plain.load_state_dict(latent_sd(), strict=True)
    plain = plain.to(DEV).eval()
    plain.use_persistent = True
    p = plain.sample(32, num_steps=20, z_T=z_T, return_latent=True)[1]
    assert plain.use_persistent and plain.model.persist_status() == 0
    plain.use_persistent = False
    w = plain.sample(32, num_steps=20, z_T=z_T, return_latent=True)[1]
    assert rel_l2(p.cpu(), w.cpu()) < 2e-3


# ------------------------------------------------------------------ 5. the trainer
TLABELS = (1, 0, 1, NULL)


@pytest.fixture
def autograd_on():
    with torch.enable_grad():
        yield


def fresh_train_model():
    from shapegen_amd.diffusion import ConditionalLatentDiffusion
    from shapegen_amd.vae import VAE3DLarge
    m = ConditionalLatentDiffusion(VAE3DLarge(), K)
    m.load_state_dict(class_sd(), strict=True)
    return m.to(DEV)


def test_training_step_against_the_statement(golden, autograd_on):
    """The golden latent batch (4 rows) with labels (1, 0, 1, null); bounds: test_latent_training_step_against_oracle's (prediction
    1e-5, loss 1e-6, every gradient rel-L2 < 2e-4)."""
    from shapegen_amd.training import LatentTrainer
    gd = golden("train_latent.npz")
    z_t, t, noise, mask = (torch.from_numpy(gd[k]) for k in ("z_t", "t", "noise", "mask"))
    E = class_table()
    loss_ref, pred_ref, grads_ref = S.training_step(model_sd(), "model.", E, TLABELS, z_t, t, noise, mask)
    m = fresh_train_model()
    tr = LatentTrainer(m.model, lr=1e-4)
    assert tr.names[-1] == "class_emb.weight" and tr.param_layout()[-1] == ("class_emb.weight", (K + 1) * 256)
    pred = tr.forward(z_t.to(DEV), t.to(DEV), mask.to(DEV), labels=torch.tensor(TLABELS))
    loss = tr.backward(noise.to(DEV))
    print(f"labelled latent step: prediction rel-L2 {rel_l2(pred.cpu(), pred_ref):.3e}, loss {loss.item():.7f} v. {loss_ref.item():.7f}")
    assert rel_l2(pred.cpu(), pred_ref) < 1e-5 and abs(loss.item() - loss_ref.item()) < 1e-6
    grads = tr.grads()
    assert set("model." + k for k in grads) == set(grads_ref)
    worst = max((rel_l2(grads[k[len("model."):]].cpu(), gr), k) for k, gr in grads_ref.items())
    print(f"worst gradient: {worst[1]} rel-L2 {worst[0]:.3e}; class_emb.weight {rel_l2(grads['class_emb.weight'].cpu(), grads_ref['model.class_emb.weight']):.3e}")
    for k, gr in grads_ref.items():
        assert rel_l2(grads[k[len("model."):]].cpu(), gr) < 2e-4, k
    assert bool((grads["class_emb.weight"][2] == 0).all())                       # class 2 has no shape in the batch
    # the table's gradient is bitwise the ordered segmented sum of the trainer's own d_te
    d_te = tr._ws["d.te"].cpu()
    want = torch.zeros(K + 1, 256)
    for i, c in enumerate(TLABELS):
        want[c] = want[c] + d_te[i]
    assert torch.equal(tr.g["class_emb.weight"].cpu(), want)
    # labels=None trains the null row alone; a model without classes refuses labels and is what it was
    tr.forward(z_t.to(DEV), t.to(DEV), mask.to(DEV))
    tr.backward(noise.to(DEV))
    gn = tr.g["class_emb.weight"]
    assert bool((gn[:K] == 0).all()) and float(gn[NULL].abs().max()) > 0
    from shapegen_amd.diffusion import LatentDiffusion
    from shapegen_amd.vae import VAE3DLarge
    plain = LatentDiffusion(VAE3DLarge()).to(DEV)
    ptr = LatentTrainer(plain.model)
    assert "class_emb.weight" not in ptr.names
    with pytest.raises(ValueError, match="without classes"):
        ptr.forward(z_t.to(DEV), t.to(DEV), mask.to(DEV), labels=torch.tensor(TLABELS))


def test_two_identical_steps_give_bitwise_equal_state(golden, autograd_on):
    gd = golden("train_latent.npz")
    z_t, t, noise, mask = (torch.from_numpy(gd[k]).to(DEV) for k in ("z_t", "t", "noise", "mask"))
    states = []
    for _ in range(2):
        m = fresh_train_model()
        tr = m.configure_optimizers()["optimizer"]
        tr.enable_ema(0.9)
        for _ in range(2):
            tr.train_step(z_t, t, noise, mask, labels=torch.tensor(TLABELS))
        states.append(R.snapshot(m))
    assert R.compare(states[0], states[1]) == {}
    assert not torch.equal(states[0]["sd.model.class_emb.weight"], class_table())      # AdamW moved the table with everything else


class LabelledBatches(R.Batches):
    """R.Batches whose items are (grids, labels)."""

    def __init__(self, x, labels, batch, train):
        super().__init__(x, batch, train)
        self.labels = labels

    def _pair(self, i):
        return self.x[i * self.batch:(i + 1) * self.batch], self.labels[i * self.batch:(i + 1) * self.batch]

    def train_dataloader(self):
        return (self._pair(i) for i in torch.randperm(self.train).tolist())

    def val_dataloader(self):
        return iter([self._pair(self.train)])


def labelled_make(kind):
    """R.make's latent run with classes: the same seeds and grids, labels i mod K, p_uncond 0.25."""
    import random
    from shapegen_amd.diffusion import ConditionalLatentDiffusion
    from shapegen_amd.vae import VAE3DLarge
    assert kind == "latent"
    torch.manual_seed(7)
    random.seed(7)
    np.random.seed(7)
    g = torch.Generator().manual_seed(11)
    model = ConditionalLatentDiffusion(VAE3DLarge(), K, p_uncond=0.25)
    return model.to(DEV), LabelledBatches(R._voxels(12, g), torch.arange(12) % K, 4, 2)


def test_resumed_labelled_run_is_the_uninterrupted_run(tmp_path, monkeypatch, autograd_on):
    """2 + 2 epochs with `save_last` and `ckpt_path` against 4 epochs in one go through tests/resume_runs.py, EMA on: parameters
    (class_emb among them), both moments and the EMA buffer bitwise; label dropout draws from the restored random stream."""
    from shapegen_amd.checkpoint import read_checkpoint
    from shapegen_amd.diffusion import ConditionalLatentDiffusion
    from shapegen_amd.vae import VAE3DLarge
    monkeypatch.setattr(R, "make", labelled_make)
    ma, ha, na = R.run("latent", ema_decay=0.9)
    sa = R.snapshot(ma)
    assert "ema" in sa and not torch.equal(sa["ema"], ma._trainer.P.cpu())
    m1, h1, n1 = R.run("latent", ema_decay=0.9, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True, max_steps=4)
    assert len(h1) == 2 and n1 == na[:4]
    del m1
    last = str(tmp_path / "run-last.ckpt")
    ck = read_checkpoint(last)
    assert ck["epoch"] == 1 and ck["global_step"] == 4
    assert ck["hyper_parameters"]["num_classes"] == K and ck["hyper_parameters"]["p_uncond"] == 0.25
    assert "model.class_emb.weight" in ck["state_dict"] and "model.class_emb.weight" in ck["ema_state_dict"]
    mc, hc, nc = R.run("latent", ckpt_path=last, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True)
    sc = R.snapshot(mc)
    print(f"labelled latent run resumed: differing tensors {R.compare(sa, sc)}, loss spread {R.loss_spread(ha, hc):.3e}")
    assert nc == na[4:] and [h[3] for h in hc] == [h[3] for h in ha]
    assert R.compare(sa, sc) == {}
    final = read_checkpoint(last)
    assert final["shapegen_amd"]["trainer"]["layout"][-1] == ("class_emb.weight", (K + 1) * 256)
    ema = ConditionalLatentDiffusion.load_from_checkpoint(last, vae=VAE3DLarge(), weights="ema")
    assert ema.num_classes == K
    assert torch.equal(ema.state_dict()["model.class_emb.weight"], mc._trainer.ema_state_dict()["class_emb.weight"].cpu())


# ------------------------------------------------------------------ 6. the entry scripts
def test_entry_scripts_class_conditional(tmp_path):
    """train_point_ldm.py --class-conditional for one VAE epoch and one diffusion epoch on synthetic shapes, then generate_mesh_ldm.py
    --label 1 --guidance 2 from its checkpoint, and once more on synthetic weights with --num-classes 3; fresh child processes, each
    under its own time limit."""
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(args):
        r = subprocess.run([sys.executable] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    run([os.path.join(ROOT, "train_point_ldm.py"), "--class-conditional", "--train-vae-epochs", "1", "--train-diffusion-epochs", "1",
         "--synthetic-shapes", "20", "--batch-size", "4", "--steps", "12", "--save-last", "--out", str(tmp_path / "t"),
         "--data-dir", str(tmp_path / "none")])
    assert os.path.isfile(tmp_path / "t" / "latent_diffusion_samples.npz")
    last = str(tmp_path / "checkpoints" / "point_ldm" / "latent_diffusion" / "latent_diffusion-last.ckpt")
    ck = torch.load(last, map_location="cpu", weights_only=False)
    assert ck["hyper_parameters"]["num_classes"] == 3 and tuple(ck["state_dict"]["model.class_emb.weight"].shape) == (4, 256)
    gen = [os.path.join(ROOT, "generate_mesh_ldm.py"), "--label", "1", "--guidance", "2", "--num-samples", "4", "--steps", "12"]
    for out, extra in (("g", ["--ldm-ckpt", last]), ("s", ["--num-classes", "3"])):
        run(gen + extra + ["--out", str(tmp_path / out)])
        files = sorted(glob.glob(str(tmp_path / out / "mesh_*.obj")))
        assert len(files) == 4
        for f in files:
            rows = [line.split() for line in open(f) if line.startswith("v ")]
            assert np.isfinite(np.array([[float(x) for x in row[1:4]] for row in rows], dtype=np.float64)).all()
        meta = json.load(open(tmp_path / out / "generation.json"))
        assert meta["label"] == 1 and meta["guidance"] == 2.0 and meta["num_classes"] == 3
