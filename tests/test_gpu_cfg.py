"""Class conditioning with classifier-free guidance on the GPU: the four new kernels against torch bit for bit, the guided
samplers against the float statement (tests/cfg_statement.py) over the CPU oracle network within the sampler bounds of DESIGN
section 4, the bitwise identities (scale 1 = one forward, graph replay = eager, shards = whole batch, known rows of `complete`),
one training step against the statement with tests/test_gpu_train.py's bounds, repeatability, resume, EMA, the entry scripts.

Shapes: K = 3 classes (table rows 0..2 and the null row 3); samplers B = 3, N = 128, labels (0, 2, null): 3 * 128 * 3 = 1152
elements span several blocks of the combine kernel in either form."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cfg_statement as S
import resume_runs as R
from helpers import counted_replays, point_sd, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"

K, NULL = 3, 3
B, N, T, T_DPM = 3, 128, 8, 12
LABELS = (0, 2, NULL)
SCALES = {"one": 2.0, "per_shape": (1.0, 2.0, 3.5)}
# sampler clouds rel-L2 <= 2e-3 in fp16; fp32 mode rel-L2 <= 5e-5 with max-abs <= 1e-3 * max(1, max|x| / 100)
TOL = {"fp16": dict(rel=2e-3, maxabs=None), "fp32": dict(rel=5e-5, maxabs=1e-3)}


def class_table():
    """nn.Embedding's default init, N(0, 1), from a fixed seed: (K + 1, 256)."""
    return torch.randn(K + 1, 256, generator=torch.Generator().manual_seed(5))


def class_sd():
    sd = point_sd()
    sd["model.class_emb.weight"] = class_table()
    return sd


_models = {}


def model_of(prec, n=N):
    from shapegen_amd.diffusion import PointCloudDiffusion
    if (prec, n) not in _models:
        m = PointCloudDiffusion(num_points=n, num_classes=K)
        m.load_state_dict(class_sd(), strict=True)
        m = m.to(DEV).eval()
        m.model.set_precision(prec)
        _models[(prec, n)] = m
    return _models[(prec, n)]


def reseed(m, seed=7):
    torch.manual_seed(seed)
    m._philox_offset = 0


def inputs():
    g = torch.Generator().manual_seed(11)
    x_T = torch.randn(B, N, 3, generator=g)
    noises = [torch.randn(B, N, 3, generator=g) for _ in range(T - 1)]
    return x_T, noises


_refs = {}


def reference(kind, scale_key):
    """The statement over the CPU oracle network, computed once per case and left unchanged."""
    if (kind, scale_key) not in _refs:
        x_T, noises = inputs()
        _refs[(kind, scale_key)] = S.sample(kind, point_sd(), "model.", class_table(), LABELS, SCALES[scale_key], x_T,
                                            T_DPM if kind == "dpm" else T, noises)
    return _refs[(kind, scale_key)]


def run_sampler(m, kind, scale, x_T, noises, labels=LABELS):
    w = torch.tensor(scale) if isinstance(scale, tuple) else scale
    lab = torch.tensor(labels)
    if kind == "ddim":
        return m.sample(B, N, num_steps=T, x_T=x_T.to(DEV), labels=lab, guidance_scale=w)
    if kind == "ddpm":
        return m.sample2(B, N, num_steps=T, x_T=x_T.to(DEV), noises=[z.to(DEV) for z in noises], labels=lab, guidance_scale=w)
    return m.sample_dpm(B, N, num_steps=T_DPM, x_T=x_T.to(DEV), labels=lab, guidance_scale=w)


# ------------------------------------------------------------------ 1. kernels of csrc/pointwise.hip
@pytest.mark.parametrize("width", [1, 3])
def test_step_select_labels_kernel_bitwise(width):
    """B = 3, labels (2, 0, null), T = 5, 64 bias elements, 7 calls (the clamp at T - 1 is hit twice): rows, rates, counter."""
    from shapegen_amd import _lib
    lib = _lib.load()
    steps, tb, cols = 5, 64, 4
    g = torch.Generator().manual_seed(1)
    table = torch.randn(steps, tb, generator=g)
    cb = torch.randn(K + 1, tb, generator=g)
    rates = torch.randn(cols, steps, width, generator=g)
    d = lambda t: t.to(DEV).contiguous()
    dt, dc, dr = d(table), d(cb), d(rates)
    for labels in ((2, 0, NULL), (7, -1, 0)):                                   # outside the table: read as the null row
        rows_of = [l if 0 <= l <= K else NULL for l in labels] + [NULL]
        dl = torch.tensor(labels, dtype=torch.int32, device=DEV)
        counter = torch.zeros(2, dtype=torch.int32, device=DEV)
        out = torch.full((3 + 1, tb), 9.0, device=DEV)
        cur = torch.full((cols * width,), 9.0, device=DEV)
        for call in range(7):
            _lib.check(lib.pcd_step_select_labels(counter.data_ptr(), steps, dt.data_ptr(), tb, out.data_ptr(), dc.data_ptr(), K + 1,
                                                  dl.data_ptr(), 3, NULL, dr.data_ptr(), cols, width, cur.data_ptr(), _lib.stream_ptr()))
            k = min(call, steps - 1)
            assert counter.tolist() == [k + 1, k]
            want = torch.stack([table[k] + cb[r] for r in rows_of])
            assert torch.equal(out.cpu(), want), (labels, call)
            assert torch.equal(cur.cpu(), rates[:, k, :].reshape(-1))
    # the unlabelled select leaves the same rates and counter
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    one, cur2 = torch.empty(tb, device=DEV), torch.empty(cols * width, device=DEV)
    for call in range(7):
        _lib.check(lib.pcd_step_select_cols(counter.data_ptr(), steps, dt.data_ptr(), tb, one.data_ptr(), dr.data_ptr(), cols, width,
                                            cur2.data_ptr(), _lib.stream_ptr()))
    assert counter.tolist() == [steps, steps - 1] and torch.equal(cur2, cur) and torch.equal(one.cpu(), table[steps - 1])


@pytest.mark.parametrize("per_shape_w", [False, True])
def test_cfg_combine_kernel_bitwise(per_shape_w):
    """(3, 37, 3): n = 333, n % 4 = 1.  Against the unfused fp32 expression eu + w * (ec - eu), from 16-byte aligned pointers
    (four per lane and a tail) and from pointers one float past a boundary (one per lane)."""
    from shapegen_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(2)
    ec, eu = torch.randn(3, 37, 3, generator=g), torch.randn(3, 37, 3, generator=g)
    w = torch.tensor([1.0, 2.0, 3.5]) if per_shape_w else torch.tensor([2.0])
    d = ec - eu
    want = eu + w.expand(3)[:, None, None] * d
    dw = w.to(DEV)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=DEV)
        assert buf.data_ptr() % 16 == 0
        buf[1:].copy_(t.reshape(-1))
        return buf[1:]

    for a, b in ((ec.to(DEV).contiguous(), eu.to(DEV).contiguous()), (shifted(ec), shifted(eu)), (shifted(ec), eu.to(DEV).contiguous())):
        u0 = b.clone()
        _lib.check(lib.pcd_cfg_combine(a.data_ptr(), b.data_ptr(), dw.data_ptr(), int(per_shape_w), 333, 111, _lib.stream_ptr()))
        assert torch.equal(a.cpu().reshape(3, 37, 3), want) and torch.equal(b, u0)
    if per_shape_w:                                                              # w = 1 is the expression too, not a copy
        assert torch.equal(want[0], eu[0] + 1.0 * (ec[0] - eu[0]))


# ------------------------------------------------------------------ 2. kernels of csrc/train.hip
def test_embedding_kernels_bitwise():
    """B = 5, labels (2, 0, 2, null, 2), dim 256: forward; backward against a float loop in ascending b; row 1, which no shape
    uses, is written as exactly zero; two runs agree bitwise."""
    from shapegen_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    labels = (2, 0, 2, NULL, 2)
    temb, table, dtemb = torch.randn(5, 256, generator=g), torch.randn(K + 1, 256, generator=g), torch.randn(5, 256, generator=g) * 1e3
    dl = torch.tensor(labels, dtype=torch.int32, device=DEV)
    dt, dtab, dd = temb.to(DEV), table.to(DEV), dtemb.to(DEV)
    _lib.check(lib.pcd_embed_add_rows(dt.data_ptr(), dtab.data_ptr(), dl.data_ptr(), 5, 256, K + 1, _lib.stream_ptr()))
    assert torch.equal(dt.cpu(), temb + table[list(labels)])
    want = torch.zeros(K + 1, 256)
    for b, c in enumerate(labels):
        want[c] = want[c] + dtemb[b]
    outs = []
    for _ in range(2):
        out = torch.full((K + 1, 256), 9.0, device=DEV)
        _lib.check(lib.pcd_embed_rows_backward(dd.data_ptr(), dl.data_ptr(), 5, 256, K + 1, out.data_ptr(), _lib.stream_ptr()))
        outs.append(out.cpu())
    assert torch.equal(outs[0], want) and torch.equal(outs[0], outs[1])
    assert bool((outs[0][1] == 0).all()) and not torch.equal(want[2], dtemb[0] + (dtemb[2] + dtemb[4]))


def test_class_bias_goes_through_the_packed_time_columns():
    """class_bias() = the folded time columns of enc1.conv1 applied to the embedding rows, no bias term, in both precisions;
    rebuilt when the weights are invalidated."""
    from shapegen_amd import packing
    _, ex = packing.pack_point_unet(point_sd(), "model.", 256, 256)
    want = class_table().double().numpy() @ ex["e1w_t"].T
    for prec in ("fp16", "fp32"):
        m = model_of(prec)
        cb = m.model.class_bias()
        assert cb.shape == (K + 1, 64) and cb.dtype == torch.float32 and rel_l2(cb.cpu(), want) < 1e-6
        assert m.model.class_bias() is cb
    m = model_of("fp16")
    with torch.no_grad():
        m.model.class_emb.weight[1] += 1.0
    m.model.invalidate()
    cb2 = m.model.class_bias()
    assert not torch.equal(cb2[1], cb[1]) and torch.equal(cb2[0], m.model.class_bias()[0])
    m.load_state_dict(class_sd(), strict=True)                                   # loading invalidates too
    assert rel_l2(m.model.class_bias().cpu(), want) < 1e-6
    # the module's own forward adds the same rows
    g = torch.Generator().manual_seed(4)
    x, t = torch.randn(B, N, 3, generator=g), torch.tensor([0.2, 0.5, 0.9])
    with torch.no_grad():
        ref = S.eps_of(point_sd(), "model.", class_table(), LABELS, x, t)
    got = model_of("fp32").model(x.to(DEV), t.to(DEV), torch.tensor(LABELS))
    assert rel_l2(got.cpu(), ref) < 1e-4                                         # the fp32 mode's eps bound (networks._Denoiser)
    none = model_of("fp32").model(x.to(DEV), t.to(DEV))
    null = model_of("fp32").model(x.to(DEV), t.to(DEV), torch.tensor([NULL] * B))
    assert torch.equal(none, null) and torch.equal(none[2], got[2]) and not torch.equal(none[0], got[0])


# ------------------------------------------------------------------ 3. guided samplers against the statement
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("scale_key", ["one", "per_shape"])
@pytest.mark.parametrize("kind", ["ddim", "ddpm", "dpm"])
def test_guided_samplers_against_the_statement(kind, scale_key, prec):
    """DDIM and DDPM (injected noises) at (3, 128), T = 8; sample_dpm at K = 12 (graph path); labels (0, 2, null); scale 2.0 and
    per-shape scales (1.0, 2.0, 3.5).  Guidance multiplies a forward's error by at most 2 w - 1, so the fp16 figures are expected
    near 3 x completion's 2.6e-4.
    The figures are printed before the assertions; all twelve cases hold their bound on an MI355X, the figures themselves are
    not recorded yet (DESIGN section 4 says the same)."""
    x_T, noises = inputs()
    want = reference(kind, scale_key)
    assert torch.isfinite(want).all()
    got = run_sampler(model_of(prec), kind, SCALES[scale_key], x_T, noises).cpu()
    tol = TOL[prec]
    r, mx = rel_l2(got, want), float((got - want).abs().max())
    print(f"cfg {kind} scale {scale_key} [{prec}]: rel-L2 {r:.3e}  max-abs {mx:.3e}  max|x| {float(want.abs().max()):.3g}")
    assert r <= tol["rel"], (kind, scale_key, prec, r)
    if tol["maxabs"] is not None:
        assert mx <= tol["maxabs"] * max(1.0, float(want.abs().max()) / 100.0), (kind, scale_key, prec, mx)


# ------------------------------------------------------------------ 4. bitwise identities
def test_scale_one_runs_one_forward_and_is_the_conditional_run():
    m = model_of("fp16")
    x_T, noises = inputs()
    calls, inner = [], m.model.forward_with_bias
    m.model.forward_with_bias = lambda x, tb, stride, out=None: (calls.append(stride), inner(x, tb, stride, out=out))[1]
    try:
        one = run_sampler(m, "ddim", 1.0, x_T, noises)
        assert calls == [1] * T                                                  # no second forward
        del calls[:]
        ones = run_sampler(m, "ddim", (1.0, 1.0, 1.0), x_T, noises)
        assert calls == [1] * T
        del calls[:]
        two = run_sampler(m, "ddim", 2.0, x_T, noises)
        assert calls == [1, 0] * T
    finally:
        del m.model.forward_with_bias
    assert torch.equal(one, ones) and not torch.equal(one, two)
    # ... and it is the statement's conditional-only run
    with torch.no_grad():
        want = S.sample("ddim", point_sd(), "model.", class_table(), LABELS, 1.0, x_T, T)
    assert rel_l2(one.cpu(), want) <= TOL["fp16"]["rel"]
    # labels=None on a class model is the null class
    assert torch.equal(m.sample(B, N, num_steps=T, x_T=x_T.to(DEV)), m.sample(B, N, num_steps=T, x_T=x_T.to(DEV), labels=[NULL] * B))


def test_null_labels_with_guidance_agree_with_scale_one():
    """All labels null: eps_c = eps_u, so scale 2 is eu + 2 (eu - eu): its own scale-1 run to the fp32 bound."""
    m = model_of("fp32")
    x_T, noises = inputs()
    a = run_sampler(m, "ddim", 1.0, x_T, noises, labels=(NULL,) * B).cpu()
    b = run_sampler(m, "ddim", 2.0, x_T, noises, labels=(NULL,) * B).cpu()
    r, mx = rel_l2(b, a), float((a - b).abs().max())
    print(f"null labels, scale 2 v. scale 1 [fp32]: rel-L2 {r:.3e} max-abs {mx:.3e}")
    assert r <= TOL["fp32"]["rel"] and mx <= TOL["fp32"]["maxabs"] * max(1.0, float(a.abs().max()) / 100.0)


@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_graph_replay_equals_eager_stepping(kind):
    """(2, 64), 20 steps: one eager step, two graphs of 8, the rest eager; DDIM and DDPM with on-device noise."""
    m = model_of("fp16", 64)
    steps = 20
    assert steps - 2 >= m.GRAPH_MIN_STEPS and m.use_graphs
    x_T = torch.randn(2, 64, 3, generator=torch.Generator().manual_seed(13)).to(DEV)
    fn = m.sample if kind == "ddim" else m.sample2
    outs = []
    for graphs in (True, False):
        with counted_replays(m, graphs) as seen:
            reseed(m)
            outs.append(fn(2, 64, num_steps=steps, x_T=x_T, labels=[1, NULL], guidance_scale=torch.tensor([2.0, 1.5])))
            assert len(seen) == (2 if graphs else 0)
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()


def test_two_shards_equal_the_whole_batch_through_sample_sharded():
    from shapegen_amd import dist as D
    m = model_of("fp16")
    labels, scales = torch.tensor([0, 2, NULL, 1]), torch.tensor([1.0, 2.0, 3.5, 2.0])
    reseed(m)
    whole = D.sample_sharded(m, 4, N, T, sampler="sample2", labels_global=labels, guidance_scale=scales)
    halves, inner = [], D.world
    try:
        for rank in (0, 1):
            D.world = lambda rank=rank: (rank, 2)
            reseed(m)
            halves.append(D.sample_sharded(m, 4, N, T, sampler="sample2", gather=False, labels_global=labels, guidance_scale=scales))
    finally:
        D.world = inner
    assert halves[0].shape == (2, N, 3) and torch.equal(torch.cat(halves), whole)
    reseed(m)
    assert torch.equal(m.sample2(4, N, num_steps=T, labels=labels, guidance_scale=scales), whole)
    reseed(m)
    assert not torch.equal(m.sample2(4, N, num_steps=T, labels=labels), whole)


def test_complete_with_labels_keeps_known_rows_bitwise():
    from shapegen_amd import dist as D
    m = model_of("fp16")
    g = torch.Generator().manual_seed(21)
    partial = torch.randn(B, N, 3, generator=g)
    partial = partial / partial.norm(dim=2).max(dim=1).values[:, None, None]
    counts = torch.tensor([0, 37, 128])
    reseed(m)
    out = m.complete(partial.to(DEV), N, num_steps=12, known_counts=counts, resample=2, jump=4, labels=list(LABELS), guidance_scale=2.0)
    assert torch.isfinite(out).all()
    for b, c in enumerate(counts.tolist()):
        assert torch.equal(out[b, :c].cpu(), partial[b, :c])
    reseed(m)
    plain = m.complete(partial.to(DEV), N, num_steps=12, known_counts=counts, resample=2, jump=4)
    assert not torch.equal(plain[0], out[0]) and torch.equal(plain[2], out[2])
    reseed(m)
    assert torch.equal(D.complete_sharded(m, partial, counts, N, 12, resample=2, jump=4, labels_global=torch.tensor(LABELS),
                                          guidance_scale=2.0), out)


# ------------------------------------------------------------------ 5. training
TB, TN = 4, 128
TLABELS = (1, 0, 1, NULL)


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():
        yield


def train_inputs():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(TB, TN, 3, generator=g) * 0.5
    t = torch.rand(TB, generator=g)
    noise = torch.randn(TB, TN, 3, generator=g)
    return x, t, noise, torch.randn(x.shape, generator=g)


def train_table():
    """The training tests' embedding table: class_table() at a tenth of its scale.  Through enc1.conv1's time columns the rows then
    spread the per-shape bias by 0.11 rms, 1.7 x the xyz term (0.067) and 3.4 x what the four time embeddings spread it by (0.032).
    Unit-variance rows spread it by 1.12, 17 x the xyz term: BatchNorm's batch statistics then leave the per-point signal a
    seventeenth of enc1.conv1's activation, and storing that activation in fp16 alone moves the float statement's own prediction
    by 5.1e-2 (`statement_moved_by_fp16_activations`), most of the bound that tests/test_gpu_train.py wrote for a batch where all
    of the fp16 activations together move it by 2.2e-2."""
    return 0.1 * class_table()


def fresh_train_model(n=TN):
    from shapegen_amd.diffusion import PointCloudDiffusion
    model = PointCloudDiffusion(num_points=n, num_classes=K)
    sd = point_sd()
    sd["model.class_emb.weight"] = train_table()
    model.load_state_dict(sd, strict=True)
    return model.to(DEV)


def statement_moved_by_fp16_activations(sd, E, labels, x_t, t):
    """rel-L2 by which the float statement's own train-mode prediction moves when every ReLU output is rounded to fp16, the type
    the trainer keeps activations in (its GEMMs accumulate in fp32, its BatchNorm inputs stay fp32).  CPU only."""
    relu = F.relu
    with torch.no_grad():
        exact = S.eps_of({k: v.clone() for k, v in sd.items()}, "model.", E, labels, x_t, t, train=True)
        F.relu = lambda x, *a, **kw: relu(x).half().float()
        try:
            rounded = S.eps_of({k: v.clone() for k, v in sd.items()}, "model.", E, labels, x_t, t, train=True)
        finally:
            F.relu = relu
    return rel_l2(rounded, exact)


def test_training_step_against_the_statement():
    """One step at (4, 128), labels (1, 0, 1, null).  The input is conditioned first: the statement's own class_emb gradient under a
    3e-4 input perturbation (tools/train_conditioning.py's measure) must keep a cosine of at least 0.9 (measured on the CPU: 0.928;
    the other tensors 0.937 at the least).  Bounds: tests/test_gpu_train.py's, class_emb.weight held to the same cosine and norm-ratio bounds
    as every other tensor.

    The input is also conditioned for the type the trainer stores activations in: rounding the statement's own ReLU outputs to
    fp16 must move its prediction by no more than 2.5e-2, the trainer's measured figure on the batch that the 6e-2 bound was
    written for (the same rounding moves that batch's statement by 2.2e-2).  `train_table()` meets it with 2.1e-2; with
    unit-variance rows the statement moves by 5.8e-2 and the trainer's prediction measured 6.5e-2 (see `train_table`)."""
    from shapegen_amd.training import PointTrainer
    x_t, t, noise, pert = train_inputs()
    sd = point_sd()
    E = train_table()
    moved16 = statement_moved_by_fp16_activations(sd, E, TLABELS, x_t, t)
    print(f"statement's prediction moves by {moved16:.3e} when its activations are rounded to fp16")
    assert moved16 <= 2.5e-2
    sd_ref = {k: v.clone() for k, v in sd.items()}
    loss_ref, grads_ref = S.training_step(sd_ref, "model.", E, TLABELS, x_t, t, noise)
    _, moved = S.training_step({k: v.clone() for k, v in sd.items()}, "model.", E, TLABELS, x_t + 3e-4 * pert, t, noise)
    a, b = grads_ref["model.class_emb.weight"].double(), moved["model.class_emb.weight"].double()
    conditioning = float((a * b).sum() / (a.norm() * b.norm()))
    print(f"statement's class_emb gradient cosine under a 3e-4 input perturbation: {conditioning:.3f}")
    assert conditioning >= 0.9
    with torch.no_grad():
        pred_ref = S.eps_of({k: v.clone() for k, v in sd.items()}, "model.", E, TLABELS, x_t, t, train=True)
    model = fresh_train_model()
    tr = PointTrainer(model.model, lr=1e-4)
    pred = tr.forward(x_t.to(DEV), t.to(DEV), labels=torch.tensor(TLABELS))
    loss = tr.backward(noise.to(DEV))
    print(f"prediction rel-L2 {rel_l2(pred.cpu(), pred_ref):.3e}")
    assert rel_l2(pred.cpu(), pred_ref) < 6e-2
    assert abs(loss.item() - loss_ref.item()) <= 1e-2 * loss_ref.item()
    grads = tr.grads()
    assert set("model." + k for k in grads) == set(grads_ref)
    cos = {}
    for k, gr in grads_ref.items():
        mine = grads[k[len("model."):]].cpu()
        assert mine.shape == gr.shape and torch.isfinite(mine).all(), k
        if gr.dim() > 1 and gr.norm() > 0:
            cos[k] = F.cosine_similarity(mine.reshape(1, -1), gr.reshape(1, -1)).item()
            assert 0.8 < mine.norm().item() / gr.norm().item() < 1.25, k
    ce = "model.class_emb.weight"
    print(f"class_emb.weight: cosine {cos[ce]:.3f}, norm ratio {grads['class_emb.weight'].norm().item() / grads_ref[ce].norm().item():.3f}; "
          f"all tensors: cosine min {min(cos.values()):.3f} median {np.median(list(cos.values())):.3f}; loss {loss.item():.5f} v. {loss_ref.item():.5f}")
    assert ce in cos and min(cos.values()) > 0.85 and np.median(list(cos.values())) > 0.9, sorted(cos.items(), key=lambda kv: kv[1])[:5]
    assert bool((grads["class_emb.weight"][2] == 0).all())                       # class 2 has no shape in the batch
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            assert torch.allclose(v.cpu(), sd_ref[k], rtol=2e-2, atol=2e-2), k
    # the gradient of the table is bitwise the ordered segmented sum of the trainer's own dtemb buffer
    dtemb = tr._ws["bwd.dtemb"].cpu()
    want = torch.zeros(K + 1, 256)
    for i, c in enumerate(TLABELS):
        want[c] = want[c] + dtemb[i]
    assert torch.equal(tr.g["class_emb.weight"].cpu(), want)
    # labels=None trains the null row alone; a model without classes refuses labels
    tr.forward(x_t.to(DEV), t.to(DEV), update_stats=False)
    tr.backward(noise.to(DEV))
    gn = tr.g["class_emb.weight"]
    assert bool((gn[:K] == 0).all()) and float(gn[NULL].abs().max()) > 0
    from shapegen_amd.diffusion import PointCloudDiffusion
    plain = PointCloudDiffusion(num_points=TN).to(DEV)
    with pytest.raises(ValueError):
        PointTrainer(plain.model).forward(x_t.to(DEV), t.to(DEV), labels=torch.tensor(TLABELS))


def test_two_identical_steps_give_bitwise_equal_state():
    x_t, t, noise, _ = train_inputs()
    states = []
    for _ in range(2):
        model = fresh_train_model()
        tr = model.configure_optimizers()["optimizer"]
        tr.enable_ema(0.9)
        for _ in range(2):
            tr.train_step(x_t.to(DEV), t.to(DEV), noise.to(DEV), labels=torch.tensor(TLABELS))
        states.append(R.snapshot(model))
    assert R.compare(states[0], states[1]) == {}
    assert not torch.equal(states[0]["sd.model.class_emb.weight"], train_table())      # AdamW moved the table with everything else


class LabelledBatches(R.Batches):
    """R.Batches whose items are (clouds, labels)."""

    def __init__(self, x, labels, batch, train):
        super().__init__(x, batch, train)
        self.labels = labels

    def _pair(self, i):
        return self.x[i * self.batch:(i + 1) * self.batch], self.labels[i * self.batch:(i + 1) * self.batch]

    def train_dataloader(self):
        return (self._pair(i) for i in torch.randperm(self.train).tolist())

    def val_dataloader(self):
        return iter([self._pair(self.train)])


def labelled_run(**fit_kw):
    """R.run for a class-conditional point model on labelled synthetic clouds: 4 batches of (4, 256) per epoch."""
    import random
    from shapegen_amd.diffusion import PointCloudDiffusion
    from shapegen_amd.training import fit
    torch.manual_seed(7)
    random.seed(7)
    np.random.seed(7)
    g = torch.Generator().manual_seed(11)
    model = R._eager_plateau(PointCloudDiffusion)(num_points=256, num_classes=K, p_uncond=0.25).to(DEV)
    data = LabelledBatches(torch.rand(20, 256, 3, generator=g) * 2 - 1, torch.arange(20) % K, 4, 4)
    notes = R.record_steps(model)
    history = fit(model, data, max_epochs=R.EPOCHS, log=lambda *_: None, **fit_kw)
    return model, history, notes


def test_resumed_labelled_run_is_the_uninterrupted_run_and_ema_table_loads(tmp_path):
    """2 + 2 epochs with `save_last` and `ckpt_path` against 4 epochs in one go, EMA on: parameters (class_emb among them), buffers,
    both moments and the EMA buffer bitwise; label dropout draws from the restored random stream.  `weights="ema"` loads the averaged
    table."""
    from shapegen_amd.checkpoint import read_checkpoint
    from shapegen_amd.diffusion import PointCloudDiffusion
    ma, ha, na = labelled_run(ema_decay=0.9)
    sa = R.snapshot(ma)
    assert not torch.equal(sa["ema"], ma._trainer.P.cpu())
    m1, h1, n1 = labelled_run(ema_decay=0.9, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True, max_steps=8)
    assert len(h1) == 2 and n1 == na[:8]
    del m1
    last = str(tmp_path / "run-last.ckpt")
    ck = read_checkpoint(last)
    assert ck["epoch"] == 1 and ck["global_step"] == 8
    assert ck["hyper_parameters"]["num_classes"] == K and ck["hyper_parameters"]["p_uncond"] == 0.25
    assert "model.class_emb.weight" in ck["state_dict"] and "model.class_emb.weight" in ck["ema_state_dict"]
    mc, hc, nc = labelled_run(ckpt_path=last, ckpt_dir=str(tmp_path), ckpt_name="run", save_last=True)
    sc = R.snapshot(mc)
    print(f"labelled point run resumed: differing tensors {R.compare(sa, sc)}")
    assert nc == na[8:] and [h[3] for h in hc] == [h[3] for h in ha]
    assert R.compare(sa, sc) == {}
    # the averaged table
    final = read_checkpoint(last)
    ema = PointCloudDiffusion.load_from_checkpoint(last, weights="ema")
    raw = PointCloudDiffusion.load_from_checkpoint(last)
    assert ema.num_classes == K
    tr = mc._trainer
    assert torch.equal(ema.state_dict()["model.class_emb.weight"], tr.ema_state_dict()["class_emb.weight"].cpu())
    assert torch.equal(raw.state_dict()["model.class_emb.weight"], mc.state_dict()["model.class_emb.weight"].cpu())
    assert not torch.equal(ema.state_dict()["model.class_emb.weight"], raw.state_dict()["model.class_emb.weight"])
    assert final["shapegen_amd"]["trainer"]["layout"][-1] == ("class_emb.weight", (K + 1) * 256)
    # a trainer of a model without classes refuses this optimizer state (another parameter layout)
    plain = PointCloudDiffusion(num_points=256).to(DEV)
    with pytest.raises(RuntimeError, match="layout"):
        plain.configure_optimizers()["optimizer"].load_state_dict(tr.state_dict())


# ------------------------------------------------------------------ 6. the entry scripts
def test_entry_scripts_class_conditional(tmp_path):
    """train_point_ddpm.py --class-conditional for one epoch on synthetic clouds, then generate_point_ddpm.py --label 1 --guidance 2
    from its checkpoint, and once more on the synthetic-weights model; fresh child processes, each under its own time limit."""
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(args):
        r = subprocess.run([sys.executable] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    run([os.path.join(ROOT, "train_point_ddpm.py"), "--class-conditional", "--epochs", "1", "--num-points", "256", "--batch-size", "8",
         "--synthetic-shapes", "40", "--sample-steps", "5", "--out", str(tmp_path / "p"), "--data-dir", str(tmp_path / "none")])
    assert np.load(tmp_path / "p" / "samples.npy").shape == (10, 256, 3)
    ckpts = glob.glob(str(tmp_path / "checkpoints" / "point_ddpm" / "*" / "*.ckpt"))
    assert len(ckpts) == 1
    ck = torch.load(ckpts[0], map_location="cpu", weights_only=False)
    assert ck["hyper_parameters"]["num_classes"] == 3 and tuple(ck["state_dict"]["model.class_emb.weight"].shape) == (4, 256)
    gen = [os.path.join(ROOT, "generate_point_ddpm.py"), "--label", "1", "--guidance", "2", "--num-samples", "4", "--steps", "12",
           "--num-points", "256"]
    run(gen + ["--ckpt-dir", os.path.dirname(ckpts[0]), "--out", str(tmp_path / "g")])
    z = np.load(tmp_path / "g" / "generated.npz")
    assert z["samples"].shape == (4, 256, 3) and np.isfinite(z["samples"]).all() and int(z["label"]) == 1 and float(z["guidance"]) == 2.0
    run(gen + ["--ckpt-dir", str(tmp_path / "none"), "--out", str(tmp_path / "s")])
    z = np.load(tmp_path / "s" / "generated.npz")
    assert z["samples"].shape == (4, 256, 3) and np.isfinite(z["samples"]).all()
