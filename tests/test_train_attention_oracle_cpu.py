"""Pins the train-mode statement of the attention denoiser (tests/attn_train_statement.py) to
tests/golden/train_attention.npz, captured from the reference's PointCloudDiffusion with UNetAttentionPointExperimental
in train() mode, autograd and torch.optim.AdamW (`python tools/make_golden_train_attention.py`)."""
import numpy as np
import torch

from attn_train_statement import attention_training_step
from helpers import una_sd
from oracle import torch_oracle as O
from shapegen_amd import specs


def _digest_idx(name, numel):
    return (np.abs(specs.hash_uniform("digest." + name, 64, 7)) * (numel - 1)).astype(np.int64)


def test_attention_training_step_matches_reference(golden):
    g = golden("train_attention.npz")
    sd = {"model." + k: v for k, v in una_sd().items()}
    x_t, t, noise = (torch.from_numpy(g[k]) for k in ("x_t", "t", "noise"))
    assert torch.equal(O.add_noise(torch.from_numpy(g["x0"]), t, noise)[0], x_t)
    loss, pred, grads = attention_training_step(sd, "model.", x_t, t, noise)
    assert abs(loss.item() - float(g["loss"])) <= 1e-5
    assert np.abs(pred.numpy() - g["pred"]).max() <= 1e-4 * max(1.0, np.abs(g["pred"]).max())
    names = [str(n) for n in g["param_names"]]
    assert sorted(names) == sorted(grads.keys())
    top = max(float(g["grad." + k][0]) for k in names)
    zero = set()
    for k in names:
        flat = grads[k].reshape(-1).double()
        want = g["grad." + k]
        if want[0] < 1e-6 * top:
            # analytic zero (a bias in front of a BatchNorm, emb1.bias): both sides hold rounding noise only
            assert flat.norm().item() < 1e-6 * top, k
            zero.add(k)
            continue
        got = np.concatenate([[flat.norm().item(), flat.sum().item()], flat[torch.from_numpy(_digest_idx(k, flat.numel()))].numpy()])
        scale = max(want[0], 1e-12)
        assert abs(got[0] - want[0]) <= 1e-4 * scale, k
        assert np.abs(got[2:] - want[2:]).max() <= 1e-4 * max(np.abs(want[2:]).max(), 1e-3 * scale / flat.numel() ** 0.5) + 1e-9, k
    for k, v in sd.items():
        if k.endswith(("running_mean", "running_var")):
            assert np.allclose(v.numpy(), g["buf1." + k], rtol=1e-5, atol=1e-6), k
    params = {k: sd[k].clone() for k in names}
    O.adamw_step(params, grads, {}, lr=1e-4, weight_decay=1e-5)
    for k in names:
        if k in zero:
            continue             # AdamW normalises the rounding noise to a full-size step: its sign is not reproducible
        flat = params[k].reshape(-1).double()
        got = flat[torch.from_numpy(_digest_idx(k, flat.numel()))].numpy()
        # entries with an analytic-zero gradient (the key bias of in_proj: softmax is shift invariant) are skipped as well
        live = np.abs(g["grad." + k][2:]) > 1e-5 * g["grad." + k][0]
        assert np.abs(got - g["param1." + k])[live].max(initial=0.0) <= 2e-6, k
