"""tests/vae_train_statement.py (the per-layer yardstick of the GPU tests in test_gpu_train_vae.py) composed over
specs.VAE_ENC / VAE_DEC, against oracle.torch_oracle.vae_training_step, which tests/golden/train_vae.npz pins to the
reference.  Both run in float64 and state the same function, so they agree to rounding."""
import torch
import torch.nn.functional as F

import vae_train_statement as S
from helpers import as_torch, rel_l2, synth_voxels
from oracle import torch_oracle as O
from shapegen_amd import specs


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def test_vae_statement_matches_oracle_f64():
    sd = _f64(as_torch(specs.synth_state_dict(specs.vae3d_large_spec(prefix="vae."), seed=0, gain=1.3)))
    x = synth_voxels(2, 5).double()
    eps = torch.randn(2, 256, generator=torch.Generator().manual_seed(1)).double()
    want = O.vae_training_step(_f64(sd), "vae.", x, eps, 0.01, specs.VAE_ENC, specs.VAE_DEC)
    got = S.vae_training_step(sd, "vae.", x, eps, 0.01, specs.VAE_ENC, specs.VAE_DEC)
    assert want[0].dtype == torch.float64 and got[0].dtype == torch.float64
    for name, a, b in zip(("loss", "recon_loss", "kl", "recon", "mu", "logvar"), got[:6], want[:6]):
        assert rel_l2(a, b) < 1e-9, (name, rel_l2(a, b))
    g_got, g_want = got[6], want[6]
    assert sorted(g_got) == sorted(g_want) and len(g_got) == 98     # 2 x (5 convs x 2 + 4 blocks x 8) + 4 downsamples x 2 + 3 linears x 2
    n_zero = 0
    for k, gr in g_want.items():
        if S.is_bias_before_batchnorm(k):
            # analytic zero: both sides hold float64 rounding noise of the layer's gradient scale, nothing to compare
            scale = g_want[k[:-len("bias")] + "weight"].norm()
            assert gr.norm() < 1e-9 * scale and g_got[k].norm() < 1e-9 * scale, k
            n_zero += 1
            continue
        assert gr.norm() > 0, k
        assert rel_l2(g_got[k], gr) < 1e-9, (k, rel_l2(g_got[k], gr))
    assert n_zero == 16          # two per residual block, 4 + 4 blocks


def test_fp16_operand_noise_floor_of_the_oracle_gradients():
    """Where S.FP16_OPERAND_FLOOR comes from: the oracle's fp32 step as is and with every conv / linear input and weight
    rounded through fp16, per class of 1-D parameter the worst 1 - cosine and |log norm ratio| between the two.  The
    committed figures must be what this measures (10 %: thread count and library version move the last digits)."""
    sd = as_torch(specs.synth_state_dict(specs.vae3d_large_spec(prefix="vae."), seed=0, gain=1.3))
    x = synth_voxels(2, 5)
    eps = torch.randn(2, 256, generator=torch.Generator().manual_seed(1))
    plain = O.vae_training_step(dict(sd), "vae.", x, eps, 0.01, specs.VAE_ENC, specs.VAE_DEC)[6]
    conv3d = F.conv3d
    with S.fp16_operands():
        assert F.conv3d is not conv3d
        rounded = O.vae_training_step(dict(sd), "vae.", x, eps, 0.01, specs.VAE_ENC, specs.VAE_DEC)[6]
    assert F.conv3d is conv3d                                   # the patch is undone
    floor = {}
    for k, g in plain.items():
        c = S.tensor_class(k)
        if c is None or S.is_bias_before_batchnorm(k):
            continue
        cs, lr = S.cos_and_log_ratio(rounded[k], g)
        f = floor.setdefault(c, [0.0, 0.0])
        f[0], f[1] = max(f[0], 1 - cs), max(f[1], abs(lr))
    print("fp16-operand floor:", floor)
    assert sorted(floor) == sorted(S.FP16_OPERAND_FLOOR)
    for c, (one_minus_cos, log_ratio) in S.FP16_OPERAND_FLOOR.items():
        assert abs(floor[c][0] - one_minus_cos) < 0.1 * one_minus_cos, (c, floor[c])
        assert abs(floor[c][1] - log_ratio) < 0.1 * log_ratio, (c, floor[c])


def test_row_matrix_conversions_round_trip():
    x = torch.arange(2 * 3 * 4 * 4 * 4, dtype=torch.float64).reshape(2, 3, 4, 4, 4)
    rows = S.ncdhw_to_rows(x)
    assert rows.shape == (128, 3) and rows[1 * 64 + 2 * 16 + 3 * 4 + 1, 2] == x[1, 2, 2, 3, 1]
    padded = torch.zeros(192, 64, dtype=torch.float64)
    padded[:128, :3] = rows
    assert torch.equal(S.rows_to_ncdhw(padded, 2, 4, 3), x)
