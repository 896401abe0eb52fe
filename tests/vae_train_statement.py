"""Plain torch statement of what one layer of `VAE3DLarge` computes in train() mode, and of one whole training step
composed from those layers (reference networks.py:488-504 ResidualBlock3D, :2225-2264 encoder / decoder, :2341-2396
calculate_loss).  It works in whatever dtype its operands have (the tests feed float64) on NCDHW tensors, and holds no
trainer code: tests/test_train_vae_statement_cpu.py pins it to the oracle (and so to the reference, through
tests/golden/train_vae.npz); the GPU tests use it as the yardstick for the trainer's layers."""
import contextlib

import torch
import torch.nn.functional as F

BN_EPS = 1e-5


# ---------------------------------------------------------------- NCDHW <-> channels-last row matrices [B*D*H*W][C]
def rows_to_ncdhw(rows, b, d, c):
    """The first b*d^3 rows and c columns of a (row- and channel-padded) channels-last matrix as (b, c, d, d, d)."""
    return rows[:b * d ** 3, :c].reshape(b, d, d, d, c).permute(0, 4, 1, 2, 3)


def ncdhw_to_rows(x):
    return x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1])


# ---------------------------------------------------------------- layers
def batchnorm3d_train(z, gamma, beta):
    """BatchNorm3d on batch statistics: per-channel mean and biased variance over (N, D, H, W).  -> (y, mean, var)"""
    mean = z.mean(dim=(0, 2, 3, 4))
    var = ((z - mean.view(1, -1, 1, 1, 1)) ** 2).mean(dim=(0, 2, 3, 4))
    xhat = (z - mean.view(1, -1, 1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1, 1) + BN_EPS)
    return xhat * gamma.view(1, -1, 1, 1, 1) + beta.view(1, -1, 1, 1, 1), mean, var


def conv(x, w, bias, transposed, stride, padding):
    if transposed:
        return F.conv_transpose3d(x, w, bias, stride=stride, padding=padding)
    return F.conv3d(x, w, bias, stride=stride, padding=padding)


def vconv(x, w, bias, transposed=False, stride=1, padding=0, gamma=None, beta=None, relu=True):
    """Conv3d / ConvTranspose3d [+ BatchNorm3d] [+ ReLU].  -> dict(z, a, mean, var); mean / var None without a BatchNorm."""
    z = conv(x, w, bias, transposed, stride, padding)
    mean = var = None
    y = z
    if gamma is not None:
        y, mean, var = batchnorm3d_train(z, gamma, beta)
    return {"z": z, "a": F.relu(y) if relu else y, "mean": mean, "var": var}


def res_block(x, P):
    """ResidualBlock3D: relu(bn2(conv2(relu(bn1(conv1(x))))) + identity), identity = downsample(x) (a 1x1x1 Conv3d) where
    the channel count changes.  P: conv1.weight, conv1.bias, bn1.weight, bn1.bias, conv2.*, bn2.*, [downsample.*].
    -> dict(c1, c2 (the two `vconv` results), r (the identity path), out)"""
    c1 = vconv(x, P["conv1.weight"], P["conv1.bias"], False, 1, 1, P["bn1.weight"], P["bn1.bias"], relu=True)
    c2 = vconv(c1["a"], P["conv2.weight"], P["conv2.bias"], False, 1, 1, P["bn2.weight"], P["bn2.bias"], relu=False)
    r = conv(x, P["downsample.weight"], P["downsample.bias"], False, 1, 0) if "downsample.weight" in P else x
    return {"c1": c1, "c2": c2, "r": r, "out": F.relu(c2["a"] + r)}


def block_params(sd, key):
    """The entries of sd under `key.` with that prefix removed."""
    return {k[len(key) + 1:]: v for k, v in sd.items() if k.startswith(key + ".")}


def run_program(sd, prefix, prog, x, last_relu):
    for i, (idx, op, a) in enumerate(prog):
        key = f"{prefix}.{idx}"
        if op == "res":
            x = res_block(x, block_params(sd, key))["out"]
        else:
            relu = last_relu or i < len(prog) - 1
            x = vconv(x, sd[key + ".weight"], sd[key + ".bias"], op == "convT", a[3], a[4], relu=relu)["a"]
    return x


# ---------------------------------------------------------------- the whole step
def is_bias_before_batchnorm(key):
    """A conv bias directly in front of a BatchNorm3d (the two convs of a residual block): the batch mean removes it, so
    its gradient is the analytic zero."""
    return key.endswith((".conv1.bias", ".conv2.bias"))


def vae_forward_loss(sd, p, x, eps, kl_weight, enc_prog, dec_prog):
    """-> (loss, recon_loss, kl, recon, mu, logvar)"""
    b = x.shape[0]
    h = run_program(sd, p + "encoder", enc_prog, x, last_relu=True).reshape(b, 512)
    mu = h @ sd[p + "fc_mu.weight"].t() + sd[p + "fc_mu.bias"]
    logvar = h @ sd[p + "fc_logvar.weight"].t() + sd[p + "fc_logvar.bias"]
    z = mu + eps * torch.exp(logvar / 2)
    d = (z @ sd[p + "decoder_input.weight"].t() + sd[p + "decoder_input.bias"]).reshape(b, 512, 4, 4, 4)
    recon = torch.sigmoid(run_program(sd, p + "decoder", dec_prog, d, last_relu=False))
    bce = -(x * torch.log(recon).clamp_min(-100) + (1 - x) * torch.log(1 - recon).clamp_min(-100))     # torch's BCE log clamp
    recon_loss = bce.mean()
    kl = -0.5 * (1 + logvar - mu ** 2 - torch.exp(logvar)).mean()
    return recon_loss + kl_weight * kl, recon_loss, kl, recon, mu, logvar


def vae_training_step(sd, p, x, eps, kl_weight, enc_prog, dec_prog):
    """Same surface as oracle.torch_oracle.vae_training_step, without the running statistics:
    -> (loss, recon_loss, kl, recon, mu, logvar, {key: grad})."""
    work = dict(sd)
    leaves = {}
    for k, v in sd.items():
        if k.startswith(p) and v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
            leaves[k] = v.detach().clone().requires_grad_(True)
            work[k] = leaves[k]
    with torch.enable_grad():
        out = vae_forward_loss(work, p, x, eps, kl_weight, enc_prog, dec_prog)
        out[0].backward()
    return tuple(t.detach() for t in out) + ({k: v.grad for k, v in leaves.items()},)


# ---------------------------------------------------------------- the trainer's forward rounding points, emulated
class _RoundF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.half().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


@contextlib.contextmanager
def fp16_operands():
    """Inside: every F.conv3d / F.conv_transpose3d / F.linear rounds its input and its weight through fp16 (the operands
    of the trainer's GEMMs); sums, biases and gradients stay in the caller's precision.  Used to measure, on the
    reference side alone, how far fp16 operands move a gradient."""
    saved = {n: getattr(F, n) for n in ("conv3d", "conv_transpose3d", "linear")}

    def wrap(fn):
        def rounded(x, w, *args, **kw):
            return fn(_RoundF16.apply(x), _RoundF16.apply(w), *args, **kw)
        return rounded
    try:
        for n, fn in saved.items():
            setattr(F, n, wrap(fn))
        yield
    finally:
        for n, fn in saved.items():
            setattr(F, n, fn)


def tensor_class(key):
    """The classes of 1-D parameters of VAE3DLarge, or None for a matrix / kernel."""
    if key.endswith(".weight") and ".bn" not in key:
        return None
    if ".bn" in key:
        return "bn_gamma" if key.endswith(".weight") else "bn_beta"
    return "fc_bias" if key.split(".")[-2] in ("fc_mu", "fc_logvar", "decoder_input") else "conv_bias"


def cos_and_log_ratio(a, b):
    a, b = a.reshape(-1).double(), b.reshape(-1).double()
    return float(a @ b / (a.norm() * b.norm())), float(torch.log(a.norm() / b.norm()))


# How far fp16 conv / linear operands alone move the oracle's 1-D gradients on the test batch (synth_voxels(2, 5), eps seed 1,
# KL weight 0.01): per class the worst tensor's 1 - cosine and |log norm ratio| between the oracle's step as is and under
# `fp16_operands()`.  Measured by tests/test_train_vae_statement_cpu.py, which fails if these drift; the GPU test allows twice this.
FP16_OPERAND_FLOOR = {"conv_bias": (3.95e-3, 2.28e-2), "bn_gamma": (4.55e-3, 2.72e-2), "bn_beta": (4.52e-3, 1.64e-2),
                      "fc_bias": (3.53e-3, 2.74e-3)}
