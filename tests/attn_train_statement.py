"""fp32 torch statement of one training step of the attention denoiser (`UNetAttentionPointExperimental` in train()
mode, F.l1_loss, autograd), built on oracle.torch_oracle's pieces with BatchNorm in train() mode.  Pinned to the
reference by tests/test_train_attention_oracle_cpu.py; the GPU tests use it as their yardstick."""
import torch
import torch.nn.functional as F

from oracle import torch_oracle as O


def leaves_of(sd):
    return {k: v for k, v in sd.items() if v.is_floating_point() and not k.endswith(("running_mean", "running_var"))}


def attention_forward_train(sd, p, x_t, t):
    """eps_hat with every BatchNorm on batch statistics; sd's running statistics are updated in place."""
    O._BN_TRAIN = True
    try:
        with torch.device(x_t.device):          # the oracle's timestep tables are built where the inputs live
            return O.unet_attention(sd, p, x_t, t)
    finally:
        O._BN_TRAIN = False


def attention_training_step(sd, p, x_t, t, noise):
    """Returns (loss, pred, {key: grad}); sd's BatchNorm running statistics are updated in place."""
    work = dict(sd)
    leaves = {}
    for k, v in leaves_of(sd).items():
        leaves[k] = v.detach().clone().requires_grad_(True)
        work[k] = leaves[k]
    with torch.enable_grad():
        pred = attention_forward_train(work, p, x_t, t)
        loss = F.l1_loss(noise, pred)
        loss.backward()
    for k in sd:
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            sd[k] = work[k]
    return loss.detach(), pred.detach(), {k: v.grad for k, v in leaves.items()}
