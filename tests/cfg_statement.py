"""The float statement of class conditioning with classifier-free guidance (Ho & Salimans) over the CPU oracle network.

The class term: temb_b = time_mlp(sinusoid(t_b)) + E[label_b], E the (num_classes + 1, dim) embedding table whose last row is
the null class.  The oracle is not edited: while a statement function runs, `oracle.torch_oracle.time_mlp` is replaced by a
wrapper that adds E[labels] to its result (restored in `finally`).  E may be an autograd leaf, so `training_step` yields its
gradient.  Guidance: eps = eps_u + w (eps_c - eps_u) per shape, in this operation order in fp32; when every scale is exactly 1
the unconditional forward does not run and eps = eps_c.  The guided samplers are the oracle's `ddim_sample` / `ddpm_sample` and
tests/dpm_statement.py over that model."""
import contextlib

import torch

import dpm_statement
from oracle import torch_oracle as O


@contextlib.contextmanager
def class_term(E, labels):
    """Inside, the oracle's time_mlp returns time_mlp(emb) + E[labels]."""
    inner = O.time_mlp
    idx = torch.as_tensor(labels, dtype=torch.long)

    def time_mlp(sd, p, emb):
        return inner(sd, p, emb) + E[idx]

    O.time_mlp = time_mlp
    try:
        yield
    finally:
        O.time_mlp = inner


def eps_of(sd, p, E, labels, x, t, **kw):
    """The class-conditional network: O.unet_pointnet_large with the class term."""
    with class_term(E, labels):
        return O.unet_pointnet_large(sd, p, x, t, **kw)


def guided_model(sd, p, E, labels, scale=1.0):
    """model(x, t) of the samplers: labels (B,) in [0, num_classes], scale a number or (B,)."""
    labels = torch.as_tensor(labels, dtype=torch.long)
    w = torch.as_tensor(scale, dtype=torch.float32).reshape(-1)
    null = torch.full_like(labels, E.shape[0] - 1)

    def model(x, t):
        ec = eps_of(sd, p, E, labels, x, t)
        if bool((w == 1.0).all()):
            return ec
        eu = eps_of(sd, p, E, null, x, t)
        d = ec - eu
        return eu + O._bc(w.expand(x.shape[0]), x) * d

    return model


def sample(kind, sd, p, E, labels, scale, x_T, steps, noises=None):
    """kind 'ddim' | 'ddpm' | 'dpm': the last x_0 of the guided sampler."""
    model = guided_model(sd, p, E, labels, scale)
    with torch.no_grad():
        if kind == "ddim":
            return O.ddim_sample(model, x_T, steps)
        if kind == "ddpm":
            return O.ddpm_sample(model, x_T, steps, noises)
        return dpm_statement.sample_dpm(model, x_T, steps)


def training_step(sd, p, E, labels, x_t, t, noise):
    """O.point_training_step with the class term: (loss, pred-free gradient dict incl. p + 'class_emb.weight').  sd holds no
    class_emb entry; its BatchNorm running statistics are updated in place."""
    E = E.detach().clone().requires_grad_(True)
    with class_term(E, labels):
        loss, grads = O.point_training_step(sd, p, x_t, t, noise)
    grads[p + "class_emb.weight"] = E.grad
    return loss, grads
