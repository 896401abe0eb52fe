"""The float statement of class conditioning with classifier-free guidance in latent space, over the CPU oracle's latent
denoiser.

The class term is tests/cfg_statement.py's: te_b = time_mlp(sinusoid(t_b)) + E[label_b], E the (num_classes + 1, time_dim)
table whose last row is the null class, patched into `oracle.torch_oracle.time_mlp` by `cfg_statement.class_term` while a
statement function runs (`O.latent_unet` and `O.latent_training_step` call it too).  Guidance: eps = eps_u + w (eps_c - eps_u) per
shape, in this operation order in fp32; when every scale is exactly 1 the unconditional forward does not run.  The samplers
are the oracle's `ddim_sample`, `ddpm_sample`, `ddim_from_state` and tests/dpm_statement.py over that model."""
import torch

import dpm_statement
from cfg_statement import class_term
from oracle import torch_oracle as O


def eps_of(sd, p, E, labels, z, t, **kw):
    """The class-conditional latent denoiser: O.latent_unet with the class term."""
    with class_term(E, labels):
        return O.latent_unet(sd, p, z, t, **kw)


def guided_model(sd, p, E, labels, scale=1.0):
    """model(z, t) of the samplers: labels (B,) in [0, num_classes], scale a number or (B,)."""
    labels = torch.as_tensor(labels, dtype=torch.long)
    w = torch.as_tensor(scale, dtype=torch.float32).reshape(-1)
    null = torch.full_like(labels, E.shape[0] - 1)

    def model(z, t):
        ec = eps_of(sd, p, E, labels, z, t)
        if bool((w == 1.0).all()):
            return ec
        eu = eps_of(sd, p, E, null, z, t)
        d = ec - eu
        return eu + O._bc(w.expand(z.shape[0]), z) * d

    return model


def sample(kind, sd, p, E, labels, scale, z_T, steps, noises=None, start_t=None):
    """kind 'ddim' | 'ddpm' | 'dpm' | 'state' (`ddim_from_state` from z_T at start_t): the last z_0 of the guided sampler."""
    model = guided_model(sd, p, E, labels, scale)
    with torch.no_grad():
        if kind == "ddim":
            return O.ddim_sample(model, z_T, steps)
        if kind == "ddpm":
            return O.ddpm_sample(model, z_T, steps, noises)
        if kind == "state":
            return O.ddim_from_state(model, z_T, start_t, steps)
        return dpm_statement.sample_dpm(model, z_T, steps)


def training_step(sd, p, E, labels, z_t, t, noise, dropout_mask):
    """O.latent_training_step with the class term: (loss, prediction, gradient dict incl. p + 'class_emb.weight').  sd holds no
    class_emb entry."""
    E = E.detach().clone().requires_grad_(True)
    with class_term(E, labels):
        loss, pred, grads = O.latent_training_step(sd, p, z_t, t, noise, dropout_mask)
    grads[p + "class_emb.weight"] = E.grad
    return loss, pred, grads
