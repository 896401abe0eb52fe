"""Capture tests/golden/train_attention.npz: one training step of the reference's PointCloudDiffusion with the attention
denoiser (`UNetAttentionPointExperimental`, networks.py:597-722, wired in place of diffusion.py:28's UNetPointNetLarge:
the reference's one-import change) in train() mode -- add_noise, F.l1_loss, autograd, one torch.optim.AdamW step
(diffusion.py:60,70-86,170-186).  Run in the build container (imports the reference through oracle/ref_shim):

    python tools/make_golden_train_attention.py

Layout as G13 (`oracle/make_golden.py train`): inputs, loss, prediction, per-parameter gradient digests
(norm, sum, 64 hash-chosen entries), BatchNorm running statistics after the step, parameter digests after AdamW."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from oracle.make_golden import ATTN_GAIN, OUT, T, grad_digest, synth_cloud  # noqa: E402
from shapegen_amd import specs  # noqa: E402

B, N = 2, 256


def main():
    rd, rn, _, _ = ref_shim.load_reference()
    torch.manual_seed(0)
    pcd = rd.PointCloudDiffusion(num_points=N)
    pcd.model = rn.UNetAttentionPointExperimental(N, dim=256, time_dim=256)
    sd = specs.synth_state_dict(specs.unet_attention_spec(), seed=0, gain=ATTN_GAIN)      # tests/helpers.una_sd()
    pcd.load_state_dict(T({"model." + k: v for k, v in sd.items()}), strict=True)
    pcd.train()
    x0 = torch.from_numpy(synth_cloud(B, N, 33))
    t = torch.tensor([0.3, 0.75])
    torch.manual_seed(7)
    noise_replay = torch.randn_like(x0)
    torch.manual_seed(7)
    with torch.enable_grad():
        x_t, noise, _, _ = pcd.add_noise(x0, t)
        assert torch.equal(noise, noise_replay)
        pred = pcd.model(x_t, t)
        loss = torch.nn.functional.l1_loss(noise, pred)
        opt = torch.optim.AdamW(pcd.parameters(), lr=pcd.lr, weight_decay=1e-5)
        opt.zero_grad()
        loss.backward()
    g = {"x0": x0.numpy(), "t": t.numpy(), "noise": noise.numpy(), "x_t": x_t.detach().numpy(), "loss": loss.item(),
         "pred": pred.detach().numpy()}
    names = []
    for k, prm in pcd.named_parameters():
        g["grad." + k] = grad_digest(k, prm.grad)[0]
        names.append(k)
    opt.step()
    for k, prm in pcd.named_parameters():
        flat = prm.detach().reshape(-1).double()
        idx = (np.abs(specs.hash_uniform("digest." + k, 64, 7)) * (flat.numel() - 1)).astype(np.int64)
        g["param1." + k] = flat[torch.from_numpy(idx)].numpy()
    for k, v in pcd.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            g["buf1." + k] = v.numpy()
    g["param_names"] = np.array(names)
    path = os.path.join(OUT, "train_attention.npz")
    np.savez_compressed(path, **g)
    print("train_attention.npz", os.path.getsize(path), "bytes, loss", loss.item(), "entries", len(g))


if __name__ == "__main__":
    main()
