"""Writes golden_tta.npz, keys_tta.json and keys_autoencoderkl.json from the REAL classes of the reference on the CPU:

    python tests/golden/make_golden_tta.py <amphion root>

``models.tta.ldm.audioldm.AudioLDM`` (small UNet: tests/tta_ref.py small_hp) on two inputs, each with a 3-step guided sampling loop through the real model
under the test scheduler, and ``models.tta.autoencoder.autoencoder.AutoencoderKL.decode`` (ch 32) on three latents.  The reference imports
``omegaconf.listconfig.ListConfig`` for a type test only; a stand-in serves.  Its ``zero_module`` layers leave ``__init__`` at zero (the UNet's
output would be exactly 0), so every weight is re-drawn from the seed (tta_ref.synth_state_dict).  The npz holds seeds, inputs and outputs only:
the weights regenerate from the seed."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import tta_ref as R  # noqa: E402

SEED, VAE_SEED, STEPS, GUIDANCE = 20261, 20262, 3, 3.0
UNET_INPUTS = {"a": (5, 39, 7), "b": (4, 8, 5)}              # name -> (H, W, context tokens)
VAE_INPUTS = {"a": (5, 7), "b": (2, 3), "c": (4, 8)}


def sample(model, text_embeddings, scheduler, num_steps, guidance_scale, latents):
    """the loop of the reference's inference (audioldm_inference.py:133-169) around the REAL model, stated here so that the golden does not
    depend on the package's ``generate_latents``, which it checks"""
    scheduler.set_timesteps(num_steps)
    for t in scheduler.timesteps:
        x2 = scheduler.scale_model_input(torch.cat([latents, latents]), timestep=t)
        eps = model(x2, torch.stack([t, t]), text_embeddings)
        eps_uncond, eps_text = eps[:1], eps[1:]
        latents = scheduler.step(eps_uncond + guidance_scale * (eps_text - eps_uncond), t, latents).prev_sample
    return latents


def main(root):
    sys.path.insert(0, root)
    oc, lc = types.ModuleType("omegaconf"), types.ModuleType("omegaconf.listconfig")

    class ListConfig(list):
        pass

    lc.ListConfig, oc.listconfig = ListConfig, lc
    sys.modules["omegaconf"], sys.modules["omegaconf.listconfig"] = oc, lc
    from models.tta.autoencoder.autoencoder import AutoencoderKL
    from models.tta.ldm.audioldm import AudioLDM

    out = {"seed": np.int64(SEED), "vae_seed": np.int64(VAE_SEED), "steps": np.int64(STEPS), "guidance": np.float64(GUIDANCE)}
    hp = R.small_hp()
    model = AudioLDM(R.Cfg(hp)).eval()
    keys = list(model.state_dict().keys())
    model.load_state_dict(R.synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, SEED))
    for name, (H, W, Tk) in UNET_INPUTS.items():
        g = torch.Generator().manual_seed(SEED + H * W)
        x = torch.randn(2, 4, H, W, generator=g)
        t = torch.tensor([731, 12])
        ctx = torch.randn(2, Tk, hp["context_dim"], generator=g)
        lat = torch.randn(1, 4, H, W, generator=g)
        with torch.no_grad():
            y = model(x, t, ctx)
            sch = R.TestScheduler()
            lat_out = sample(model, ctx, sch, STEPS, GUIDANCE, lat)
        assert float(y.abs().max()) > 1e-3
        for k, v in (("x", x), ("t", t), ("ctx", ctx), ("y", y), ("lat", lat), ("lat_out", lat_out)):
            out[f"unet_{name}_{k}"] = v.numpy()
    vhp = R.small_vae_hp()
    vae = AutoencoderKL(R.Cfg(vhp)).eval()
    vkeys = list(vae.state_dict().keys())
    vae.load_state_dict(R.synth_state_dict({k: v.shape for k, v in vae.state_dict().items()}, VAE_SEED))
    for name, (H, W) in VAE_INPUTS.items():
        z = torch.randn(1, 4, H, W, generator=torch.Generator().manual_seed(VAE_SEED + H * W))
        with torch.no_grad():
            mel = vae.decode(z)
        out[f"vae_{name}_z"], out[f"vae_{name}_mel"] = z.numpy(), mel.numpy()
    np.savez_compressed(os.path.join(HERE, "golden_tta.npz"), **out)
    with open(os.path.join(HERE, "keys_tta.json"), "w") as f:
        json.dump(keys, f, indent=0)
    with open(os.path.join(HERE, "keys_autoencoderkl.json"), "w") as f:
        json.dump(vkeys, f, indent=0)
    print("wrote", len(out), "arrays,", len(keys), "+", len(vkeys), "keys")


if __name__ == "__main__":
    main(sys.argv[1])
