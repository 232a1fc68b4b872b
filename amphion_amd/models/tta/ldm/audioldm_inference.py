"""The sampling loop of AudioLDM (models/tta/ldm/audioldm_inference.py:133-169) around the HIP UNet, and the decode that follows.

The scheduler is the caller's: any object with diffusers' ``set_timesteps`` / ``timesteps`` / ``scale_model_input`` / ``step(...).prev_sample``
(the reference builds a ``PNDMScheduler``).  Its arithmetic and the guidance on the 780-element latent stay torch ops.  The T5 text encoder,
the file handling and the vocoder hand-off are the caller's too: ``text_embeddings`` is [uncond; text]."""
from __future__ import annotations

import torch


@torch.no_grad()
def generate_latents(model, text_embeddings, scheduler, num_steps, guidance_scale, latents):
    """``latents`` [1, z_channels, H, W] (the caller's draw) -> the denoised latents after ``num_steps`` scheduler steps of classifier-free
    guidance with ``text_embeddings`` [2, Tk, context_dim] = [uncond; text]"""
    model.eval()
    scheduler.set_timesteps(num_steps)
    for t in scheduler.timesteps:
        t = t.to(latents.device)
        latent_model_input = torch.cat([latents] * 2)
        latent_model_input = scheduler.scale_model_input(latent_model_input, timestep=t)
        noise_pred = model(latent_model_input, torch.cat([t.unsqueeze(0)] * 2), text_embeddings)
        noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
        noise_pred = noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond)
        latents = scheduler.step(noise_pred, t, latents).prev_sample
    return latents


@torch.no_grad()
def text_to_mel(model, autoencoderkl, text_embeddings, scheduler, num_steps, guidance_scale, latents):
    """``generate_latents`` followed by ``AutoencoderKL.decode``: -> the mel [1, 1, 16 H, 16 W] the vocoder takes"""
    return autoencoderkl.decode(generate_latents(model, text_embeddings, scheduler, num_steps, guidance_scale, latents))
