"""models/tts/naturalspeech2/diffusion_flow.py on the HIP kernels: the flow-matching form, ``xt <- xt - h * WaveNet(xt, t)`` along the fixed
step times.  The WaveNet's step-invariant terms and the embeddings of all step times are formed once; the update is a torch ``add_``; the
op-level range flag is read once after the last step."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.tts.naturalspeech2.diffusion import _check_inputs, step_times
from amphion_amd.models.tts.naturalspeech2.wavenet import WaveNet


class DiffusionFlow(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.diff_estimator = WaveNet(cfg.wavenet)
        self.beta_min, self.beta_max, self.sigma, self.noise_factor = cfg.beta_min, cfg.beta_max, cfg.sigma, cfg.noise_factor

    def forward(self, x, x_mask, cond, spk_query_emb, offset=1e-5):
        raise NotImplementedError("DiffusionFlow.forward is the training path: not on the HIP path")

    @torch.no_grad()
    def cal_dxt(self, xt, x_mask, cond, spk_query_emb, diffusion_step, h):
        """one evaluation at one time for the whole batch (read on the host) -> h * flow_pred"""
        xt, c, spk = _check_inputs(xt, x_mask, cond, spk_query_emb, "DiffusionFlow.cal_dxt")
        t = float(diffusion_step.detach().float().reshape(-1)[0].cpu())
        with _lib.on_device(xt.device):
            state = self.diff_estimator.prepare(c, spk, [t])
            return h * self.diff_estimator.step(state, xt, 0)

    @torch.no_grad()
    def reverse_diffusion(self, z, x_mask, cond, n_timesteps, spk_query_emb):
        """z [B, latent, T], cond [B, T, d], spk_query_emb [B, Q, d] -> x0 [B, latent, T]"""
        z, c, spk = _check_inputs(z, x_mask, cond, spk_query_emb, "DiffusionFlow.reverse_diffusion")
        n = int(n_timesteps)
        if n < 1:
            raise ValueError("DiffusionFlow.reverse_diffusion: n_timesteps must be at least 1 (the reference divides by it)")
        times, h = step_times(n, False)
        wn = self.diff_estimator
        with _lib.on_device(z.device):
            xt = z.clone()
            state = wn.prepare(c, spk, times)
            for i in range(n):
                xt.add_(wn.step(state, xt, i), alpha=-h)
            _lib.range_check(z.device)
        return xt
