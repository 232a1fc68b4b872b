"""models/tts/naturalspeech2/diffusion.py on the HIP kernels: the probability-flow ODE solver around the WaveNet (euler and midpoint).

``reverse_diffusion`` knows every step time before its loop, so the WaveNet's step-invariant terms and the step embeddings of all times are
formed once (``WaveNet.prepare``); a step is then the WaveNet's launches and ONE ``amp_ns2_ode_step`` (the element-wise tail of ``cal_dxt`` and
``xt - dxt``; the midpoint solver's first half also forms ``x_mid`` in it).  The step's scalars are formed as the reference forms them, in fp32
torch on a one-element tensor, on the host: there is no per-step host synchronisation.  The op-level range flag is read once, after the last
step (``AmpError`` with AMP_ERR_RANGE, as the other models raise it)."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.tts.naturalspeech2.wavenet import WaveNet
from amphion_amd.modules.hip_ops import ns2_ode_step


def step_times(n_timesteps, midpoint):
    """the fp32 step times of the reference's loop, ``(1.0 - (i + 0.5) * h) * ones`` and, for midpoint, ``t + 0.5 * h``, as Python floats"""
    h = 1.0 / max(n_timesteps, 1)
    one = torch.ones(1, dtype=torch.float32)
    out = []
    for i in range(n_timesteps):
        t = (1.0 - (i + 0.5) * h) * one
        out.append(float(t))
        if midpoint:
            out.append(float(t + 0.5 * h))
    return out, h


def _check_inputs(z, x_mask, cond, spk_query_emb, who):
    if x_mask is not None:
        raise NotImplementedError(f"{who}: x_mask is the training path; the reference's inference passes None")
    z = _lib.require_device_tensor(z, f"{who} input")
    cond = _lib.require_device_tensor(cond, f"{who} condition")
    spk = _lib.require_device_tensor(spk_query_emb, f"{who} speaker queries")
    if z.dim() != 3 or cond.dim() != 3 or spk.dim() != 3 or cond.shape[0] != z.shape[0] or cond.shape[1] != z.shape[2] or spk.shape[0] != z.shape[0]:
        raise ValueError(f"{who}: expected z [B, latent, T], cond [B, T, d] and spk_query_emb [B, Q, d], got {tuple(z.shape)}, {tuple(cond.shape)}, "
                         f"{tuple(spk.shape)}")
    return z, cond.transpose(1, 2).contiguous(), spk.transpose(1, 2).contiguous()


class Diffusion(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.diff_estimator = WaveNet(cfg.wavenet)
        self.beta_min, self.beta_max, self.sigma, self.noise_factor = cfg.beta_min, cfg.beta_max, cfg.sigma, cfg.noise_factor
        if cfg.ode_solver not in ("euler", "midpoint"):
            raise ValueError(f"Diffusion: ode_solver must be 'euler' or 'midpoint', got {cfg.ode_solver!r}")

    def forward(self, x, x_mask, cond, spk_query_emb, offset=1e-5):
        raise NotImplementedError("Diffusion.forward is the training path: not on the HIP path")

    @torch.no_grad()
    def get_cum_beta(self, time_step):
        return self.beta_min * time_step + 0.5 * (self.beta_max - self.beta_min) * (time_step ** 2)

    @torch.no_grad()
    def get_beta_t(self, time_step):
        return self.beta_min + (self.beta_max - self.beta_min) * time_step

    def scalars(self, t, h):
        """exp(-cum_beta / (2 sigma^2)), the variance, h * beta_t and 1 / sigma^2 at time t (a Python float holding an fp32 value): each formed
        as ``cal_dxt`` forms it, in fp32 torch on a one-element tensor"""
        ts = torch.tensor([t], dtype=torch.float32)
        cum_beta, beta_t = self.get_cum_beta(ts), self.get_beta_t(ts)
        s2 = self.sigma ** 2
        return (float(torch.exp(-0.5 * cum_beta / s2)), float(s2 * (1.0 - torch.exp(-cum_beta / s2))), float(h * beta_t),
                float(torch.tensor(1.0 / s2, dtype=torch.float32)))

    @torch.no_grad()
    def cal_dxt(self, xt, x_mask, cond, spk_query_emb, diffusion_step, h):
        """one evaluation at one time for the whole batch (read on the host) -> dxt; ``reverse_diffusion`` does not go through here"""
        xt, c, spk = _check_inputs(xt, x_mask, cond, spk_query_emb, "Diffusion.cal_dxt")
        t = float(diffusion_step.detach().float().reshape(-1)[0].cpu())
        with _lib.on_device(xt.device):
            state = self.diff_estimator.prepare(c, spk, [t])
            x0 = self.diff_estimator.step(state, xt, 0)
            return xt - ns2_ode_step(xt, x0, xt, *self.scalars(t, h))

    @torch.no_grad()
    def reverse_diffusion(self, z, x_mask, cond, n_timesteps, spk_query_emb):
        """z [B, latent, T], cond [B, T, d], spk_query_emb [B, Q, d] -> x0 [B, latent, T]"""
        z, c, spk = _check_inputs(z, x_mask, cond, spk_query_emb, "Diffusion.reverse_diffusion")
        mid = self.cfg.ode_solver == "midpoint"
        times, h = step_times(int(n_timesteps), mid)
        wn = self.diff_estimator
        with _lib.on_device(z.device):
            xt = z.clone()
            if times:
                state = wn.prepare(c, spk, times)
            x_mid = torch.empty_like(xt) if mid else None
            for i in range(int(n_timesteps)):
                if not mid:
                    ns2_ode_step(xt, wn.step(state, xt, i), xt, *self.scalars(times[i], h), out=xt)
                    continue
                ns2_ode_step(xt, wn.step(state, xt, 2 * i), xt, *self.scalars(times[2 * i], h), midpoint_half=True, out=x_mid)
                ns2_ode_step(x_mid, wn.step(state, x_mid, 2 * i + 1), xt, *self.scalars(times[2 * i + 1], h), out=xt)
            _lib.range_check(z.device)
        return xt

    @torch.no_grad()
    def reverse_diffusion_from_t(self, z, x_mask, cond, n_timesteps, spk_query_emb, t_start):
        raise NotImplementedError("Diffusion.reverse_diffusion_from_t (the reference's debugging entry) is not on the HIP path")
