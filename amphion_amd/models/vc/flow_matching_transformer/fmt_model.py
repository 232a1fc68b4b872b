"""Vevo's flow-matching transformer (models/vc/flow_matching_transformer/fmt_model.py: ``FlowMatchingTransformer``): the sampler
``reverse_diffusion`` around ``DiffLlama`` on the gfx950 kernels.  Same constructor arguments (the ``cfg=`` overrides included) and
``state_dict`` keys (``cond_emb.weight``, ``diff_estimator.*``); ``cond_emb`` stays an ``nn.Embedding`` / ``nn.Linear`` because callers invoke
it directly (models/vc/vevo/vevo_utils.py:554-563).

Two computations leave the Euler loop, both with the bits of the per-step recomputation: ``cond_mlp(cond)`` is computed once per call, and the
classifier-free branch's ``cond_mlp(0)`` once, as a single column.  The per-step combination (classifier-free guidance, the std rescale, the
Euler update) is [B, T, mel]-sized and stays in torch on the device.  Training (``forward``, ``compute_loss``, ``loss_t``,
``forward_diffusion``) is outside the HIP path."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd import _lib

from .llama_nar import DiffLlama

_CFG_KEYS = ("mel_dim", "hidden_size", "num_layers", "num_heads", "cfg_scale", "use_cond_code", "cond_codebook_size", "cond_dim", "time_scheduler",
             "sigma", "cond_scale_factor")


class FlowMatchingTransformer(nn.Module):
    def __init__(self, mel_dim=100, hidden_size=1024, num_layers=12, num_heads=16, cfg_scale=0.2, use_cond_code=True, cond_codebook_size=1024,
                 cond_dim=1024, cond_scale_factor=1, sigma=1e-5, time_scheduler="linear", cfg=None):
        super().__init__()
        self.cfg = cfg
        args = dict(mel_dim=mel_dim, hidden_size=hidden_size, num_layers=num_layers, num_heads=num_heads, cfg_scale=cfg_scale,
                    use_cond_code=use_cond_code, cond_codebook_size=cond_codebook_size, cond_dim=cond_dim, time_scheduler=time_scheduler, sigma=sigma,
                    cond_scale_factor=cond_scale_factor)
        for k in _CFG_KEYS:                            # fmt_model.py:32-90: an attribute of cfg overrides the argument
            setattr(self, k, getattr(cfg, k) if cfg is not None and hasattr(cfg, k) else args[k])
        if self.use_cond_code:
            self.cond_emb = nn.Embedding(self.cond_codebook_size, self.hidden_size)
        else:
            self.cond_emb = nn.Linear(self.cond_dim, self.hidden_size)
        self.reset_parameters()
        self.diff_estimator = DiffLlama(mel_dim=self.mel_dim, hidden_size=self.hidden_size, num_heads=self.num_heads, num_layers=self.num_layers)

    def reset_parameters(self):
        """fmt_model.py:190-226 for the modules this class holds when it runs (``cond_emb``; the estimator is built afterwards)"""
        for m in self.modules():
            if isinstance(m, nn.Linear):
                m.weight.data.normal_(mean=0.0, std=0.02)
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.Embedding):
                m.weight.data.normal_(mean=0.0, std=0.02)

    def _training_only(self, name):
        raise NotImplementedError(f"FlowMatchingTransformer.{name}: training is not on the HIP path (eval-only scope: reverse_diffusion)")

    def forward_diffusion(self, x, t):
        self._training_only("forward_diffusion")

    def loss_t(self, x, x_mask, t, cond=None):
        self._training_only("loss_t")

    def compute_loss(self, x, x_mask, cond=None):
        self._training_only("compute_loss")

    def forward(self, x, x_mask, cond_code=None, cond_feature=None):
        self._training_only("forward")

    @torch.no_grad()
    def reverse_diffusion(self, cond, prompt, x_mask=None, prompt_mask=None, n_timesteps=10, cfg=1.0, rescale_cfg=0.75, *, noise=None):
        """fmt_model.py:228-283.  cond [B, Tp + Tt, hidden] (``cond_emb`` of the codes), prompt [B, Tp, mel] -> the target mel [B, Tt, mel].
        ``noise`` (keyword-only, this package's one extension) replaces the ``torch.randn`` start [B, Tt, mel]."""
        est = self.diff_estimator
        cond = _lib.require_device_tensor(cond, "reverse_diffusion cond")
        prompt = _lib.require_device_tensor(prompt, "reverse_diffusion prompt")
        if cond.dim() != 3 or prompt.dim() != 3 or cond.shape[0] != prompt.shape[0] or cond.shape[2] != self.hidden_size \
                or prompt.shape[2] != self.mel_dim or cond.shape[1] <= prompt.shape[1] or cond.device != prompt.device:
            raise ValueError(f"reverse_diffusion: expected cond [B, Tp + Tt, {self.hidden_size}] and prompt [B, Tp, {self.mel_dim}] with Tt >= 1 on one "
                             f"device, got {tuple(cond.shape)} on {cond.device} and {tuple(prompt.shape)} on {prompt.device}")
        if int(n_timesteps) < 1:
            raise ValueError(f"reverse_diffusion: n_timesteps={n_timesteps}")
        B, dev = cond.shape[0], cond.device
        step = 1.0 / n_timesteps
        prompt_len = prompt.shape[1]
        target_len = cond.shape[1] - prompt_len
        with _lib.on_device(dev):
            xt_mask = None                             # no mask given: every key is valid, as the reference's masks of ones say
            if x_mask is not None or prompt_mask is not None:
                if x_mask is None:
                    x_mask = torch.ones(B, target_len, device=dev)
                if prompt_mask is None:
                    prompt_mask = torch.ones(B, prompt_len, device=dev)
                xt_mask = torch.cat([prompt_mask, x_mask], dim=1)
            if noise is None:
                z = torch.randn((B, target_len, self.mel_dim), dtype=cond.dtype, device=dev, requires_grad=False)
            else:
                z = _lib.require_device_tensor(noise, "reverse_diffusion noise")
                if tuple(z.shape) != (B, target_len, self.mel_dim) or z.device != dev:
                    raise ValueError(f"reverse_diffusion: noise must be {(B, target_len, self.mel_dim)} on {dev}, got {tuple(z.shape)} on {z.device}")
            cond_cf = est.cond_embedding_cf(cond)                                               # once per call, not per step
            uncond_cf = est.zero_cond_embedding_cf(B, target_len, dev) if cfg > 0 else None     # cond_mlp(0): one column
            xt = z
            for i in range(n_timesteps):               # Euler steps at the midpoint times, from x0 = z ~ N(0, 1) at t = 0 to t = 1
                t = (0 + (i + 0.5) * step) * torch.ones(B, dtype=z.dtype, device=dev)
                flow = est(torch.cat([prompt, xt], dim=1), t, None, xt_mask, cond_embedding_cf=cond_cf)[:, prompt_len:, :]
                if cfg > 0:                            # classifier-free guidance on the target part alone, then the std rescale
                    uncond = est(xt, t, None, x_mask, cond_embedding_cf=uncond_cf)
                    pos_std = flow.std()               # over the whole tensor, batch included, unbiased
                    guided = flow + cfg * (flow - uncond)
                    flow = rescale_cfg * (guided * pos_std / guided.std()) + (1 - rescale_cfg) * guided
                xt = xt + flow * step
        return xt
