"""MaskGCT's text-to-semantic model (models/tts/maskgct/maskgct_t2s.py: ``MaskGCT_T2S`` around ``DiffLlamaPrefix``), eval mode, on the gfx950
kernels: ``reverse_diffusion`` follows the reference loop line by line (the launch sequence of a step is maskgct_s2a.py's).  Computed once per
call: ``cond_mlp(phone_emb(phone_id))`` and the prompt's embedding.

One quirk of the reference is kept: the classifier-free branch passes ``phone_mask[:, prompt_len:]`` beside a zero-length phone embedding
(maskgct_t2s.py:301-308).  With P phones <= prompt_len that slice is empty and the branch is the plain path; with P > prompt_len the mask is
longer than the sequence and the reference fails with a shape error -- here a ``ValueError`` that names the condition."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle
from amphion_amd.modules.hip_ops import embed_sum_c

from ._sampler import ExtendedTable, check_codes, decode_tokens, guide
from .llama_nar import DiffLlamaPrefix
from .maskgct_s2a import _reset

_CFG_KEYS = ("hidden_size", "num_layers", "num_heads", "cfg_scale", "cond_codebook_size", "cond_dim", "use_phone_cond")


class MaskGCT_T2S(nn.Module):
    def __init__(self, hidden_size=1024, num_layers=16, num_heads=16, cfg_scale=0.2, cond_codebook_size=8192, cond_dim=1024, use_phone_cond=True,
                 cfg=None):
        super().__init__()
        args = dict(hidden_size=hidden_size, num_layers=num_layers, num_heads=num_heads, cfg_scale=cfg_scale, cond_codebook_size=cond_codebook_size,
                    cond_dim=cond_dim, use_phone_cond=use_phone_cond)
        for k in _CFG_KEYS:                            # maskgct_t2s.py:49-81: an attribute of cfg overrides the argument
            setattr(self, k, getattr(cfg, k) if cfg is not None and hasattr(cfg, k) else args[k])
        self.mask_emb = nn.Embedding(1, self.hidden_size)
        self.to_logit = nn.Linear(self.hidden_size, self.cond_codebook_size)
        self.cond_emb = nn.Embedding(self.cond_codebook_size, self.hidden_size)
        if self.use_phone_cond:
            self.phone_emb = nn.Embedding(1024, self.hidden_size, padding_idx=1023)
        _reset(self)
        self.diff_estimator = DiffLlamaPrefix(hidden_size=self.hidden_size, num_heads=self.num_heads, num_layers=self.num_layers,
                                              use_phone_cond=self.use_phone_cond)
        self._logit_h = _PwHandle()
        self._ext = ExtendedTable()

    def mask_prob(self, t):
        return torch.sin(t * torch.pi / 2).to(t.device)

    def _eval_only(self, name):
        raise NotImplementedError(f"MaskGCT_T2S.{name}: training is not on the HIP path (eval-only scope: reverse_diffusion)")

    def forward_diffusion(self, x0, t):
        self._eval_only("forward_diffusion")

    def loss_t(self, x0, x_mask, t, phone_embedding=None, phone_mask=None):
        self._eval_only("loss_t")

    def compute_loss(self, x0, x_mask, phone_embedding=None, phone_mask=None):
        self._eval_only("compute_loss")

    def forward(self, x0, x_mask, phone_id=None, phone_mask=None):
        self._eval_only("forward")

    def phone_embedding_cf(self, phone_id):
        """``cond_mlp(phone_emb(phone_id))`` channel-first [B, hidden, P]: once per call"""
        est = self.diff_estimator
        return est._cond(est.cond_mlp, embed_sum_c(phone_id[None].contiguous(), [self.phone_emb.weight], None, check=False))

    def prompt_embedding_cf(self, prompt_code):
        """``cond_emb(prompt)`` channel-first [B, hidden, Tp]: once per call"""
        return embed_sum_c(prompt_code[None].contiguous(), [self.cond_emb.weight], None, check=False)

    @torch.no_grad()
    def reverse_diffusion(self, prompt, target_len, phone_id, prompt_mask=None, temp=0.9, filter_thres=0.98, n_timesteps=40, cfg=1.0,
                          rescale_cfg=1.0, *, noise=None, record=None):
        """maskgct_t2s.py:225-363.  prompt [B, Tp] int64 semantic codes, phone_id [B, P] int64 -> the target's semantic codes [B, target_len]
        int64.  ``noise`` (keyword-only, this package's extension): a callable ``noise(shape) -> uniform fp32 tensor`` called in the reference's
        order with its shapes -- [B, T, V] before each non-greedy sample, [B, T] before each re-masking; without it the draws are the device's.
        ``record``: a list that receives every step's guided embeds [B, T, hidden]."""
        if self.training:
            self._eval_only("reverse_diffusion in training mode")
        if not self.use_phone_cond:
            raise NotImplementedError("MaskGCT_T2S.reverse_diffusion needs use_phone_cond (the reference reads self.phone_emb)")
        est = self.diff_estimator
        if not isinstance(prompt, torch.Tensor) or not prompt.is_cuda or prompt.dim() != 2 or prompt.dtype != torch.int64 or prompt.shape[1] < 1 \
                or not isinstance(phone_id, torch.Tensor) or phone_id.device != prompt.device or phone_id.dim() != 2 or phone_id.dtype != torch.int64 \
                or phone_id.shape[0] != prompt.shape[0] or phone_id.shape[1] < 1 or int(target_len) < 1 or int(n_timesteps) < 1:
            raise ValueError("reverse_diffusion: expected int64 prompt [B, Tp] and phone_id [B, P] on one ROCm device (Tp, P >= 1), target_len >= 1 "
                             "and n_timesteps >= 1")
        dev = prompt.device
        B, prompt_len = prompt.shape
        P, seq_len = phone_id.shape[1], int(target_len)
        if cfg > 0 and P > prompt_len:
            raise ValueError(f"reverse_diffusion: with cfg > 0 the reference's unconditional branch passes phone_mask[:, prompt_len:] beside a "
                             f"zero-length phone embedding; with P = {P} phones > prompt_len = {prompt_len} that mask is longer than the sequence "
                             "and the reference fails with a shape error")
        C, V = self.hidden_size, self.cond_codebook_size
        with _lib.on_device(dev):
            key_mask = est._key_mask([None, prompt_mask, None], [P, prompt_len, seq_len], B, dev)
            phone_cf = self.phone_embedding_cf(phone_id)                                    # once per call
            cur_prompt = self.prompt_embedding_cf(prompt)                                   # once per call
            cum = torch.zeros((B, C, seq_len), dtype=torch.float32, device=dev)
            table = self._ext.get(self.cond_emb, self.mask_emb)

            def build_input(idx):
                return embed_sum_c(idx[None], [table], cum, check=False)

            def forwards(cur, t):
                embeds = est.forward_cf(torch.cat([cur_prompt, cur], dim=2), t, key_mask, phone_cf)[:, :, prompt_len:]
                if cfg > 0:                            # the target alone, no phones, every key valid (x_mask is ones)
                    embeds = guide(embeds, est.forward_cf(cur, t, None, None), cfg, rescale_cfg)
                return embeds

            seq = decode_tokens(B, seq_len, int(n_timesteps), V, dev, build_input, forwards, self._logit_h, self.to_logit, temp, filter_thres,
                                noise, record)
            check_codes(dev)
        return seq
