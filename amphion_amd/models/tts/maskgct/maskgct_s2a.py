"""MaskGCT's semantic-to-acoustic model (models/tts/maskgct/maskgct_s2a.py: ``MaskGCT_S2A`` around ``DiffLlama``), eval mode, on the gfx950
kernels: ``reverse_diffusion`` follows the reference loop line by line.  Per step: one ``amp_embed_sum_c`` builds the input, the conditional
and the unconditional forward run, the guidance arithmetic is torch on [B, hidden, T], one pointwise GEMM gives the logits channel-first, one
``amp_mask_sample`` the ids and their confidence, and the [B, T]-sized re-masking is torch.  What does not change over the steps is computed
once: ``cond_mlp(cond + layer_emb)`` per layer and the prompt's embedding sum per call."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle

from ._sampler import ExtendedTable, check_codes, decode_tokens, embed_sum_chain, guide
from .llama_nar import DiffLlama

_CFG_KEYS = ("num_quantizer", "hidden_size", "num_layers", "num_heads", "codebook_size", "cfg_scale", "mask_layer_schedule", "cond_codebook_size",
             "cond_dim", "predict_layer_1")


def _reset(module):
    """``reset_parameters`` for the modules the class holds when it runs (the estimator is built afterwards)"""
    for m in module.modules():
        if isinstance(m, nn.Linear):
            m.weight.data.normal_(mean=0.0, std=0.02)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.Embedding):
            m.weight.data.normal_(mean=0.0, std=0.02)
            if m.padding_idx is not None:
                m.weight.data[m.padding_idx].zero_()


class MaskGCT_S2A(nn.Module):
    def __init__(self, num_quantizer=12, hidden_size=1024, num_layers=16, num_heads=16, codebook_size=1024, cfg_scale=0.15,
                 mask_layer_schedule="linear", cond_codebook_size=1024, cond_dim=1024, predict_layer_1=True, cfg=None):
        super().__init__()
        args = dict(num_quantizer=num_quantizer, hidden_size=hidden_size, num_layers=num_layers, num_heads=num_heads, codebook_size=codebook_size,
                    cfg_scale=cfg_scale, mask_layer_schedule=mask_layer_schedule, cond_codebook_size=cond_codebook_size, cond_dim=cond_dim,
                    predict_layer_1=predict_layer_1)
        for k in _CFG_KEYS:                            # maskgct_s2a.py:52-99: an attribute of cfg overrides the argument
            setattr(self, k, getattr(cfg, k) if cfg is not None and hasattr(cfg, k) else args[k])
        self.layer_emb = nn.Embedding(self.num_quantizer, self.hidden_size)
        self.mask_emb = nn.Embedding(1, self.hidden_size)
        self.token_emb = nn.ModuleList([nn.Embedding(self.codebook_size, self.hidden_size) for _ in range(self.num_quantizer)])
        self.to_logits = nn.ModuleList([nn.Linear(self.hidden_size, self.codebook_size) for _ in range(self.num_quantizer)])
        self.cond_emb = nn.Embedding(self.cond_codebook_size, self.hidden_size)
        _reset(self)
        self.diff_estimator = DiffLlama(hidden_size=self.hidden_size, num_heads=self.num_heads, num_layers=self.num_layers)
        self._logit_h = [_PwHandle() for _ in range(self.num_quantizer)]
        self._ext = [ExtendedTable() for _ in range(self.num_quantizer)]

    def mask_prob(self, t):
        return torch.sin(t * torch.pi / 2).to(t.device)

    def _eval_only(self, name):
        raise NotImplementedError(f"MaskGCT_S2A.{name}: training is not on the HIP path (eval-only scope: reverse_diffusion)")

    def mask_layer(self, t):
        self._eval_only("mask_layer")

    def forward_diffusion(self, x0, t):
        self._eval_only("forward_diffusion")

    def loss_t(self, x0, x_mask, t, cond=None):
        self._eval_only("loss_t")

    def compute_loss(self, x0, x_mask, cond=None):
        self._eval_only("compute_loss")

    def forward(self, x0, x_mask, cond_code=None):
        self._eval_only("forward")

    def prompt_embedding_cf(self, prompt_code):
        """sum over the quantizers of ``token_emb[i](prompt[:, :, i])``, channel-first [B, hidden, Tp]: once per call"""
        codes = prompt_code.permute(2, 0, 1).contiguous()
        return embed_sum_chain(codes, [e.weight for e in self.token_emb])

    def layer_cond_cf(self, cond, layer):
        """``cond_mlp(cond + layer_emb(layer))`` channel-first [B, hidden, Tp + Tt]: once per layer"""
        return self.diff_estimator.cond_embedding_cf(cond + self.layer_emb.weight[layer][None, None, :])

    @torch.no_grad()
    def reverse_diffusion(self, cond, prompt, x_mask=None, prompt_mask=None, temp=1.5, filter_thres=0.98, max_layer=None, gt_code=None,
                          n_timesteps=[10, 4, 4, 4, 4, 4, 4, 4], cfg=1.0, rescale_cfg=1.0, *, noise=None, record=None):
        """maskgct_s2a.py:317-469.  cond [B, Tp + Tt, hidden] (``cond_emb`` of the semantic codes), prompt [B, Tp, num_quantizer] int64 ->
        the target's acoustic codes [B, Tt, max_layer] int64.  ``noise`` (keyword-only, this package's extension): a callable
        ``noise(shape) -> uniform fp32 tensor`` called in the reference's order with its shapes -- [B, Tt, V] before each non-greedy sample,
        [B, Tt] before each re-masking; without it the draws are the device's.  ``record``: a list that receives every step's guided embeds
        [B, Tt, hidden]."""
        if self.training:
            self._eval_only("reverse_diffusion in training mode")
        assert len(n_timesteps) == self.num_quantizer
        est = self.diff_estimator
        cond = _lib.require_device_tensor(cond, "reverse_diffusion cond")
        dev = cond.device
        if cond.dim() != 3 or cond.shape[2] != self.hidden_size or not isinstance(prompt, torch.Tensor) or prompt.dim() != 3 \
                or prompt.shape[0] != cond.shape[0] or prompt.shape[2] != self.num_quantizer or prompt.device != dev or prompt.dtype != torch.int64 \
                or not 0 < prompt.shape[1] < cond.shape[1]:
            raise ValueError(f"reverse_diffusion: expected cond [B, Tp + Tt, {self.hidden_size}] and int64 prompt [B, Tp, {self.num_quantizer}] with "
                             f"Tp, Tt >= 1 on one device, got {tuple(cond.shape)} and {tuple(getattr(prompt, 'shape', ()))}")
        B, prompt_len = prompt.shape[0], prompt.shape[1]
        seq_len = cond.shape[1] - prompt_len
        C, V = self.hidden_size, self.codebook_size
        max_layer = self.num_quantizer if max_layer is None else max_layer
        with _lib.on_device(dev):
            key_mask = est._key_mask([prompt_mask, x_mask], [prompt_len, seq_len], B, dev)
            x_key_mask = None if key_mask is None else key_mask[:, prompt_len:].contiguous()
            cum = torch.zeros((B, C, seq_len), dtype=torch.float32, device=dev)
            xt = torch.zeros((B, seq_len, max_layer), dtype=torch.int64, device=dev)
            gt_layer = 0
            if gt_code is not None:
                gt_layer = gt_code.shape[-1]
                xt[:, :, :gt_layer] = gt_code
                cum = embed_sum_chain(gt_code.to(dev).permute(2, 0, 1).contiguous(), [e.weight for e in self.token_emb[:gt_layer]], cum)
            cur_prompt = self.prompt_embedding_cf(prompt)                                   # once per call
            mask_token = self.mask_emb.weight[0]
            for layer in range(gt_layer, max_layer):
                cond_cf = self.layer_cond_cf(cond, layer)                                   # once per layer
                uncond_cf = cond_cf[:, :, prompt_len:].contiguous() if cfg > 0 else None
                table = self._ext[layer].get(self.token_emb[layer], self.mask_emb)
                extra = (mask_token * float(max_layer - 1 - layer))[None, :, None]
                layer_cum = cum

                def build_input(idx):
                    return embed_sum_chain(idx[None], [table], layer_cum) + extra

                def forwards(cur, t):
                    embeds = est.forward_cf(torch.cat([cur_prompt, cur], dim=2), t, cond_cf, key_mask)[:, :, prompt_len:]
                    if cfg > 0:
                        embeds = guide(embeds, est.forward_cf(cur, t, uncond_cf, x_key_mask), cfg, rescale_cfg)
                    return embeds

                seq = decode_tokens(B, seq_len, n_timesteps[layer], V, dev, build_input, forwards, self._logit_h[layer], self.to_logits[layer],
                                    temp, filter_thres, noise, record)
                cum = embed_sum_chain(seq[None], [self.token_emb[layer].weight], cum)
                xt[..., layer] = seq
            check_codes(dev)
        return xt
