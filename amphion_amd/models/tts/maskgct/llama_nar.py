"""MaskGCT's two estimators (models/tts/maskgct/llama_nar.py: ``DiffLlama``, ``DiffLlamaPrefix``), eval mode, on the gfx950 kernels.  Same
class names, constructor arguments and ``state_dict`` keys; the forward is composed channel-first from the building blocks of Vevo's
flow-matching transformer (``models/vc/flow_matching_transformer/llama_nar.py``: the decoder layer, the adaptive norm, the stacked norm-weight
GEMM), which are imported, not copied.

    DiffLlama        x is already [B, T, hidden]: h = x + cond_mlp(cond); the output is the final adaptive norm's [B, T, hidden] (MaskGCT S2A)
    DiffLlamaPrefix  cond_mlp(phone_embedding) is prepended along time and phone_mask to the key mask; RoPE positions run over the whole
                     concatenation; the phone part of the output is dropped (MaskGCT T2S).  A phone embedding of zero frames, or None, is the
                     plain path and launches nothing for cond_mlp.

Head dimension 64 or 96 (``amp_rope_attention``).  ``load_state_dict`` drops the keys that carry nothing of the computation:
``*.rotary_emb.inv_freq`` and the zero-row ``embed_tokens.weight`` that ``LlamaModel.__init__`` leaves in DiffLlama.  ``forward_cf`` is the
channel-first form the samplers call: no transposes between the estimator, the logits GEMM and the sampler kernel."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.vc.flow_matching_transformer.llama_nar import (LlamaAdaptiveRMSNorm, LlamaNARDecoderLayer, SinusoidalPosEmb, _drop_inv_freq,
                                                                        _Mlp2, _pw, _Stacked, _StackedPwHandle)
from amphion_amd.modules.hip_ops import rope_tables


def _drop_unused(state_dict, prefix, *_):
    _drop_inv_freq(state_dict, prefix)
    state_dict.pop(prefix + "embed_tokens.weight", None)


def _mlp(hidden_size):
    return nn.Sequential(nn.Linear(hidden_size, hidden_size * 4), nn.SiLU(), nn.Linear(hidden_size * 4, hidden_size))


class _NarEstimator(nn.Module):
    """what the two estimators share: the layers, the final norm, the step embedding and its MLP, and the walk through them"""

    def __init__(self, hidden_size, num_heads, num_layers):
        super().__init__()
        name = type(self).__name__
        if hidden_size % num_heads or hidden_size // num_heads not in (64, 96):
            raise NotImplementedError(f"{name}: head dimension {hidden_size}/{num_heads} is not on the HIP path (64 or 96)")
        self.hidden_size, self.num_heads, self.num_layers = hidden_size, num_heads, num_layers
        self.max_position_embeddings = 4096
        self.layers = nn.ModuleList([LlamaNARDecoderLayer(hidden_size, num_heads, layer_idx=i) for i in range(num_layers)])
        self.norm = LlamaAdaptiveRMSNorm(hidden_size, dim_cond=hidden_size)
        self.diff_step_embedding = SinusoidalPosEmb(hidden_size)
        self.diff_step_mlp = _mlp(hidden_size)
        self.embed_tokens = None
        self._register_load_state_dict_pre_hook(_drop_unused)
        self._step, self._cond = _Mlp2(), _Mlp2()
        self._norm_w = _StackedPwHandle()

    def _post_init(self):
        keep = {id(n.to_weight) for n in self._norms()}
        for m in self.modules():                       # LlamaModel.post_init: normal(0, 0.02), zero biases; to_weight keeps its own
            if isinstance(m, nn.Linear) and id(m) not in keep:
                m.weight.data.normal_(mean=0.0, std=0.02)
                if m.bias is not None:
                    m.bias.data.zero_()

    def _norms(self):
        return [n for layer in self.layers for n in (layer.input_layernorm, layer.post_attention_layernorm)] + [self.norm]

    def _check(self, t, shape, name):
        t = _lib.require_device_tensor(t, f"{type(self).__name__} {name}")
        if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)) or t.numel() == 0:
            raise ValueError(f"{type(self).__name__}: expected {name} of shape {list(shape)} (None = any), got {tuple(t.shape)}")
        w = self.norm.to_weight.weight
        if t.device != w.device:
            raise RuntimeError(f"{type(self).__name__}: {name} is on {t.device} but the parameters are on {w.device}: move the module to the input's device")
        return t

    def _refuse(self, extra):
        if self.training:
            raise NotImplementedError(f"{type(self).__name__}: training mode is not on the HIP path (eval-only scope): call .eval()")
        if any(v is not None and v is not False for v in extra.values()):
            raise NotImplementedError(f"{type(self).__name__}: {' / '.join(extra)} are not on the HIP path (the reference's callers pass none)")

    @staticmethod
    def _key_mask(masks, lengths, B, dev):
        """the key mask of a concatenation along time; None when no part has one"""
        if all(m is None for m in masks):
            return None
        parts = []
        for m, n in zip(masks, lengths):
            if m is None:
                parts.append(torch.ones((B, n), dtype=torch.uint8, device=dev))
                continue
            if not isinstance(m, torch.Tensor) or tuple(m.shape) != (B, n) or m.device != dev:
                raise ValueError(f"the mask of a [{B}, {n}] part must be a {(B, n)} tensor on {dev}")
            parts.append((m != 0).to(torch.uint8))
        return torch.cat(parts, dim=1)

    def cond_embedding_cf(self, cond):
        """``cond_mlp(cond)`` of cond [B, T, hidden], channel-first [B, hidden, T]: a sampler computes it once per call, not once per step
        (the same launches: the same bits)"""
        cond = self._check(cond, (None, None, self.hidden_size), "cond")
        with _lib.on_device(cond.device):
            return self._cond(self.cond_mlp, cond.transpose(1, 2).contiguous())

    def _run(self, h, diffusion_step, key_mask):
        """h [B, C, T] -> the final adaptive norm's output [B, C, T]"""
        B, C, T = h.shape
        if T > self.max_position_embeddings:
            raise ValueError(f"{type(self).__name__}: {T} frames exceed max_position_embeddings = {self.max_position_embeddings}")
        diffusion_step = self._check(diffusion_step, (B,), "diffusion_step")
        step = self._step(self.diff_step_mlp, self.diff_step_embedding(diffusion_step)[:, :, None].contiguous())   # [B, C, 1]
        w = _pw(self._norm_w, _Stacked([n.to_weight for n in self._norms()]), step)[:, :, 0]                         # [B, (2L + 1) C]
        cos, sin = rope_tables(T, C // self.num_heads, h.device)
        for i, layer in enumerate(self.layers):
            h = layer.forward_cf(h, w[:, 2 * i * C:(2 * i + 1) * C], w[:, (2 * i + 1) * C:(2 * i + 2) * C], cos, sin, key_mask)
        return self.norm.forward_cf(h, w[:, 2 * len(self.layers) * C:])


class DiffLlama(_NarEstimator):
    def __init__(self, hidden_size=1024, num_heads=16, num_layers=16, config=None):
        super().__init__(hidden_size, num_heads, num_layers)
        self.cond_mlp = _mlp(hidden_size)
        self._post_init()

    def forward_cf(self, x_cf, diffusion_step, cond_embedding_cf, key_mask=None):
        """x_cf, cond_embedding_cf [B, hidden, T]; key_mask [B, T] uint8 or None -> [B, hidden, T]"""
        x_cf = self._check(x_cf, (None, self.hidden_size, None), "x")
        cond_embedding_cf = self._check(cond_embedding_cf, tuple(x_cf.shape), "cond_embedding_cf")
        with _lib.on_device(x_cf.device):
            return self._run(x_cf + cond_embedding_cf, diffusion_step, key_mask)

    def forward(self, x, diffusion_step, cond, x_mask, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None, *,
                cond_embedding_cf=None):
        """x [B, T, hidden], diffusion_step [B], cond [B, T, hidden], x_mask [B, T] (nonzero = valid; None = all valid) -> [B, T, hidden].
        ``cond_embedding_cf`` (keyword-only) replaces ``cond`` by an already computed ``cond_embedding_cf(cond)``."""
        self._refuse(dict(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, past_key_values=past_key_values,
                          inputs_embeds=inputs_embeds, use_cache=use_cache, output_attentions=output_attentions,
                          output_hidden_states=output_hidden_states))
        x = self._check(x, (None, None, self.hidden_size), "x")
        B, T, _ = x.shape
        if cond_embedding_cf is None:
            cond_embedding_cf = self.cond_embedding_cf(self._check(cond, (B, T, self.hidden_size), "cond"))
        key_mask = self._key_mask([x_mask], [T], B, x.device)
        return self.forward_cf(x.transpose(1, 2).contiguous(), diffusion_step, cond_embedding_cf, key_mask).transpose(1, 2)


class DiffLlamaPrefix(_NarEstimator):
    def __init__(self, hidden_size=1024, num_heads=16, num_layers=16, use_phone_cond=True, config=None):
        super().__init__(hidden_size, num_heads, num_layers)
        self.use_phone_cond = use_phone_cond
        if use_phone_cond:
            self.cond_mlp = _mlp(hidden_size)
        self._post_init()

    def forward_cf(self, x_cf, diffusion_step, key_mask=None, phone_embedding_cf=None):
        """x_cf [B, hidden, T]; phone_embedding_cf [B, hidden, P] = ``cond_embedding_cf(phone_embedding)`` or None; key_mask [B, P + T] uint8
        over the concatenation or None -> [B, hidden, T], the phone part dropped"""
        x_cf = self._check(x_cf, (None, self.hidden_size, None), "x")
        P = 0
        with _lib.on_device(x_cf.device):
            if phone_embedding_cf is not None:
                phone_embedding_cf = self._check(phone_embedding_cf, (x_cf.shape[0], self.hidden_size, None), "phone_embedding_cf")
                P = phone_embedding_cf.shape[2]
                x_cf = torch.cat([phone_embedding_cf, x_cf], dim=2)
            if key_mask is not None and tuple(key_mask.shape) != (x_cf.shape[0], x_cf.shape[2]):
                raise ValueError(f"DiffLlamaPrefix: the key mask must cover the {x_cf.shape[2]} frames of phones + x, got {tuple(key_mask.shape)}")
            out = self._run(x_cf, diffusion_step, key_mask)
            return out[:, :, P:] if P else out

    def forward(self, x, diffusion_step, x_mask, phone_embedding=None, phone_mask=None, input_ids=None, attention_mask=None, position_ids=None,
                past_key_values=None, inputs_embeds=None, use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None):
        """x [B, T, hidden], diffusion_step [B], x_mask [B, T], phone_embedding [B, P, hidden] or None, phone_mask [B, P] -> [B, T, hidden]"""
        self._refuse(dict(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, past_key_values=past_key_values,
                          inputs_embeds=inputs_embeds, use_cache=use_cache, output_attentions=output_attentions,
                          output_hidden_states=output_hidden_states))
        x = self._check(x, (None, None, self.hidden_size), "x")
        B, T, _ = x.shape
        phone_cf, P = None, 0
        if self.use_phone_cond and phone_embedding is not None and phone_embedding.shape[1] > 0:
            phone_cf = self.cond_embedding_cf(self._check(phone_embedding, (B, None, self.hidden_size), "phone_embedding"))
            P = phone_cf.shape[2]
        if P:
            key_mask = self._key_mask([phone_mask, x_mask], [P, T], B, x.device)
        else:
            if self.use_phone_cond and phone_embedding is not None and phone_mask is not None and phone_mask.shape[1] != 0:
                raise ValueError(f"DiffLlamaPrefix: a phone mask of {phone_mask.shape[1]} frames beside a phone embedding of none (the reference "
                                 "fails with a shape error here)")
            key_mask = self._key_mask([x_mask], [T], B, x.device)
        return self.forward_cf(x.transpose(1, 2).contiguous(), diffusion_step, key_mask, phone_cf).transpose(1, 2)
