"""The non-autoregressive Llama of Vevo's flow-matching transformer and MaskGCT's S2A (models/vc/flow_matching_transformer/llama_nar.py:
``DiffLlama``, ``LlamaAdaptiveRMSNorm``, ``SinusoidalPosEmb``), eval mode, on the gfx950 kernels.  Same class names, constructor arguments and
``state_dict`` keys; plain ``nn.Module``s hold the parameters (``transformers`` is not imported), and ``load_state_dict`` drops the
``*.rotary_emb.inv_freq`` buffers that checkpoints saved under older ``transformers`` carry.

The forward is composed channel-first ([B, C, T]) from launches:

    every nn.Linear                       ``amp_pw_forward``; q | k | v are ONE stacked handle and gate | up another, o_proj and down_proj (and
                                          mel_mlp's second Linear, which adds the condition) add the residual stream AFTER the accumulation
                                          through the ``res + gamma (.) (Wx + b)`` epilogue with gamma = 1, as FACodec's transformer does
    nn.SiLU, silu(gate) * up              ``amp_silu`` (in place), ``amp_swiglu`` on the stacked GEMM's output
    the 2L + 1 LlamaAdaptiveRMSNorm       their weights depend on the diffusion step alone: ONE stacked [(2L + 1) C, C] pointwise GEMM on the
                                          step embedding's [B, C, 1] column per forward, and one ``amp_rms_norm_c_adaptive`` launch per norm that
                                          reads its slice of that result through the batch stride
    LlamaAttention                        ``amp_rope_attention`` on the three row blocks of the stacked GEMM's output, read in place: HF's
                                          rotate-half RoPE, the key mask of ``_prepare_decoder_attention_mask`` (llama_nar.py:197-234: every
                                          query row is computed, padded keys contribute nothing), flash-style -- no [H, T, T] tensor

That is 11 + 8 L launches per forward with the condition's embedding given (L = layers: 8 per layer; 3 each for mel_mlp, diff_step_mlp and
mel_out_mlp, the stacked norm weights, the final norm), 3 more when ``cond_mlp`` runs inside.  Head dimension
64 only (Vevo and MaskGCT S2A: 1024 / 16).  Training, dropout, ``past_key_values``, ``output_attentions`` and friends are outside the HIP path."""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle, pw_forward
from amphion_amd.modules.hip_ops import rms_norm_c_adaptive, rope_attention, rope_tables, silu, swiglu

AMP_PW_BIAS, AMP_PW_SCALE_RES = 0, 2      # include/amphion_hip.h: amp_pw_epilogue


class _Stacked:
    """what ``pw_forward`` reads of an nn.Linear, for several Linears of one input stacked along the output axis (q | k | v, gate | up, the
    ``to_weight`` of every adaptive norm)"""

    def __init__(self, linears):
        self.linears = list(linears)
        self.in_features = self.linears[0].in_features
        self.out_features = sum(lin.out_features for lin in self.linears)


class _StackedPwHandle:
    """``_PwHandle`` for a ``_Stacked``: one packed device copy of all its weights, rebuilt when any parameter, the device or the precision
    changes"""

    def __init__(self):
        self._cache = HandleCache("amp_pw_destroy")

    def get(self, st, device):
        tensors = [lin.weight for lin in st.linears] + [lin.bias for lin in st.linears]
        return self._cache.get(param_sig(tensors, str(device), _lib.get_precision()), self._build, st, device)

    def _build(self, st, device):
        w = torch.cat([host_f32(lin.weight) for lin in st.linears], 0).contiguous()
        b = None
        if any(lin.bias is not None for lin in st.linears):
            b = torch.cat([host_f32(lin.bias) if lin.bias is not None else torch.zeros(lin.out_features) for lin in st.linears]).contiguous()
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_pw_create(st.in_features, st.out_features, _p(w), _p(b), ctypes.byref(h)))
        return h


_ones = {}     # (n, device) -> the gamma = 1 of the residual epilogue


def _gamma_one(n, device):
    t = _ones.get((n, device))
    if t is None:
        t = _ones[(n, device)] = torch.ones(n, dtype=torch.float32, device=device)
    return t


def _pw(handle, lin, x, res=None):
    """lin(x) along the channel axis of x [B, cin, T] (+ res, added after the accumulation) -> [B, cout, T]"""
    out = torch.empty((x.shape[0], lin.out_features, x.shape[2]), dtype=torch.float32, device=x.device)
    if res is None:
        return pw_forward(handle, lin, x, AMP_PW_BIAS, out)
    return pw_forward(handle, lin, x, AMP_PW_SCALE_RES, out, gamma=_gamma_one(lin.out_features, x.device), res=res)


def _drop_inv_freq(state_dict, prefix, *_):
    for k in [k for k in state_dict if k.startswith(prefix) and k.endswith("rotary_emb.inv_freq")]:
        del state_dict[k]


class SinusoidalPosEmb(nn.Module):
    """llama_nar.py:17-29: the diffusion step t [B] -> [B, dim], sines of t * f_i then cosines, f_i = 10000^(-i / (dim/2 - 1)); plain torch on
    the device (one row per item)"""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        half = self.dim // 2
        rate = math.log(10000) / (half - 1)
        freqs = torch.exp(torch.arange(half, device=x.device) * -rate)
        phase = x[:, None] * freqs[None, :] * 1.0
        return torch.cat((phase.sin(), phase.cos()), dim=-1)


class LlamaAdaptiveRMSNorm(nn.Module):
    """llama_nar.py:32-50: ``to_weight(cond) * x * rsqrt(mean(x^2) + eps)``, the weight one row per item"""

    def __init__(self, hidden_size=1024, eps=1e-6, dim_cond=1024):
        super().__init__()
        self.to_weight = nn.Linear(dim_cond, hidden_size)
        nn.init.zeros_(self.to_weight.weight)
        nn.init.ones_(self.to_weight.bias)
        self.variance_epsilon = eps
        self._h = _PwHandle()

    def forward_cf(self, x, weight):
        """x [B, C, T] channel-first; weight [B, C] (a slice of a wider tensor is read in place)"""
        return rms_norm_c_adaptive(x, weight, eps=self.variance_epsilon)

    def forward(self, hidden_states, cond_embedding):
        """hidden_states [B, T, C], cond_embedding [B, dim_cond], as the reference takes them"""
        x = _lib.require_device_tensor(hidden_states, "LlamaAdaptiveRMSNorm input")
        c = _lib.require_device_tensor(cond_embedding, "LlamaAdaptiveRMSNorm condition")
        if x.dim() != 3 or c.dim() != 2 or c.shape[0] != x.shape[0] or c.shape[1] != self.to_weight.in_features or x.shape[2] != self.to_weight.out_features:
            raise ValueError(f"LlamaAdaptiveRMSNorm: expected [B, T, {self.to_weight.out_features}] and a condition [B, {self.to_weight.in_features}], "
                             f"got {tuple(x.shape)} and {tuple(c.shape)}")
        with _lib.on_device(x.device):
            w = _pw(self._h, self.to_weight, c[:, :, None].contiguous())
            return self.forward_cf(x.transpose(1, 2).contiguous(), w).transpose(1, 2)


class LlamaAttention(nn.Module):
    """the parameter holder of HF's LlamaAttention without biases: ``{q,k,v,o}_proj.weight``"""

    def __init__(self, hidden_size, num_heads):
        super().__init__()
        self.hidden_size, self.num_heads, self.head_dim = hidden_size, num_heads, hidden_size // num_heads
        self.q_proj = nn.Linear(hidden_size, hidden_size, bias=False)
        self.k_proj = nn.Linear(hidden_size, hidden_size, bias=False)
        self.v_proj = nn.Linear(hidden_size, hidden_size, bias=False)
        self.o_proj = nn.Linear(hidden_size, hidden_size, bias=False)
        self._qkv, self._out = _StackedPwHandle(), _PwHandle()

    def forward_cf(self, x, res, cos, sin, key_mask):
        """res + o_proj(attention(x)), channel-first"""
        C = self.hidden_size
        qkv = _pw(self._qkv, _Stacked((self.q_proj, self.k_proj, self.v_proj)), x)
        att = rope_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], self.num_heads, cos, sin, key_mask)
        return _pw(self._out, self.o_proj, att, res=res)


class LlamaMLP(nn.Module):
    """HF's LlamaMLP without biases: ``down_proj(silu(gate_proj(x)) * up_proj(x))``"""

    def __init__(self, hidden_size, intermediate_size):
        super().__init__()
        self.gate_proj = nn.Linear(hidden_size, intermediate_size, bias=False)
        self.up_proj = nn.Linear(hidden_size, intermediate_size, bias=False)
        self.down_proj = nn.Linear(intermediate_size, hidden_size, bias=False)
        self._gu, self._down = _StackedPwHandle(), _PwHandle()

    def forward_cf(self, x, res):
        return _pw(self._down, self.down_proj, swiglu(_pw(self._gu, _Stacked((self.gate_proj, self.up_proj)), x)), res=res)


class LlamaNARDecoderLayer(nn.Module):
    """llama_nar.py:53-124: a Llama decoder layer whose two norms are adaptive"""

    def __init__(self, hidden_size, num_heads, layer_idx=0):
        super().__init__()
        self.hidden_size, self.layer_idx = hidden_size, layer_idx
        self.self_attn = LlamaAttention(hidden_size, num_heads)
        self.mlp = LlamaMLP(hidden_size, hidden_size * 4)
        self.input_layernorm = LlamaAdaptiveRMSNorm(hidden_size, dim_cond=hidden_size)
        self.post_attention_layernorm = LlamaAdaptiveRMSNorm(hidden_size, dim_cond=hidden_size)

    def forward_cf(self, x, w_in, w_post, cos, sin, key_mask):
        x = self.self_attn.forward_cf(self.input_layernorm.forward_cf(x, w_in), x, cos, sin, key_mask)
        return self.mlp.forward_cf(self.post_attention_layernorm.forward_cf(x, w_post), x)


class _Mlp2:
    """nn.Sequential(Linear, SiLU, Linear) on [B, C, T]: two pointwise GEMMs around an in-place ``amp_silu``"""

    def __init__(self):
        self._h0, self._h2 = _PwHandle(), _PwHandle()

    def __call__(self, seq, x, res=None):
        y = _pw(self._h0, seq[0], x)
        return _pw(self._h2, seq[2], silu(y, out=y), res=res)


class DiffLlama(nn.Module):
    def __init__(self, mel_dim=100, hidden_size=1024, num_heads=16, num_layers=16, dropout=0.1, ffn_dropout=0.1, attention_dropout=0.0,
                 config=None):
        super().__init__()
        if hidden_size % num_heads or hidden_size // num_heads != 64:
            raise NotImplementedError(f"DiffLlama: head dimension {hidden_size}/{num_heads} is not on the HIP path (64 only: Vevo and MaskGCT S2A)")
        self.mel_dim, self.hidden_size, self.num_heads, self.num_layers = mel_dim, hidden_size, num_heads, num_layers
        self.max_position_embeddings = 4096
        self.layers = nn.ModuleList([LlamaNARDecoderLayer(hidden_size, num_heads, layer_idx=i) for i in range(num_layers)])
        self.norm = LlamaAdaptiveRMSNorm(hidden_size, dim_cond=hidden_size)
        self.diff_step_embedding = SinusoidalPosEmb(hidden_size)
        self.diff_step_mlp = nn.Sequential(nn.Linear(hidden_size, hidden_size * 4), nn.SiLU(), nn.Linear(hidden_size * 4, hidden_size))
        self.cond_mlp = nn.Sequential(nn.Linear(hidden_size, hidden_size * 4), nn.SiLU(), nn.Linear(hidden_size * 4, hidden_size))
        self.mel_mlp = nn.Sequential(nn.Linear(mel_dim, hidden_size * 4), nn.SiLU(), nn.Linear(hidden_size * 4, hidden_size))
        self.mel_out_mlp = nn.Sequential(nn.Linear(hidden_size, hidden_size * 4), nn.SiLU(), nn.Linear(hidden_size * 4, mel_dim))
        self.embed_tokens = None
        keep = {id(n.to_weight) for n in self._norms()}
        for m in self.modules():                       # LlamaModel.post_init: normal(0, initializer_range = 0.02), zero biases; to_weight keeps its own
            if isinstance(m, nn.Linear) and id(m) not in keep:
                m.weight.data.normal_(mean=0.0, std=0.02)
                if m.bias is not None:
                    m.bias.data.zero_()
        self._register_load_state_dict_pre_hook(_drop_inv_freq)
        self._step, self._cond, self._mel, self._out = _Mlp2(), _Mlp2(), _Mlp2(), _Mlp2()
        self._norm_w = _StackedPwHandle()

    def _norms(self):
        return [n for layer in self.layers for n in (layer.input_layernorm, layer.post_attention_layernorm)] + [self.norm]

    def _check(self, t, shape, name):
        t = _lib.require_device_tensor(t, f"DiffLlama {name}")
        if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)) or t.numel() == 0:
            raise ValueError(f"DiffLlama: expected {name} of shape {list(shape)} (None = any), got {tuple(t.shape)}")
        w = self.norm.to_weight.weight
        if t.device != w.device:
            raise RuntimeError(f"DiffLlama: {name} is on {t.device} but the parameters are on {w.device}: move the module to the input's device")
        return t

    def cond_embedding_cf(self, cond):
        """``cond_mlp(cond)`` of cond [B, T, hidden], channel-first [B, hidden, T]: what ``forward`` takes as ``cond_embedding_cf`` so that a
        sampler computes it once per call instead of once per step (the same launches: the same bits)"""
        cond = self._check(cond, (None, None, self.hidden_size), "cond")
        with _lib.on_device(cond.device):
            return self._cond(self.cond_mlp, cond.transpose(1, 2).contiguous())

    def zero_cond_embedding_cf(self, B, T, device):
        """``cond_embedding_cf(zeros [B, T, hidden])`` from ONE column: every column of the pointwise GEMMs is computed alone, so the column
        of a zero condition is the same everywhere (the classifier-free branch of the sampler)"""
        with _lib.on_device(torch.device(device)):
            col = self._cond(self.cond_mlp, torch.zeros((1, self.hidden_size, 1), dtype=torch.float32, device=device))
            return col.expand(B, self.hidden_size, T).contiguous()

    def forward(self, x, diffusion_step, cond, x_mask, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=False, *,
                cond_embedding_cf=None):
        """x [B, T, mel], diffusion_step [B], cond [B, T, hidden], x_mask [B, T] (nonzero = valid; None = all valid) -> [B, T, mel];
        ``return_dict=True``: {"output", "hidden_states": every layer's output [B, T, hidden]}.  ``cond_embedding_cf`` (keyword-only) replaces
        ``cond`` by an already computed ``cond_embedding_cf(cond)``."""
        if self.training:
            raise NotImplementedError("DiffLlama: training mode is not on the HIP path (eval-only scope): call .eval()")
        if any(a is not None for a in (input_ids, attention_mask, position_ids, past_key_values, inputs_embeds)) or use_cache or output_attentions \
                or output_hidden_states:
            raise NotImplementedError("DiffLlama: input_ids / attention_mask / position_ids / past_key_values / inputs_embeds / use_cache / "
                                      "output_attentions / output_hidden_states are not on the HIP path (the reference's callers pass none)")
        x = self._check(x, (None, None, self.mel_dim), "x")
        B, T, _ = x.shape
        if T > self.max_position_embeddings:
            raise ValueError(f"DiffLlama: {T} frames exceed max_position_embeddings = {self.max_position_embeddings}")
        C, dev = self.hidden_size, x.device
        diffusion_step = self._check(diffusion_step, (B,), "diffusion_step")
        if cond_embedding_cf is None:
            cond_embedding_cf = self.cond_embedding_cf(self._check(cond, (B, T, C), "cond"))
        else:
            cond_embedding_cf = self._check(cond_embedding_cf, (B, C, T), "cond_embedding_cf")
        key_mask = None
        if x_mask is not None:
            if not isinstance(x_mask, torch.Tensor) or tuple(x_mask.shape) != (B, T) or x_mask.device != dev:
                raise ValueError(f"DiffLlama: x_mask must be a {(B, T)} tensor on {dev}")
            key_mask = (x_mask != 0).to(torch.uint8)
        with _lib.on_device(dev):
            h = self._mel(self.mel_mlp, x.transpose(1, 2).contiguous(), res=cond_embedding_cf)         # mel_mlp(x) + cond_mlp(cond)
            step = self._step(self.diff_step_mlp, self.diff_step_embedding(diffusion_step)[:, :, None].contiguous())   # [B, C, 1]
            norms = self._norms()
            w = _pw(self._norm_w, _Stacked([n.to_weight for n in norms]), step)[:, :, 0]                  # [B, (2L + 1) C]
            cos, sin = rope_tables(T, C // self.num_heads, dev)
            hidden = []
            for i, layer in enumerate(self.layers):
                h = layer.forward_cf(h, w[:, 2 * i * C:(2 * i + 1) * C], w[:, (2 * i + 1) * C:(2 * i + 2) * C], cos, sin, key_mask)
                if return_dict:
                    hidden.append(h.transpose(1, 2).clone())
            h = self.norm.forward_cf(h, w[:, 2 * len(self.layers) * C:])
            out = self._out(self.mel_out_mlp, h).transpose(1, 2).contiguous()
        if return_dict:
            return {"output": out, "hidden_states": hidden}
        return out
