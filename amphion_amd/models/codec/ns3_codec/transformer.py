"""The transformer encoder of FACodec (models/codec/ns3_codec/transformer.py:13-234): 4 pre-LN transformer layers (hidden 256, 4 heads, FFN
Conv1d(256, 1024, 5) -> ReLU -> Linear), eval mode, plain (``use_cln=False``: the timbre and mel-spectrogram encoders) or conditioned on a
speaker embedding (``use_cln=True``: the redecoder's prosody encoder).  Same class names, constructor arguments and ``state_dict`` keys
(``nn.LayerNorm`` / ``nn.MultiheadAttention`` / ``nn.Conv1d`` / ``nn.Linear`` hold the parameters; their forwards are not used).

It runs once per utterance at the frame rate and is composed channel-first ([B, 256, T]) from existing launches: the channel LayerNorm
(``amp_layer_norm_c``), the pointwise GEMM (``amp_pw_forward``) for the q | k | v projection, out_proj and ffn_2 -- the last two with its
``res + gamma (.) (Wx + b)`` epilogue and gamma = 1, which adds the residual stream AFTER the accumulation -- the conv kernel for the k = 5
conv with ReLU on store, and torch's scaled-dot-product attention on the device for the attention core.  (The conv kernels' own residual
argument starts the accumulator from bias + residual, so every product is rounded at the magnitude of the residual stream: measured 2.6 -
8.3e-6 per ffn_2 on a stream of magnitude 4 - 8, against 0.3 - 0.5e-6 for an fp32 GEMM that adds the stream last.  Fine for a waveform, not
for an embedding that is compared at 1e-6.)

The position-embedding quirk of the reference is kept: ``PositionalEncoding.forward`` adds ``pe[: x.size(0)]`` to a BATCH-FIRST tensor
(transformer.py:50, called with [B, T, d]), so row ``pe[b]`` is added to EVERY frame of item b -- the result depends on the item's index in the
batch, not on time.

``use_cln=True``: ``ln_1`` / ``ln_2`` / ``last_ln`` are ``StyleAdaptiveLayerNorm``.  The condition [B, T, d] is averaged over time once per
forward (every norm takes the same mean, transformer.py:25), each norm's ``style`` Linear runs on that [B, d, 1] column through the pointwise
GEMM, and its [B, 2 d] result is the per-item scale | shift of ONE ``amp_layer_norm_c_style`` launch: two launches per norm, nine norms per
forward.  A padding mask is refused in both forms."""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle, pw_forward
from amphion_amd.modules.hip_ops import add_channel_bias_, layer_norm_c, layer_norm_c_style

AMP_PW_BIAS, AMP_PW_SCALE_RES = 0, 2      # include/amphion_hip.h: amp_pw_epilogue


class _LinearView:
    """what ``_PwHandle`` reads of an nn.Linear, for a weight / bias pair held elsewhere (``MultiheadAttention.in_proj_*``)"""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias
        self.out_features, self.in_features = weight.shape


def pw(handle, lin, x, res=None):
    """lin(x) along the channel axis of x [B, cin, T] (+ res, added after the accumulation) -> [B, cout, T]"""
    out = torch.empty((x.shape[0], lin.out_features, x.shape[2]), dtype=torch.float32, device=x.device)
    if res is None:
        return pw_forward(handle, lin, x, AMP_PW_BIAS, out)
    return pw_forward(handle, lin, x, AMP_PW_SCALE_RES, out, gamma=torch.ones(lin.out_features, dtype=torch.float32, device=x.device), res=res)


class ConvCache:
    """An ``amp_conv`` handle for a Conv1d / Linear whose parameters live in a torch module: weight [cout, cin, k] or [cout, cin], rebuilt when
    a parameter, the device or the precision changes.  Owns no parameters."""

    def __init__(self, k=1, padding=0, tanh=False):
        self.k, self.padding, self.tanh = k, padding, tanh
        self._cache = HandleCache("amp_conv_destroy")

    def _ensure(self, weight, bias, device):
        return self._cache.get(param_sig((weight, bias), str(device), _lib.get_precision()), self._build, weight, bias, device)

    def _build(self, weight, bias, device):
        w, b = host_f32(weight), host_f32(bias)
        cout, cin = w.shape[0], w.shape[1]
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_conv_create(0, cin, cout, self.k, 1, 1, self.padding, _p(w), _p(b), ctypes.byref(h)))
            self._cache.adopt(h)
            if self.tanh:
                _lib.check(_lib.lib().amp_conv_set_option(h, _lib.AMP_CONV_OPT_TANH, 1))
        return h

    def __call__(self, weight, bias, x, slope_out=1.0):
        """x [B, cin, T] -> lrelu_out(conv(x) + bias) [B, cout, T] (slope_out = 0: ReLU)"""
        B, _, T = x.shape
        dev = x.device
        h = self._ensure(weight, bias, dev)
        out = torch.empty((B, weight.shape[0], T), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().amp_conv_forward(h, _p(x), B, T, 1.0, None, float(slope_out), _p(out), _lib.current_stream_ptr(dev)))
        return out


class StyleAdaptiveLayerNorm(nn.Module):
    """transformer.py:13-32: ``style`` is the only parameter holder (``norm`` has no affine)"""

    def __init__(self, normalized_shape, eps=1e-5):
        super().__init__()
        self.in_dim = normalized_shape
        self.norm = nn.LayerNorm(self.in_dim, eps=eps, elementwise_affine=False)
        self.style = nn.Linear(self.in_dim, self.in_dim * 2)
        self.style.bias.data[: self.in_dim] = 1
        self.style.bias.data[self.in_dim:] = 0
        self._h = _PwHandle()

    def forward_cf(self, x, cond_mean):
        """x [B, d, T] channel-first, cond_mean [B, d, 1] (the condition's mean over time) -> gamma * LN(x) + beta"""
        return layer_norm_c_style(x, pw(self._h, self.style, cond_mean), eps=self.norm.eps)

    def forward(self, x, condition):
        """x [B, T, d], condition [B, T, d], as the reference takes them"""
        x = _lib.require_device_tensor(x, "StyleAdaptiveLayerNorm input")
        condition = _lib.require_device_tensor(condition, "StyleAdaptiveLayerNorm condition")
        if x.dim() != 3 or x.shape[2] != self.in_dim or condition.dim() != 3 or condition.shape[2] != self.in_dim or condition.shape[0] != x.shape[0]:
            raise ValueError(f"StyleAdaptiveLayerNorm: expected x and condition [B, T, {self.in_dim}], got {tuple(x.shape)} and {tuple(condition.shape)}")
        with _lib.on_device(x.device):
            m = torch.mean(condition, dim=1, keepdim=True).transpose(1, 2).contiguous()
            return self.forward_cf(x.transpose(1, 2).contiguous(), m).transpose(1, 2)


def _norm(ln, x, cond_mean):
    if cond_mean is None:
        return layer_norm_c(x, ln.weight.detach(), ln.bias.detach(), eps=ln.eps)
    return ln.forward_cf(x, cond_mean)


class PositionalEncoding(nn.Module):
    def __init__(self, d_model, dropout, max_len=5000):
        super().__init__()
        self.dropout = dropout
        position = torch.arange(max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2) * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, 1, d_model)
        pe[:, 0, 0::2] = torch.sin(position * div_term)
        pe[:, 0, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe)

    def forward_cf(self, x):
        """x [B, d, T] channel-first -> a new tensor with pe[b] added to every frame of item b (the reference's quirk, see the module docstring)"""
        B = x.shape[0]
        if B > self.pe.shape[0]:
            raise ValueError(f"PositionalEncoding: batch {B} exceeds the table's {self.pe.shape[0]} rows (the reference indexes it with the batch size)")
        return add_channel_bias_(x.clone(), self.pe[:B, 0].contiguous())


class TransformerFFNLayer(nn.Module):
    def __init__(self, encoder_hidden, conv_filter_size, conv_kernel_size, encoder_dropout):
        super().__init__()
        self.encoder_hidden = encoder_hidden
        self.conv_filter_size = conv_filter_size
        self.conv_kernel_size = conv_kernel_size
        self.encoder_dropout = encoder_dropout
        if conv_kernel_size % 2 != 1:
            raise NotImplementedError("TransformerFFNLayer: an even conv_kernel_size changes the length; not on the HIP path")
        self.ffn_1 = nn.Conv1d(encoder_hidden, conv_filter_size, conv_kernel_size, padding=conv_kernel_size // 2)
        self.ffn_1.weight.data.normal_(0.0, 0.02)
        self.ffn_2 = nn.Linear(conv_filter_size, encoder_hidden)
        self.ffn_2.weight.data.normal_(0.0, 0.02)
        self._c1, self._c2 = ConvCache(conv_kernel_size, conv_kernel_size // 2), _PwHandle()

    def forward_cf(self, x, res):
        """res + ffn_2(relu(ffn_1(x))), channel-first"""
        h = self._c1(self.ffn_1.weight, self.ffn_1.bias, x, slope_out=0.0)
        return pw(self._c2, self.ffn_2, h, res=res)


class TransformerEncoderLayer(nn.Module):
    def __init__(self, encoder_hidden, encoder_head, conv_filter_size, conv_kernel_size, encoder_dropout, use_cln):
        super().__init__()
        self.encoder_hidden = encoder_hidden
        self.encoder_head = encoder_head
        self.conv_filter_size = conv_filter_size
        self.conv_kernel_size = conv_kernel_size
        self.encoder_dropout = encoder_dropout
        self.use_cln = use_cln
        norm = StyleAdaptiveLayerNorm if use_cln else nn.LayerNorm
        self.ln_1 = norm(encoder_hidden)
        self.ln_2 = norm(encoder_hidden)
        self.self_attn = nn.MultiheadAttention(encoder_hidden, encoder_head, batch_first=True)
        self.ffn = TransformerFFNLayer(encoder_hidden, conv_filter_size, conv_kernel_size, encoder_dropout)
        self._qkv, self._out = _PwHandle(), _PwHandle()

    def forward_cf(self, x, cond_mean=None):
        B, H, T = x.shape
        nh = self.encoder_head
        a = self.self_attn
        h = _norm(self.ln_1, x, cond_mean)
        qkv = pw(self._qkv, _LinearView(a.in_proj_weight, a.in_proj_bias), h)
        q, k, v = (t.reshape(B, nh, H // nh, T).transpose(2, 3) for t in qkv.chunk(3, 1))
        att = F.scaled_dot_product_attention(q, k, v).transpose(2, 3).reshape(B, H, T).contiguous()
        x = pw(self._out, a.out_proj, att, res=x)
        h = _norm(self.ln_2, x, cond_mean)
        return self.ffn.forward_cf(h, x)


class TransformerEncoder(nn.Module):
    def __init__(self, enc_emb_tokens=None, encoder_layer=4, encoder_hidden=256, encoder_head=4, conv_filter_size=1024, conv_kernel_size=5,
                 encoder_dropout=0.1, use_cln=False, cfg=None):
        super().__init__()
        self.encoder_layer = encoder_layer if encoder_layer is not None else cfg.encoder_layer
        self.encoder_hidden = encoder_hidden if encoder_hidden is not None else cfg.encoder_hidden
        self.encoder_head = encoder_head if encoder_head is not None else cfg.encoder_head
        self.conv_filter_size = conv_filter_size if conv_filter_size is not None else cfg.conv_filter_size
        self.conv_kernel_size = conv_kernel_size if conv_kernel_size is not None else cfg.conv_kernel_size
        self.encoder_dropout = encoder_dropout if encoder_dropout is not None else cfg.encoder_dropout
        self.use_cln = use_cln if use_cln is not None else cfg.use_cln
        if enc_emb_tokens is not None:
            raise NotImplementedError("TransformerEncoder: token embeddings are not on the HIP path (FACodec passes features)")
        self.use_enc_emb = False
        self.position_emb = PositionalEncoding(self.encoder_hidden, self.encoder_dropout)
        self.layers = nn.ModuleList([TransformerEncoderLayer(self.encoder_hidden, self.encoder_head, self.conv_filter_size, self.conv_kernel_size,
                                                             self.encoder_dropout, self.use_cln) for _ in range(self.encoder_layer)])
        self.last_ln = StyleAdaptiveLayerNorm(self.encoder_hidden) if self.use_cln else nn.LayerNorm(self.encoder_hidden)

    def forward_cf(self, x, cond_mean=None):
        """x [B, hidden, T] channel-first -> [B, hidden, T]; ``use_cln=True``: cond_mean [B, hidden] or [B, hidden, 1], the condition's mean
        over time"""
        if self.training:
            raise NotImplementedError("TransformerEncoder: training mode (dropout) is not on the HIP path: call .eval()")
        x = _lib.require_device_tensor(x, "TransformerEncoder input")
        if x.dim() != 3 or x.shape[1] != self.encoder_hidden or x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError(f"TransformerEncoder: expected a non-empty [B, {self.encoder_hidden}, T] input, got {tuple(x.shape)}")
        if self.use_cln:
            if cond_mean is None:
                raise ValueError("TransformerEncoder: use_cln=True needs a condition")
            cond_mean = _lib.require_device_tensor(cond_mean, "TransformerEncoder condition")
            if cond_mean.numel() != x.shape[0] * self.encoder_hidden or cond_mean.shape[0] != x.shape[0] or cond_mean.device != x.device:
                raise ValueError(f"TransformerEncoder: expected a condition mean {(x.shape[0], self.encoder_hidden)} on {x.device}, got "
                                 f"{tuple(cond_mean.shape)} on {cond_mean.device}")
            cond_mean = cond_mean.reshape(x.shape[0], self.encoder_hidden, 1)
        elif cond_mean is not None:
            raise ValueError("TransformerEncoder: a condition needs use_cln=True (the reference ignores it; passing one is a mistake)")
        with _lib.on_device(x.device):
            x = self.position_emb.forward_cf(x)
            for layer in self.layers:
                x = layer.forward_cf(x, cond_mean)
            return _norm(self.last_ln, x, cond_mean)

    def forward(self, x, key_padding_mask=None, condition=None):
        """x [B, T, hidden] batch-first, as the reference takes it -> [B, T, hidden]"""
        if key_padding_mask is not None:
            raise NotImplementedError("TransformerEncoder: a padding mask is not on the HIP path (FACodec passes None)")
        if not self.use_cln:
            if condition is not None:
                raise NotImplementedError("TransformerEncoder: a condition with use_cln=False is ignored by the reference; not on the HIP path")
            return self.forward_cf(x.transpose(1, 2).contiguous()).transpose(1, 2)
        if condition is None:
            raise ValueError("TransformerEncoder: use_cln=True needs a condition [B, T, hidden]")
        x = _lib.require_device_tensor(x, "TransformerEncoder input")
        condition = _lib.require_device_tensor(condition, "TransformerEncoder condition")
        if condition.dim() != 3 or x.dim() != 3 or condition.shape[0] != x.shape[0] or condition.shape[2] != self.encoder_hidden or condition.shape[1] < 1:
            raise ValueError(f"TransformerEncoder: expected a condition [B, T, {self.encoder_hidden}], got {tuple(condition.shape)}")
        if condition.device != x.device:
            raise RuntimeError(f"TransformerEncoder: the condition is on {condition.device}, the input on {x.device}")
        with _lib.on_device(x.device):
            m = torch.mean(condition, dim=1)                  # every norm takes this mean (transformer.py:25)
        return self.forward_cf(x.transpose(1, 2).contiguous(), m).transpose(1, 2)
