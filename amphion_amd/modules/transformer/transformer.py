"""modules/transformer/transformer.py: the pre-norm ``TransformerEncoderLayer`` / ``TransformerEncoder`` of VALL-E under the reference's parameter
names (``self_attn.in_proj_weight`` / ``in_proj_bias`` / ``out_proj.*``, ``linear1``, ``linear2``, ``norm1``, ``norm2``, ``norm``), eval mode, on
the gfx950 kernels, channel-first [B, C, T]:

    whole sequence (``forward_cf``)   ``amp_layer_norm_c`` -> the stacked q | k | v GEMM -> ``amp_prefix_attention`` (``prefix`` given: text sees
                                      text, audio sees text and the audio up to itself) or ``amp_cross_attention`` as full self-attention ->
                                      ``out_proj`` with the residual in the GEMM's epilogue -> ``amp_layer_norm_c`` -> ``linear1`` as a one-tap
                                      conv with ReLU on store -> ``linear2`` with the residual.  With ``caches`` every column's k and v go to
                                      the layer's KV cache (``amp_kv_append`` under identity rotation tables)
    one column (``step_cf``)          ``amp_pw_forward_vec_ln`` (LN -> q | k | v) -> ``amp_kv_append`` -> ``amp_attention_decode`` ->
                                      ``amp_pw_forward_vec`` (out_proj + residual) -> ``amp_pw_forward_vec_ln`` (LN -> linear1 -> ReLU) ->
                                      ``amp_pw_forward_vec`` (linear2 + residual)

An ``AdaptiveLayerNorm`` runs as ``amp_layer_norm_c`` with its host-folded gamma | beta (modules/norms/norm.py).  Not on the HIP path
(``NotImplementedError``): post-norm layers, activations other than ReLU, head dimensions other than 64.  The modules hold the parameters and the
channel-first methods VALL-E calls; the reference's [B, T, C] ``forward`` with arbitrary masks is not provided."""
from __future__ import annotations

import copy
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle
from amphion_amd.models.vc.flow_matching_transformer.llama_nar import _gamma_one, _pw
from amphion_amd.modules.hip_ops import (attention_decode, cross_attention, kv_append, layer_norm_c, prefix_attention, pw_forward_vec,
                                         pw_forward_vec_ln)
from amphion_amd.modules.norms import AdaptiveLayerNorm, LayerNorm


class _Lin:
    """what ``pw_forward`` reads of an nn.Linear, for a weight | bias pair that is not one (``in_proj_weight`` / ``in_proj_bias``)"""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias
        self.out_features, self.in_features = weight.shape


class _ReluLinear:
    """relu(lin(x)) along the channel axis of [B, cin, T] in one launch: the Linear as a one-tap conv whose epilogue is ``leaky_relu`` at slope
    0.  The packed device copy is rebuilt when the parameters, the device or the precision change."""

    def __init__(self):
        self._cache = HandleCache("amp_conv_destroy")

    def _build(self, lin, device):
        w, b = host_f32(lin.weight), host_f32(lin.bias)
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_conv_create(0, lin.in_features, lin.out_features, 1, 1, 1, 0, _p(w), _p(b), ctypes.byref(h)))
        return h

    def __call__(self, lin, x):
        dev = x.device
        h = self._cache.get(param_sig((lin.weight, lin.bias), str(dev), _lib.get_precision()), self._build, lin, dev)
        B, _, T = x.shape
        out = torch.empty((B, lin.out_features, T), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().amp_conv_forward(h, _p(x), B, T, 1.0, None, 0.0, _p(out), _lib.current_stream_ptr(dev)))
        return out


class MultiheadAttention(nn.Module):
    """the parameters of the reference's ``MultiheadAttention`` with nn.Linear projections: ``in_proj_weight`` [3 d, d], ``in_proj_bias``,
    ``out_proj``"""

    def __init__(self, embed_dim, num_heads, dropout=0.0, batch_first=False):
        super().__init__()
        if embed_dim % num_heads or embed_dim // num_heads != 64:
            raise NotImplementedError(f"MultiheadAttention: head dimension {embed_dim}/{num_heads} is not on the HIP path (64)")
        self.embed_dim, self.num_heads, self.head_dim, self.batch_first = embed_dim, num_heads, embed_dim // num_heads, batch_first
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)
        self._qkv, self._out = _PwHandle(), _PwHandle()

    def in_proj(self):
        return _Lin(self.in_proj_weight, self.in_proj_bias)


class TransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation=F.relu, batch_first=False, norm_first=False,
                 layer_norm_cls=LayerNorm, layer_norm_eps=1e-5, adaptive_layer_norm=False):
        super().__init__()
        if not norm_first:
            raise NotImplementedError("TransformerEncoderLayer: norm_first=False (post-norm) is not on the HIP path")
        if activation not in (F.relu, "relu"):
            raise NotImplementedError("TransformerEncoderLayer: the HIP path covers the ReLU feed-forward")
        self.self_attn = MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=batch_first)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm_first = norm_first
        self.dropout1, self.dropout2 = nn.Dropout(dropout), nn.Dropout(dropout)
        self.activation = F.relu
        norm1, norm2 = layer_norm_cls(d_model, eps=layer_norm_eps), layer_norm_cls(d_model, eps=layer_norm_eps)
        if adaptive_layer_norm:
            norm1, norm2 = AdaptiveLayerNorm(d_model, norm1), AdaptiveLayerNorm(d_model, norm2)
        self.norm1, self.norm2 = norm1, norm2
        self._l1, self._l2, self._relu1 = _PwHandle(), _PwHandle(), _ReluLinear()

    def forward_cf(self, x, stage_embedding=None, prefix=None, cache=None, ident=None):
        """x [B, C, T] -> the layer's output.  ``prefix``: the prefix-LM rule with that many leading columns (None: full self-attention).
        ``cache`` (kcache, vcache) with ``ident`` (the identity rotation tables): filled with the T columns at positions 0 .. T - 1"""
        a = self.self_attn
        C, H = a.embed_dim, a.num_heads
        g1, b1 = self.norm1.affine(stage_embedding)
        qkv = _pw(a._qkv, a.in_proj(), layer_norm_c(x, g1, b1, eps=self.norm1.eps))
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        if cache is not None:
            kv_append(k, v, H, ident[0], ident[1], 0, cache[0], cache[1])
        att = cross_attention(q, k, v, H) if prefix is None else prefix_attention(q, k, v, H, prefix)
        x = _pw(a._out, a.out_proj, att, res=x)
        g2, b2 = self.norm2.affine(stage_embedding)
        return _pw(self._l2, self.linear2, self._relu1(self.linear1, layer_norm_c(x, g2, b2, eps=self.norm2.eps)), res=x)

    def step_cf(self, x, L, cache, ident, fused=True):
        """x [B, C, 1], the column at position L - 1 -> the layer's output; the column's k / v are appended to the cache first.
        ``fused=False``: the same step from the launches that existed before ``amp_pw_forward_vec_ln`` (the norm at T = 1, the plain
        matrix-vector product, a separate ReLU) -- the comparison route of tools/valle_bench.py."""
        a = self.self_attn
        C, H, dev = a.embed_dim, a.num_heads, x.device
        g1, b1 = self.norm1.affine()
        g2, b2 = self.norm2.affine()
        hq, h1 = a._qkv.get(a.in_proj(), dev), self._l1.get(self.linear1, dev)
        F_ = self.linear1.out_features
        if fused:
            qkv = pw_forward_vec_ln(hq, 3 * C, x, g1, b1, self.norm1.eps)
        else:
            qkv = pw_forward_vec(hq, 3 * C, layer_norm_c(x, g1, b1, eps=self.norm1.eps))
        kv_append(qkv[:, C:2 * C], qkv[:, 2 * C:], H, ident[0], ident[1], L - 1, cache[0], cache[1])
        att = attention_decode(qkv[:, :C], H, ident[0], ident[1], L, cache[0], cache[1])
        x = pw_forward_vec(a._out.get(a.out_proj, dev), C, att, gamma=_gamma_one(C, dev), res=x)
        if fused:
            f = pw_forward_vec_ln(h1, F_, x, g2, b2, self.norm2.eps, relu=True)
        else:
            f = pw_forward_vec(h1, F_, layer_norm_c(x, g2, b2, eps=self.norm2.eps)).relu_()
        return pw_forward_vec(self._l2.get(self.linear2, dev), C, f, gamma=_gamma_one(C, dev), res=x)


class TransformerEncoder(nn.Module):
    def __init__(self, encoder_layer, num_layers, norm=None):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(encoder_layer) for _ in range(num_layers)])
        self.num_layers = num_layers
        self.norm = norm

    def forward_cf(self, x, stage_embedding=None, prefix=None, caches=None, ident=None, final_norm=True):
        for i, layer in enumerate(self.layers):
            x = layer.forward_cf(x, stage_embedding, prefix, None if caches is None else caches[i], ident)
        if final_norm and self.norm is not None:
            x = self.norm.forward_cf(x, stage_embedding)
        return x

    def step_cf(self, x, L, caches, ident, fused=True):
        """one column through every layer, WITHOUT the final norm (the caller folds it into the head's matrix-vector product)"""
        for layer, cache in zip(self.layers, caches):
            x = layer.step_cf(x, L, cache, ident, fused)
        return x
