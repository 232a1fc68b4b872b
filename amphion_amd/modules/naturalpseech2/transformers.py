"""modules/naturalpseech2/transformers.py on the HIP kernels, eval mode: the encoders and predictors of NaturalSpeech2.

    TransformerEncoderLayer   LayerNorm (``amp_layer_norm_c``) or StyleAdaptiveLayerNorm (``amp_layer_norm_c_style``) -> the stacked q | k | v
                              GEMM -> ``amp_cross_attention`` as self-attention on its three row blocks -> ``out_proj`` with the residual in
                              the GEMM's epilogue -> norm -> ``ffn_1`` (k = 9, ReLU on store) -> ``ffn_2`` with the residual        7 launches
    DurationPredictor /       the k | v of ALL cross-attention layers from ONE stacked GEMM on the prompt (``in_proj_weight`` re-stacked when
    PitchPredictor            the handle is built); per attention layer LayerNorm, the q GEMM, ``amp_cross_attention``, ``out_proj`` with the
                              residual, one scale; per conv layer the conv with ReLU on store and ``amp_layer_norm_c`` with ``post = res``;
                              the head reads LN(h) + res, not LN(h), so ``amp_layer_norm_c_head`` does not fit: it is the pointwise GEMM
    LengthRegulator           ``amp_expand_path`` along the running sum of the durations

Parameters, constructor arguments and ``state_dict`` keys are the reference's.  ``forward`` takes the reference's batch-first tensors;
``forward_cf`` is the channel-first [B, C, T] path the models use.  Masks are the reference's (1 = valid); the predictors run WITHOUT a
frame mask, as ``NaturalSpeech2.inference`` calls them.

Two properties of the reference that its results depend on are kept: ``PositionalEncoding`` adds row b of its table to EVERY frame of item
b (``pe[:x.size(0)]`` on a batch-first tensor: a per-item channel bias), and ``StyleAdaptiveLayerNorm`` takes the mean of its condition over
the whole padded length."""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle
from amphion_amd.models.vc.flow_matching_transformer.llama_nar import _pw
from amphion_amd.modules.hip_ops import HipConv1d, add_channel_bias_, cross_attention, expand_path, layer_norm_c, layer_norm_c_style


def _eval_only(module, who):
    if module.training:
        raise NotImplementedError(f"{who}: training mode (dropout) is not on the HIP path: call .eval()")


class _Rows:
    """what ``_pw`` reads of an nn.Linear, for a block of rows of a wider weight (the q rows of ``in_proj_weight``) or several blocks
    stacked (the k | v rows of every cross-attention layer of a predictor); ``tensors`` are the parameters the block is cut from"""

    def __init__(self, weight, bias, tensors):
        self.weight, self.bias, self.tensors = weight, bias, tensors
        self.out_features, self.in_features = weight.shape


class _RowsHandle:
    """``_PwHandle`` for a ``_Rows``: the packed device copy is keyed on the parameters the rows are cut from"""

    def __init__(self):
        self._cache = HandleCache("amp_pw_destroy")

    def get(self, rows, device):
        return self._cache.get(param_sig(rows.tensors, str(device), _lib.get_precision(), tuple(rows.weight.shape)), self._build, rows, device)

    def _build(self, rows, device):
        w, b = host_f32(rows.weight), host_f32(rows.bias)
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_pw_create(rows.in_features, rows.out_features, _p(w), _p(b), ctypes.byref(h)))
        return h


def mha_rows(attn, lo, hi):
    """rows [lo C, hi C) of an nn.MultiheadAttention's stacked in-projection"""
    C = attn.embed_dim
    return _Rows(attn.in_proj_weight.detach()[lo * C:hi * C], attn.in_proj_bias.detach()[lo * C:hi * C], (attn.in_proj_weight, attn.in_proj_bias))


def stacked_kv_rows(attns):
    """k | v rows of several nn.MultiheadAttention modules, one after the other: [n * 2C, C]"""
    C = attns[0].embed_dim
    w = torch.cat([a.in_proj_weight.detach()[C:] for a in attns], 0)
    b = torch.cat([a.in_proj_bias.detach()[C:] for a in attns], 0)
    return _Rows(w, b, tuple(t for a in attns for t in (a.in_proj_weight, a.in_proj_bias)))


def _check_mha(attn, who):
    if not attn._qkv_same_embed_dim or attn.in_proj_bias is None or attn.bias_k is not None or attn.add_zero_attn or not attn.batch_first:
        raise NotImplementedError(f"{who}: only nn.MultiheadAttention(batch_first=True) with kdim = vdim = embed_dim and biases is on the HIP path")
    if attn.embed_dim // attn.num_heads != 64:
        raise NotImplementedError(f"{who}: head dimension {attn.embed_dim // attn.num_heads} is not on the HIP path (amp_cross_attention: 64)")


class StyleAdaptiveLayerNorm(nn.Module):
    def __init__(self, normalized_shape, eps=1e-5):
        super().__init__()
        self.in_dim = normalized_shape
        self.norm = nn.LayerNorm(self.in_dim, eps=eps, elementwise_affine=False)
        self.style = nn.Linear(self.in_dim, self.in_dim * 2)
        self.style.bias.data[: self.in_dim] = 1
        self.style.bias.data[self.in_dim:] = 0
        self._h = _PwHandle()

    def style_of(self, cond_mean):
        """cond_mean [B, C, 1]: the mean of the condition over its (padded) length -> the gamma | beta rows [B, 2C, 1]"""
        return _pw(self._h, self.style, cond_mean)

    def forward_cf(self, x, cond_mean):
        return layer_norm_c_style(x, self.style_of(cond_mean), eps=self.norm.eps)

    def forward(self, x, condition):
        """x [B, T, d], condition [B, T', d] as the reference takes them"""
        x = _lib.require_device_tensor(x, "StyleAdaptiveLayerNorm input").transpose(1, 2).contiguous()
        mean = torch.mean(condition, dim=1, keepdim=True).transpose(1, 2).contiguous()
        with _lib.on_device(x.device):
            return self.forward_cf(x, mean).transpose(1, 2)


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
        """x [B, C, T], updated in place: item b takes row b of the table at every frame, as the reference's ``pe[:x.size(0)]`` does"""
        B = x.shape[0]
        if B > self.pe.shape[0]:
            raise ValueError(f"PositionalEncoding: a batch of {B} is beyond the table of {self.pe.shape[0]} rows")
        return add_channel_bias_(x, self.pe[:B, 0])

    def forward(self, x):
        _eval_only(self, "PositionalEncoding")
        return x + self.pe[: x.size(0)]


class TransformerFFNLayer(nn.Module):
    def __init__(self, encoder_hidden, conv_filter_size, conv_kernel_size, encoder_dropout):
        super().__init__()
        self.encoder_hidden, self.conv_filter_size = encoder_hidden, conv_filter_size
        self.conv_kernel_size, self.encoder_dropout = conv_kernel_size, encoder_dropout
        self.ffn_1 = HipConv1d(encoder_hidden, conv_filter_size, conv_kernel_size, padding=conv_kernel_size // 2, weight_norm=False)
        self.ffn_2 = nn.Linear(conv_filter_size, encoder_hidden)
        self._h = _PwHandle()

    def forward_cf(self, x, res):
        return _pw(self._h, self.ffn_2, self.ffn_1(x, slope_out=0.0), res=res)

    def forward(self, x):
        _eval_only(self, "TransformerFFNLayer")
        x = _lib.require_device_tensor(x, "TransformerFFNLayer input").transpose(1, 2).contiguous()
        with _lib.on_device(x.device):
            return _pw(self._h, self.ffn_2, self.ffn_1(x, slope_out=0.0)).transpose(1, 2)


class TransformerEncoderLayer(nn.Module):
    def __init__(self, encoder_hidden, encoder_head, conv_filter_size, conv_kernel_size, encoder_dropout, use_cln):
        super().__init__()
        self.encoder_hidden, self.encoder_head, self.use_cln = encoder_hidden, encoder_head, use_cln
        self.encoder_dropout = encoder_dropout
        norm = StyleAdaptiveLayerNorm if use_cln else nn.LayerNorm
        self.ln_1, self.ln_2 = norm(encoder_hidden), norm(encoder_hidden)
        self.self_attn = nn.MultiheadAttention(encoder_hidden, encoder_head, batch_first=True)
        self.ffn = TransformerFFNLayer(encoder_hidden, conv_filter_size, conv_kernel_size, encoder_dropout)
        self._qkv, self._out = _RowsHandle(), _PwHandle()

    def _norm(self, ln, x, cond_mean):
        if self.use_cln:
            return ln.forward_cf(x, cond_mean)
        return layer_norm_c(x, ln.weight.detach(), ln.bias.detach(), eps=ln.eps)

    def forward_cf(self, x, key_mask, cond_mean):
        """x [B, C, T]; key_mask [B, T] uint8 1 = valid or None; cond_mean [B, C, 1] (style-adaptive norms) or None"""
        C = self.encoder_hidden
        _check_mha(self.self_attn, "TransformerEncoderLayer")
        qkv = _pw(self._qkv, mha_rows(self.self_attn, 0, 3), self._norm(self.ln_1, x, cond_mean))
        att = cross_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], self.encoder_head, key_mask)
        x = _pw(self._out, self.self_attn.out_proj, att, res=x)
        return self.ffn.forward_cf(self._norm(self.ln_2, x, cond_mean), x)

    def forward(self, x, key_padding_mask, conditon=None):
        """x [B, T, d]; key_padding_mask [B, T], 0 = padded, or None; conditon [B, T', d] (spelled as the reference spells it)"""
        _eval_only(self, "TransformerEncoderLayer")
        x = _lib.require_device_tensor(x, "TransformerEncoderLayer input").transpose(1, 2).contiguous()
        with _lib.on_device(x.device):
            return self.forward_cf(x, _key_mask(key_padding_mask), _cond_mean(conditon) if self.use_cln else None).transpose(1, 2)


def _key_mask(mask):
    return None if mask is None else (mask != 0).to(torch.uint8).contiguous()


def _cond_mean(condition):
    """[B, T', d] -> the mean over the WHOLE padded length as [B, d, 1]"""
    return torch.mean(condition, dim=1, keepdim=True).transpose(1, 2).contiguous()


class TransformerEncoder(nn.Module):
    def __init__(self, enc_emb_tokens=None, encoder_layer=None, encoder_hidden=None, encoder_head=None, conv_filter_size=None,
                 conv_kernel_size=None, encoder_dropout=None, use_cln=None, cfg=None):
        super().__init__()
        pick = lambda v, name: v if v is not None else getattr(cfg, name)
        self.encoder_layer = pick(encoder_layer, "encoder_layer")
        self.encoder_hidden = pick(encoder_hidden, "encoder_hidden")
        self.encoder_head = pick(encoder_head, "encoder_head")
        self.conv_filter_size = pick(conv_filter_size, "conv_filter_size")
        self.conv_kernel_size = pick(conv_kernel_size, "conv_kernel_size")
        self.encoder_dropout = pick(encoder_dropout, "encoder_dropout")
        self.use_cln = pick(use_cln, "use_cln")
        if enc_emb_tokens is not None:
            self.use_enc_emb = True
            self.enc_emb_tokens = enc_emb_tokens
        else:
            self.use_enc_emb = False
        self.position_emb = PositionalEncoding(self.encoder_hidden, self.encoder_dropout)
        self.layers = nn.ModuleList([TransformerEncoderLayer(self.encoder_hidden, self.encoder_head, self.conv_filter_size, self.conv_kernel_size,
                                                             self.encoder_dropout, self.use_cln) for _ in range(self.encoder_layer)])
        self.last_ln = StyleAdaptiveLayerNorm(self.encoder_hidden) if self.use_cln else nn.LayerNorm(self.encoder_hidden)

    def forward_cf(self, x, key_mask, cond_mean):
        """x [B, C, T] (embedded already; overwritten) -> [B, C, T]"""
        x = self.position_emb.forward_cf(x)
        for layer in self.layers:
            x = layer.forward_cf(x, key_mask, cond_mean)
        if self.use_cln:
            return self.last_ln.forward_cf(x, cond_mean)
        return layer_norm_c(x, self.last_ln.weight.detach(), self.last_ln.bias.detach(), eps=self.last_ln.eps)

    def forward(self, x, key_padding_mask, condition=None):
        """x: phone ids [B, T] (with ``enc_emb_tokens``) or [B, T, d]; key_padding_mask [B, T], 0 = padded, or None; condition [B, T', d]"""
        _eval_only(self, "TransformerEncoder")
        if x.dim() == 2 and self.use_enc_emb:
            x = self.enc_emb_tokens(x)
        x = _lib.require_device_tensor(x, "TransformerEncoder input").transpose(1, 2).contiguous()
        with _lib.on_device(x.device):
            return self.forward_cf(x, _key_mask(key_padding_mask), _cond_mean(condition) if self.use_cln else None).transpose(1, 2)


class _Predictor(nn.Module):
    """the body DurationPredictor and PitchPredictor share"""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.input_size, self.filter_size, self.kernel_size = cfg.input_size, cfg.filter_size, cfg.kernel_size
        self.conv_layers, self.cross_attn_per_layer = cfg.conv_layers, cfg.cross_attn_per_layer
        self.attn_head, self.drop_out = cfg.attn_head, cfg.drop_out
        if self.kernel_size % 2 == 0:
            raise NotImplementedError("predictor: an even kernel_size changes the length")
        self.conv = nn.ModuleList()
        self.cattn = nn.ModuleList()
        for idx in range(self.conv_layers):
            in_dim = self.input_size if idx == 0 else self.filter_size
            self.conv.append(nn.Sequential(HipConv1d(in_dim, self.filter_size, self.kernel_size, padding=self.kernel_size // 2, weight_norm=False),
                                           nn.ReLU(), nn.LayerNorm(self.filter_size), nn.Dropout(self.drop_out)))
            if idx % self.cross_attn_per_layer == 0:
                self.cattn.append(nn.Sequential(nn.MultiheadAttention(self.filter_size, self.attn_head, batch_first=True, kdim=self.filter_size,
                                                                      vdim=self.filter_size), nn.LayerNorm(self.filter_size), nn.Dropout(0.2)))
        self.linear = nn.Linear(self.filter_size, 1)
        self.linear.weight.data.normal_(0.0, 0.02)
        self._kv, self._head = _RowsHandle(), _RowsHandle()
        self._rows_sig, self._kv_rows, self._head_rows = None, None, None
        self._q = [_RowsHandle() for _ in self.cattn]
        self._o = [_PwHandle() for _ in self.cattn]

    def forward_cf(self, x, ref_emb, ref_key_mask):
        """x [B, C, N], ref_emb [B, C, T'], ref_key_mask [B, T'] uint8 1 = valid -> [B, N]"""
        if self.input_size != self.filter_size:
            raise NotImplementedError("predictor: input_size != filter_size (the first cross-attention reads the input) is not on the HIP path")
        C = self.filter_size
        attns = [seq[0] for seq in self.cattn]
        for a in attns:
            _check_mha(a, "predictor")
        kv_rows, head_rows = self._stacked(attns)
        kv = _pw(self._kv, kv_rows, ref_emb)                             # [B, n * 2C, T']: k | v of every attention layer
        inv_sqrt2 = 1.0 / math.sqrt(2.0)
        for idx, seq in enumerate(self.conv):
            res = x
            if idx % self.cross_attn_per_layer == 0:
                j = idx // self.cross_attn_per_layer
                attn, ln = self.cattn[j][0], self.cattn[j][1]
                q = _pw(self._q[j], mha_rows(attn, 0, 1), layer_norm_c(x, ln.weight.detach(), ln.bias.detach(), eps=ln.eps))
                att = cross_attention(q, kv[:, 2 * C * j:2 * C * j + C], kv[:, 2 * C * j + C:2 * C * (j + 1)], self.attn_head, ref_key_mask)
                x = _pw(self._o[j], attn.out_proj, att, res=x).mul_(inv_sqrt2)
            ln = seq[2]
            x = layer_norm_c(seq[0](x, slope_out=0.0), ln.weight.detach(), ln.bias.detach(), post=res if idx else None, eps=ln.eps)
        return _pw(self._head, head_rows, x)[:, 0]

    def _stacked(self, attns):
        """the re-stacked weights, rebuilt when a parameter they are cut from changes: the k | v rows of every attention layer, and the head
        as the first of eight rows (seven of zeros: a one-row GEMM is outside what the exact-fp32 conv behind the GEMM is tested for)"""
        tensors = [t for a in attns for t in (a.in_proj_weight, a.in_proj_bias)] + [self.linear.weight, self.linear.bias]
        sig = param_sig(tensors)
        if sig != self._rows_sig:
            w, b = self.linear.weight.detach(), self.linear.bias.detach()
            self._kv_rows = stacked_kv_rows(attns)
            self._head_rows = _Rows(torch.cat((w, w.new_zeros(7, w.shape[1])), 0), torch.cat((b, b.new_zeros(7))), (self.linear.weight, self.linear.bias))
            self._rows_sig = sig
        return self._kv_rows, self._head_rows

    def _run(self, x, mask, ref_emb, ref_mask, who):
        _eval_only(self, who)
        if mask is not None:
            raise NotImplementedError(f"{who}: a frame mask is the training path; NaturalSpeech2.inference passes None")
        x = _lib.require_device_tensor(x, f"{who} input").transpose(1, 2).contiguous()
        ref = _lib.require_device_tensor(ref_emb, f"{who} prompt")
        with _lib.on_device(x.device):
            return self.forward_cf(x, ref, _key_mask(ref_mask))


class DurationPredictor(_Predictor):
    def durations(self, log_d):
        return dict(dur_pred_log=log_d, dur_pred=log_d.exp() - 1, dur_pred_round=torch.clamp(torch.round(log_d.exp() - 1), min=0).long())

    def forward(self, x, mask, ref_emb, ref_mask):
        """x [B, N, d]; mask None; ref_emb [B, d, T']; ref_mask [B, T'], 0 = padded -> dur_pred_log, dur_pred, dur_pred_round [B, N]"""
        return self.durations(self._run(x, mask, ref_emb, ref_mask, "DurationPredictor"))


class PitchPredictor(_Predictor):
    def forward(self, x, mask, ref_emb, ref_mask):
        """x [B, T, d]; mask None; ref_emb [B, d, T']; ref_mask [B, T'], 0 = padded -> pitch_pred_log [B, T]"""
        return self._run(x, mask, ref_emb, ref_mask, "PitchPredictor")


class LengthRegulator(nn.Module):
    """Length Regulator: ``amp_expand_path`` along the running sum of the truncated durations, zero beyond an item's length"""

    def forward_cf(self, x, cum, mel_len, max_len):
        return expand_path(x, cum, None, mel_len, int(max_len))[0]

    def forward(self, x, duration, max_len):
        """x [B, N, d], duration [B, N] (each truncated by int(), negatives count 0) -> ([B, max_len or the longest, d], mel_len int64 [B])"""
        x = _lib.require_device_tensor(x, "LengthRegulator input").transpose(1, 2).contiguous()
        cum = duration.to(x.device).clamp(min=0).to(torch.int32).cumsum(1).to(torch.int32).contiguous()
        mel_len = cum[:, -1].contiguous()
        Ty = int(mel_len.max().item()) if max_len is None else int(max_len)
        if Ty < 1:
            raise ValueError("LengthRegulator: every duration is zero")
        with _lib.on_device(x.device):
            out = self.forward_cf(x, cum, mel_len.clamp(max=Ty), Ty)
        return out.transpose(1, 2), mel_len.long()
