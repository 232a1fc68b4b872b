"""The spatial transformer of AudioLDM's UNet (models/tta/ldm/attention.py) in eval mode on the HIP kernels, under the reference's names and
state_dict keys.  Everything is channel-first: a feature map [B, C, H, W] is the token sequence [B, C, T] with T = H * W as it stands, so the
reference's ``rearrange "b c h w -> b (h w) c"`` costs nothing.

One ``BasicTransformerBlock`` is: ``amp_layer_norm_c`` -> stacked q | k | v GEMM -> ``amp_cross_attention_hd`` -> ``to_out`` with the residual
epilogue; LayerNorm -> ``to_q`` -> attention against the context's k | v -> ``to_out`` with the residual; LayerNorm -> stacked GEGLU GEMM ->
``amp_geglu`` -> GEMM with the residual.  The context's k | v do not depend on x or t: ``UNetModel.prepare_context`` forms them for all layers
in one GEMM and hands each block its row block."""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import AMP_PW_BIAS, AMP_PW_SCALE_RES
from amphion_amd._lib import ptr as _p
from amphion_amd.modules.hip_ops import cross_attention_hd, geglu, group_norm, layer_norm_c

_ones = {}


def _gamma_one(n, device):
    t = _ones.get((n, device))
    if t is None:
        t = _ones[(n, device)] = torch.ones(n, dtype=torch.float32, device=device)
    return t


class StackedPw:
    """The packed device copy (``amp_pw``) of one or several weight matrices stacked along their rows -- nn.Linear weights [out, in] or 1 x 1
    nn.Conv2d weights [out, in, 1, 1], each with its bias or None -- rebuilt when a parameter, the device or the precision changes."""

    def __init__(self):
        self._cache = HandleCache("amp_pw_destroy")
        self.cout = 0

    def get(self, weights, biases, device):
        sig = param_sig(tuple(weights) + tuple(biases), str(device), _lib.get_precision(), len(weights))
        c = self._cache
        return c.handle if sig == c.sig else c.build(sig, self._build, weights, biases, device)

    def _build(self, weights, biases, device):
        w = torch.cat([host_f32(t).reshape(t.shape[0], -1) for t in weights], 0).contiguous()
        b = None
        if any(t is not None for t in biases):
            b = torch.cat([torch.zeros(wt.shape[0]) if t is None else host_f32(t) for wt, t in zip(weights, biases)], 0).contiguous()
        self.cout = w.shape[0]
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_pw_create(w.shape[1], w.shape[0], _p(w), _p(b), ctypes.byref(h)))
        return h

    def __call__(self, weights, biases, x, res=None):
        """x [B, cin, T] (contiguous) -> [B, cout, T], + res after the accumulation"""
        dev = x.device
        h = self.get(weights, biases, dev)
        B, T = x.shape[0], x.shape[2]
        out = torch.empty((B, self.cout, T), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            if res is None:
                _lib.check(_lib.lib().amp_pw_forward(h, _p(x), 0, B, T, AMP_PW_BIAS, None, None, _p(out), _lib.current_stream_ptr(dev)))
            else:
                _lib.check(_lib.lib().amp_pw_forward(h, _p(x), 0, B, T, AMP_PW_SCALE_RES, _p(_gamma_one(self.cout, dev)), _p(res), _p(out),
                                                     _lib.current_stream_ptr(dev)))
        return out


def _lin(pw, lin, x, res=None):
    return pw([lin.weight], [lin.bias], x, res)


def _cf(x, who):
    """[B, C, T] contiguous fp32 on the device"""
    x = _lib.require_device_tensor(x, who)
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError(f"{who}: expected a non-empty [B, C, T] tensor, got {tuple(x.shape)}")
    return x


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)
        self._h = StackedPw()

    def forward_cf(self, x):
        return geglu(_lin(self._h, self.proj, x))

    def forward(self, x):
        """x [B, T, dim_in] -> [B, T, dim_out]"""
        return self.forward_cf(x.transpose(1, 2).contiguous()).transpose(1, 2)


class FeedForward(nn.Module):
    def __init__(self, dim, dim_out=None, mult=4, glu=False, dropout=0.0):
        super().__init__()
        if not glu:
            raise NotImplementedError("FeedForward: glu=False is not on the HIP path (AudioLDM's blocks are gated)")
        inner_dim = int(dim * mult)
        dim_out = dim if dim_out is None else dim_out
        self.net = nn.Sequential(GEGLU(dim, inner_dim), nn.Dropout(dropout), nn.Linear(inner_dim, dim_out))
        self._h = StackedPw()

    def forward_cf(self, x, res=None):
        return _lin(self._h, self.net[2], self.net[0].forward_cf(x), res)

    def forward(self, x):
        return self.forward_cf(x.transpose(1, 2).contiguous()).transpose(1, 2)


class CrossAttention(nn.Module):
    """``to_q`` / ``to_k`` / ``to_v`` without bias, ``to_out.0`` with one, scale = dim_head ** -0.5 (attention.py:201-241); no mask"""

    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.0):
        super().__init__()
        inner_dim = dim_head * heads
        context_dim = query_dim if context_dim is None else context_dim
        if dim_head not in (32, 64, 128):
            raise NotImplementedError(f"CrossAttention: dim_head={dim_head} is not on the HIP path (amp_cross_attention_hd: 32, 64 or 128)")
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.inner_dim = inner_dim
        self.to_q = nn.Linear(query_dim, inner_dim, bias=False)
        self.to_k = nn.Linear(context_dim, inner_dim, bias=False)
        self.to_v = nn.Linear(context_dim, inner_dim, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, query_dim), nn.Dropout(dropout))
        self._qkv, self._q, self._kv, self._o = StackedPw(), StackedPw(), StackedPw(), StackedPw()

    def kv_of(self, context_cf):
        """k | v [B, 2 * inner, Tk] of a channel-first context [B, context_dim, Tk]"""
        return self._kv([self.to_k.weight, self.to_v.weight], [None, None], context_cf)

    def forward_cf(self, x, kv=None, res=None):
        """x [B, query_dim, T]; kv: the context's k | v (``kv_of``), or None for self-attention; -> to_out(attention) (+ res)"""
        C = self.inner_dim
        if kv is None:
            qkv = self._qkv([self.to_q.weight, self.to_k.weight, self.to_v.weight], [None, None, None], x)
            att = cross_attention_hd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], self.heads, scale=self.scale)
        else:
            q = _lin(self._q, self.to_q, x)
            att = cross_attention_hd(q, kv[:, :C], kv[:, C:], self.heads, scale=self.scale)
        return _lin(self._o, self.to_out[0], att, res)

    def forward(self, x, context=None, mask=None):
        """x [B, T, query_dim], context [B, Tk, context_dim] or None -> [B, T, query_dim]"""
        if mask is not None:
            raise NotImplementedError("CrossAttention: mask is not on the HIP path (the UNet passes none)")
        kv = None if context is None else self.kv_of(_cf(context.transpose(1, 2).contiguous(), "CrossAttention context"))
        return self.forward_cf(_cf(x.transpose(1, 2).contiguous(), "CrossAttention input"), kv).transpose(1, 2)


class BasicTransformerBlock(nn.Module):
    """``attn1(norm1(x)) + x``, ``attn2(norm2(x), context) + x``, ``ff(norm3(x)) + x`` (attention.py:277-281); LayerNorm eps 1e-5"""

    def __init__(self, dim, n_heads, d_head, dropout=0.0, context_dim=None, gated_ff=True, checkpoint=True):
        super().__init__()
        self.attn1 = CrossAttention(query_dim=dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.ff = FeedForward(dim, dropout=dropout, glu=gated_ff)
        self.attn2 = CrossAttention(query_dim=dim, context_dim=context_dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.norm3 = nn.LayerNorm(dim)
        self.checkpoint = checkpoint        # the reference's checkpointing runs the function under no_grad: no effect on values

    @staticmethod
    def _ln(ln, x):
        return layer_norm_c(x, ln.weight.detach(), ln.bias.detach(), eps=ln.eps)

    def forward_cf(self, x, kv=None):
        """x [B, dim, T]; kv: attn2's k | v of the context, or None (attn2 is then a second self-attention, as in the reference)"""
        x = self.attn1.forward_cf(self._ln(self.norm1, x), None, res=x)
        x = self.attn2.forward_cf(self._ln(self.norm2, x), kv, res=x)
        return self.ff.forward_cf(self._ln(self.norm3, x), res=x)

    def forward(self, x, context=None):
        kv = None if context is None else self.attn2.kv_of(_cf(context.transpose(1, 2).contiguous(), "BasicTransformerBlock context"))
        return self.forward_cf(_cf(x.transpose(1, 2).contiguous(), "BasicTransformerBlock input"), kv).transpose(1, 2)


class SpatialTransformer(nn.Module):
    """GroupNorm (eps 1e-6, no SiLU) -> ``proj_in`` (1 x 1) -> blocks -> ``proj_out`` (1 x 1) -> ``+ x_in`` (attention.py:318-329)"""

    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0.0, context_dim=None):
        super().__init__()
        self.in_channels = in_channels
        inner_dim = n_heads * d_head
        self.norm = nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)
        self.proj_in = nn.Conv2d(in_channels, inner_dim, kernel_size=1, stride=1, padding=0)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(inner_dim, n_heads, d_head, dropout=dropout, context_dim=context_dim) for _ in range(depth)])
        self.proj_out = nn.Conv2d(inner_dim, in_channels, kernel_size=1, stride=1, padding=0)
        for p in self.proj_out.parameters():
            p.detach().zero_()
        self._in, self._out = StackedPw(), StackedPw()

    def forward(self, x, context=None):
        """x [B, C, H, W]; context [B, Tk, context_dim], None, or a list with the k | v tensor of each block (``UNetModel.prepare_context``)"""
        if self.training:
            raise NotImplementedError("SpatialTransformer: training mode is not on the HIP path: call .eval()")
        x = _lib.require_device_tensor(x, "SpatialTransformer input")
        B, C, H, W = x.shape
        if isinstance(context, (list, tuple)):
            kvs = list(context)
        elif context is None:
            kvs = [None] * len(self.transformer_blocks)
        else:
            ctx = _cf(context.transpose(1, 2).contiguous(), "SpatialTransformer context")
            kvs = [blk.attn2.kv_of(ctx) for blk in self.transformer_blocks]
        x_in = x.reshape(B, C, H * W)
        n = group_norm(x_in, self.norm.weight.detach(), self.norm.bias.detach(), self.norm.eps)
        t = _lin(self._in, self.proj_in, n)
        for blk, kv in zip(self.transformer_blocks, kvs):
            t = blk.forward_cf(t, kv)
        return _lin(self._out, self.proj_out, t, res=x_in).reshape(B, C, H, W)
