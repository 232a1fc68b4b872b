"""DualCodec's ConvNeXt block (model_codec/cnn.py:12-102) on the gfx950 kernels, on channel-first [B, C, T] activations:

    [F.pad(x, (6, 0)) ->] dwconv (k = 7, groups = C) -> LayerNorm    one launch: amp_dwconv_layer_norm_c_causal (is_causal) or
                                                                   amp_dwconv_layer_norm_c (padding 3)
    pwconv1 -> GELU                                                pointwise f16x3 GEMM, GELU epilogue (amp_pw_forward)
    pwconv2 [-> gamma *] -> + residual                             pointwise f16x3 GEMM, scale + residual epilogue, in place

Same constructor arguments and ``state_dict`` keys as the reference; ``gamma`` exists only for ``layer_scale_init_value > 0`` (the
epilogue then scales by a vector of ones, which is exact).  AdaLayerNorm is refused, as in the Vocos drop-in."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.vocos import LN_EPS, _check_input, _check_tensors, _no_adanorm, _PwHandle, pw_forward


class ConvNeXtBlock(nn.Module):
    def __init__(self, dim: int, intermediate_dim: int, layer_scale_init_value: float = 0.0, adanorm_num_embeddings: Optional[int] = None,
                 is_causal=False):
        super().__init__()
        _no_adanorm(adanorm_num_embeddings)
        self.is_causal = bool(is_causal)
        self.dwconv = nn.Conv1d(dim, dim, kernel_size=7, padding=0 if is_causal else 3, groups=dim)
        self.adanorm = False
        self.norm = nn.LayerNorm(dim, eps=LN_EPS)
        self.pwconv1 = nn.Linear(dim, intermediate_dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(intermediate_dim, dim)
        self.gamma = (nn.Parameter(layer_scale_init_value * torch.ones(dim), requires_grad=True) if layer_scale_init_value > 0 else None)
        self._pw1, self._pw2 = _PwHandle(), _PwHandle()
        self._ones = {}

    def run(self, x, y, h):
        """x [B, dim, T] updated in place; y [B, dim, T] and h [B, intermediate, T] are scratch"""
        B, C, T = x.shape
        dev = x.device
        L = _lib.lib()
        front = L.amp_dwconv_layer_norm_c_causal if self.is_causal else L.amp_dwconv_layer_norm_c
        _lib.check(front(_p(x), _p(self.dwconv.weight), _p(self.dwconv.bias), 7, 1, _p(self.norm.weight), _p(self.norm.bias), None, B, C, T,
                         LN_EPS, 0, _p(y), _lib.current_stream_ptr(dev)))
        pw_forward(self._pw1, self.pwconv1, y, _lib.AMP_PW_BIAS_GELU, h)
        gamma = self.gamma
        if gamma is None:
            gamma = self._ones.get(str(dev))
            if gamma is None:
                gamma = self._ones[str(dev)] = torch.ones(C, device=dev)
        pw_forward(self._pw2, self.pwconv2, h, _lib.AMP_PW_SCALE_RES, x, gamma=gamma, res=x)
        return x

    def forward(self, x, cond_embedding_id=None):
        x = _check_input(x, self.dwconv.in_channels, "ConvNeXtBlock").clone()
        _check_tensors(self, x.device, "ConvNeXtBlock")
        y = torch.empty_like(x)
        h = torch.empty((x.shape[0], self.pwconv1.out_features, x.shape[2]), device=x.device)
        with _lib.on_device(x.device):
            self.run(x, y, h)
        _lib.range_check(x.device)
        return x


def run_blocks(blocks, x):
    """the ConvNeXt blocks of a stack on one set of scratch buffers; x [B, dim, T] is updated in place"""
    blocks = list(blocks)
    if blocks:
        y = torch.empty_like(x)
        h = torch.empty((x.shape[0], blocks[0].pwconv1.out_features, x.shape[2]), device=x.device)
        for blk in blocks:
            blk.run(x, y, h)
    return x
