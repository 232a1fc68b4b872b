"""The decoder half of AudioLDM's ``AutoencoderKL`` (models/tta/autoencoder/autoencoder.py) in eval mode on the HIP kernels, under the
reference's names and state_dict keys: ``decode(z)`` = ``post_quant_conv`` (1 x 1) -> ``Decoder2d``.  A ``ResnetBlock`` is stats -> conv2d
(GroupNorm eps 1e-6 + swish on load) -> stats -> conv2d (norm on load, residual = x or ``nin_shortcut(x)``); ``Upsample2d`` is the conv reading
the x2 nearest up-sampling in place.  The reference builds no attention in this decoder.  ``encoder.*`` and ``quant_conv.*`` are held as plain
parameters so the full state_dict loads; ``encode`` / ``forward`` are training and preprocessing and raise."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.modules.hip_ops import Conv2d3x3, group_norm_stats

from ..ldm.attention import StackedPw, _lin


def Normalize(in_channels):
    return nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)


def _conv3(cin, cout, **kw):
    c = nn.Conv2d(cin, cout, kernel_size=3, padding=kw.pop("padding", 1), **kw)
    c._hip = Conv2d3x3()
    return c


def _normed_conv(norm, conv, x, **kw):
    return conv._hip(x, conv.weight, conv.bias, norm=(group_norm_stats(x, norm.eps), norm.weight.detach(), norm.bias.detach()), **kw)


class Upsample2d(nn.Module):
    def __init__(self, in_channels, with_conv):
        super().__init__()
        if not with_conv:
            raise NotImplementedError("Upsample2d: with_conv=False is not on the HIP path")
        self.with_conv = with_conv
        self.conv = _conv3(in_channels, in_channels)

    def forward(self, x):
        return self.conv._hip(x, self.conv.weight, self.conv.bias, up2=True)


class ResnetBlock(nn.Module):
    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout):
        super().__init__()
        if conv_shortcut:
            raise NotImplementedError("ResnetBlock: conv_shortcut is not on the HIP path")
        self.in_channels = in_channels
        self.out_channels = in_channels if out_channels is None else out_channels
        self.use_conv_shortcut = conv_shortcut
        self.norm1 = Normalize(in_channels)
        self.conv1 = _conv3(in_channels, self.out_channels)
        self.norm2 = Normalize(self.out_channels)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = _conv3(self.out_channels, self.out_channels)
        if self.in_channels != self.out_channels:
            self.nin_shortcut = nn.Conv2d(in_channels, self.out_channels, kernel_size=1, stride=1, padding=0)
            self._nin = StackedPw()

    def forward(self, x):
        if self.training:
            raise NotImplementedError("ResnetBlock: training mode is not on the HIP path: call .eval()")
        x = _lib.require_device_tensor(x, "ResnetBlock input")
        B, C, H, W = x.shape
        h = _normed_conv(self.norm1, self.conv1, x)
        if self.in_channels != self.out_channels:
            x = _lin(self._nin, self.nin_shortcut, x.reshape(B, C, H * W)).reshape(B, self.out_channels, H, W)
        return _normed_conv(self.norm2, self.conv2, h, residual=x)


class _EncoderParams(nn.Module):
    """``Encoder2d``'s parameters under its keys (autoencoder.py:167-228); the encoder is preprocessing and is not run here"""

    def __init__(self, *, ch, ch_mult, num_res_blocks, in_channels, z_channels, double_z=True):
        super().__init__()
        self.conv_in = nn.Conv2d(in_channels, ch, kernel_size=3, stride=1, padding=1)
        in_ch_mult = (1,) + tuple(ch_mult)
        self.down = nn.ModuleList()
        block_in = ch
        for i_level in range(len(ch_mult)):
            block = nn.ModuleList()
            block_in, block_out = ch * in_ch_mult[i_level], ch * ch_mult[i_level]
            for _ in range(num_res_blocks):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, dropout=0.0))
                block_in = block_out
            down = nn.Module()
            down.block = block
            if i_level != len(ch_mult) - 1:
                down.downsample = nn.Module()
                down.downsample.conv = nn.Conv2d(block_in, block_in, kernel_size=3, stride=2, padding=0)
            self.down.append(down)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, dropout=0.0)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, dropout=0.0)
        self.norm_out = Normalize(block_in)
        self.conv_out = nn.Conv2d(block_in, 2 * z_channels if double_z else z_channels, kernel_size=3, stride=1, padding=1)

    def forward(self, x):
        raise NotImplementedError("AutoencoderKL.encoder: the encoder is preprocessing and is not on the HIP path")


class Decoder2d(nn.Module):
    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, dropout=0.0, resamp_with_conv=True, in_channels, z_channels,
                 give_pre_end=False, **ignorekwargs):
        super().__init__()
        self.ch = ch
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.in_channels = in_channels
        self.give_pre_end = give_pre_end
        block_in = ch * ch_mult[self.num_resolutions - 1]
        self.conv_in = _conv3(z_channels, block_in)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, dropout=dropout)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, dropout=dropout)
        self.up = nn.ModuleList()
        for i_level in reversed(range(self.num_resolutions)):
            block = nn.ModuleList()
            block_out = ch * ch_mult[i_level]
            for _ in range(self.num_res_blocks + 1):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, dropout=dropout))
                block_in = block_out
            up = nn.Module()
            up.block = block
            up.attn = nn.ModuleList()
            if i_level != 0:
                up.upsample = Upsample2d(block_in, resamp_with_conv)
            self.up.insert(0, up)
        self.norm_out = Normalize(block_in)
        self.conv_out = _conv3(block_in, out_ch)

    def forward(self, z):
        if self.training:
            raise NotImplementedError("Decoder2d: training mode is not on the HIP path: call .eval()")
        z = _lib.require_device_tensor(z, "Decoder2d input")
        self.last_z_shape = z.shape
        h = self.conv_in._hip(z, self.conv_in.weight, self.conv_in.bias)
        h = self.mid.block_2(self.mid.block_1(h))
        for i_level in reversed(range(self.num_resolutions)):
            for blk in self.up[i_level].block:
                h = blk(h)
            if i_level != 0:
                h = self.up[i_level].upsample(h)
        if self.give_pre_end:
            return h
        return _normed_conv(self.norm_out, self.conv_out, h)


class AutoencoderKL(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        if not cfg.double_z:
            raise NotImplementedError("AutoencoderKL: double_z=False is not built (the reference asserts it)")
        self.encoder = _EncoderParams(ch=cfg.ch, ch_mult=list(cfg.ch_mult), num_res_blocks=cfg.num_res_blocks, in_channels=cfg.in_channels,
                                      z_channels=cfg.z_channels, double_z=cfg.double_z)
        self.decoder = Decoder2d(ch=cfg.ch, ch_mult=list(cfg.ch_mult), num_res_blocks=cfg.num_res_blocks, out_ch=cfg.out_ch,
                                 z_channels=cfg.z_channels, in_channels=None)
        self.quant_conv = nn.Conv2d(2 * cfg.z_channels, 2 * cfg.z_channels, 1)
        self.post_quant_conv = nn.Conv2d(cfg.z_channels, cfg.z_channels, 1)
        self.embed_dim = cfg.z_channels
        self._pq = StackedPw()

    def encode(self, x):
        raise NotImplementedError("AutoencoderKL.encode: the encoder is training and preprocessing, not on the HIP path")

    def forward(self, input, sample_posterior=True):
        raise NotImplementedError("AutoencoderKL.forward: encode is training and preprocessing, not on the HIP path; use decode")

    @torch.no_grad()
    def decode(self, z):
        """z [B, z_channels, H, W] -> [B, out_ch, H * 2^(levels - 1), W * 2^(levels - 1)]"""
        z = _lib.require_device_tensor(z, "AutoencoderKL.decode input")
        B, C, H, W = z.shape
        z = _lin(self._pq, self.post_quant_conv, z.reshape(B, C, H * W)).reshape(B, C, H, W)
        return self.decoder(z)
