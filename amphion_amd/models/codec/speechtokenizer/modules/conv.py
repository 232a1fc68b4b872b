"""SConv1d / SConvTranspose1d drop-ins (models/codec/speechtokenizer/modules/conv.py:228-346) on the gfx950 kernels, eval mode only.  Same
constructor arguments and ``state_dict`` keys (``conv.conv.{bias,weight_g,weight_v}`` / ``convtr.convtr.{..}``; a folded ``weight`` loads too).

    SConv1d            reflect pad (asymmetric, with get_extra_padding_for_conv1d and pad1d's small-input rule) -> conv
                       amp_elu_pad stages the padded tensor -- with the ELU that precedes the conv everywhere in SEANet folded in when the
                       caller passes ``elu_alpha`` -- and the conv runs with padding = 0: stride 1 on the implicit-GEMM kernels (HipConv1d),
                       Conv1d(k = 2 s, stride s) on amp_sconv_forward
    SConvTranspose1d   ConvTranspose1d(k = 2 s, stride s) and the trim (left s - s // 2, right s // 2) are amp_tconv_forward with
                       padding = s - s // 2, output_padding = s % 2; the preceding ELU is amp_elu_pad with zero pads

Built: ``norm="weight_norm"`` (or ``"none"``), ``causal=False``, ``pad_mode="reflect"``, ``groups=1``.  Anything else raises
``NotImplementedError``."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.codec import _StridedConv, _TransposedConv
from amphion_amd.models.codec.amphion_codec.vocos import _check_input
from amphion_amd.modules.hip_ops import HipConv1d


def _built(who, norm, causal, pad_mode="reflect", groups=1):
    if norm not in ("weight_norm", "none"):
        raise NotImplementedError(f"{who}: norm={norm!r} is not on the HIP path (built: 'weight_norm' and 'none')")
    if causal:
        raise NotImplementedError(f"{who}: causal=True is not on the HIP path (SpeechTokenizer is built non-causal)")
    if pad_mode != "reflect":
        raise NotImplementedError(f"{who}: pad_mode={pad_mode!r} is not on the HIP path (built: 'reflect')")
    if groups != 1:
        raise NotImplementedError(f"{who}: groups={groups} is not on the HIP path")


def get_extra_padding_for_conv1d(length: int, kernel_size: int, stride: int, padding_total: int = 0) -> int:
    """conv.py:70-77 in integers: ceil((length - k + p) / stride) windows after the first"""
    n = length - kernel_size + padding_total
    frames = -(-n // stride) + 1
    return (frames - 1) * stride + (kernel_size - padding_total) - length


def elu_pad(x, pad_left=0, pad_right=0, elu_alpha=None):
    """act(reflect_pad(x)) in one pass (``amp_elu_pad``): ``elu_alpha`` None is the identity, a float is ELU with that alpha"""
    B, C, T = x.shape
    y = torch.empty((B, C, T + pad_left + pad_right), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().amp_elu_pad(_p(x), B, C, T, int(pad_left), int(pad_right), int(elu_alpha is not None),
                                      float(elu_alpha if elu_alpha is not None else 1.0), _p(y), _lib.current_stream_ptr(x.device)))
    return y


class NormConv1d(nn.Module):
    """holds the conv under the reference's key ``conv``; the norms that would add a module are refused"""

    def __init__(self, conv):
        super().__init__()
        self.conv = conv
        self.norm = nn.Identity()


class NormConvTranspose1d(nn.Module):
    def __init__(self, convtr):
        super().__init__()
        self.convtr = convtr
        self.norm = nn.Identity()


class SConv1d(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int = 1, dilation: int = 1, groups: int = 1,
                 bias: bool = True, causal: bool = False, norm: str = "none", norm_kwargs: dict = {}, pad_mode: str = "reflect"):
        super().__init__()
        _built("SConv1d", norm, causal, pad_mode, groups)
        wn = norm == "weight_norm"
        if stride == 1:
            conv = HipConv1d(in_channels, out_channels, kernel_size, dilation=dilation, padding=0, weight_norm=wn, bias=bias)
        else:
            if kernel_size != 2 * stride or dilation != 1 or not bias or not wn:
                raise NotImplementedError("SConv1d: a strided conv is on the HIP path as the weight-normed Conv1d(k = 2 * stride, stride) with a "
                                          f"bias that SEANet builds, got k={kernel_size} stride={stride} dilation={dilation}")
            conv = _StridedConv(in_channels, out_channels, stride, 0)
        self.conv = NormConv1d(conv)
        self.in_channels, self.kernel_size, self.stride, self.dilation = in_channels, kernel_size, stride, dilation
        self.causal, self.pad_mode = causal, pad_mode

    def paddings(self, T):
        """(left, right) of conv.py:274-287"""
        total = (self.kernel_size - 1) * self.dilation - (self.stride - 1)
        extra = get_extra_padding_for_conv1d(T, self.kernel_size, self.stride, total)
        right = total // 2
        return total - right, right + extra

    def run(self, x, elu_alpha=None, res=None):
        """conv(reflect_pad(ELU(x))) (+ res): the activation in front of the conv and the sum behind it ride on the two launches"""
        if res is not None and self.stride != 1:
            raise ValueError("SConv1d: a strided conv has no residual argument (amp_sconv_forward)")
        pl, pr = self.paddings(x.shape[-1])
        xp = x if (pl == 0 and pr == 0 and elu_alpha is None) else elu_pad(x, pl, pr, elu_alpha)     # a bare k = 1 conv needs no staging
        if self.stride == 1:
            return self.conv.conv(xp, res=res)
        return self.conv.conv(xp)

    def forward(self, x):
        x = _check_input(x, self.in_channels, "SConv1d")
        with _lib.on_device(x.device):
            return self.run(x)


class SConvTranspose1d(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int = 1, causal: bool = False, norm: str = "none",
                 trim_right_ratio: float = 1.0, norm_kwargs: dict = {}):
        super().__init__()
        _built("SConvTranspose1d", norm, causal)
        if kernel_size != 2 * stride or stride < 2 or norm != "weight_norm":
            raise NotImplementedError("SConvTranspose1d: on the HIP path as the weight-normed ConvTranspose1d(k = 2 * stride, stride >= 2) that "
                                      f"SEANet builds, got k={kernel_size} stride={stride} norm={norm!r}")
        assert trim_right_ratio == 1.0, "`trim_right_ratio` != 1.0 only makes sense for causal convolutions"
        self.convtr = NormConvTranspose1d(_TransposedConv(in_channels, out_channels, stride, stride - stride // 2, stride % 2))
        self.in_channels, self.causal, self.trim_right_ratio = in_channels, causal, trim_right_ratio

    def run(self, x, elu_alpha=None):
        if elu_alpha is not None:
            x = elu_pad(x, 0, 0, elu_alpha)
        return self.convtr.convtr(x)

    def forward(self, x):
        x = _check_input(x, self.in_channels, "SConvTranspose1d")
        with _lib.on_device(x.device):
            return self.run(x)
