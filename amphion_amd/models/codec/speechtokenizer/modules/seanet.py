"""SEANet encoder / decoder drop-ins (models/codec/speechtokenizer/modules/seanet.py:42-396) on the gfx950 kernels, eval mode only.  Same class
names, constructor arguments, module indices and ``state_dict`` keys.  The ``nn.ELU`` modules keep the reference's places in the Sequentials;
the forward folds each into the staging pass of the conv behind it:

    ELU -> SConv1d            amp_elu_pad (ELU + reflect pad) -> conv with padding 0 (implicit-GEMM kernels; strided: amp_sconv_forward)
    SEANetResnetBlock         shortcut(x) + block(x): the sum is the ``res`` argument of the block's last conv
    SLSTM                     amp_lstm_forward
    ELU -> SConvTranspose1d   amp_elu_pad (zero pads) -> amp_tconv_forward

Built: ``activation="ELU"``, ``norm="weight_norm"``, ``causal=False``, ``pad_mode="reflect"``, either ``true_skip`` value.  ``Snake``, the other
norms, causal mode and ``.train()`` raise ``NotImplementedError``.  Both forwards end with the op-level range check (``_lib.range_check``)."""
from __future__ import annotations

import typing as tp

import numpy as np
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.codec.amphion_codec.codec import _check_channels
from amphion_amd.models.codec.amphion_codec.vocos import _check_tensors

from .conv import SConv1d, SConvTranspose1d
from .lstm import SLSTM


def _elu(activation, activation_params, who):
    if activation != "ELU":
        raise NotImplementedError(f"{who}: activation={activation!r} is not on the HIP path (built: 'ELU')")
    return nn.ELU(**activation_params)


def _eval_only(module, who):
    if module.training:
        raise NotImplementedError(f"{who}: training mode is not on the HIP path (the kernels have no backward): call .eval()")


def _run_sequence(modules, x):
    """walk a SEANet Sequential: an ELU is carried into the conv behind it"""
    alpha = None
    for m in modules:
        if isinstance(m, nn.ELU):
            alpha = float(m.alpha)
            continue
        if isinstance(m, (SConv1d, SConvTranspose1d)):
            x = m.run(x, elu_alpha=alpha)
        elif alpha is not None:
            raise NotImplementedError(f"SEANet: an ELU in front of {type(m).__name__} is not on the HIP path")
        else:
            x = m.run(x)
        alpha = None
    if alpha is not None:
        raise NotImplementedError("SEANet: a trailing ELU is not on the HIP path")
    return x


class SEANetResnetBlock(nn.Module):
    def __init__(self, dim: int, kernel_sizes: tp.List[int] = [3, 1], dilations: tp.List[int] = [1, 1], activation: str = "ELU",
                 activation_params: dict = {"alpha": 1.0}, norm: str = "weight_norm", norm_params: tp.Dict[str, tp.Any] = {},
                 causal: bool = False, pad_mode: str = "reflect", compress: int = 2, true_skip: bool = True):
        super().__init__()
        assert len(kernel_sizes) == len(dilations), "Number of kernel sizes should match number of dilations"
        hidden = dim // compress
        block = []
        for i, (kernel_size, dilation) in enumerate(zip(kernel_sizes, dilations)):
            in_chs = dim if i == 0 else hidden
            out_chs = dim if i == len(kernel_sizes) - 1 else hidden
            block += [_elu(activation, activation_params, "SEANetResnetBlock"),
                      SConv1d(in_chs, out_chs, kernel_size=kernel_size, dilation=dilation, norm=norm, norm_kwargs=norm_params, causal=causal,
                              pad_mode=pad_mode)]
        self.dim = dim
        self.block = nn.Sequential(*block)
        self.shortcut: nn.Module
        if true_skip:
            self.shortcut = nn.Identity()
        else:
            self.shortcut = SConv1d(dim, dim, kernel_size=1, norm=norm, norm_kwargs=norm_params, causal=causal, pad_mode=pad_mode)

    def run(self, x):
        res = x if isinstance(self.shortcut, nn.Identity) else self.shortcut.run(x)
        mods = list(self.block)
        h = x
        for i in range(0, len(mods), 2):
            last = i + 2 == len(mods)
            h = mods[i + 1].run(h, elu_alpha=float(mods[i].alpha), res=res if last else None)
        return h

    def forward(self, x):
        _eval_only(self, "SEANetResnetBlock")
        x = _check_channels(x, self.dim, "SEANetResnetBlock")
        _check_tensors(self, x.device, "SEANetResnetBlock")
        with _lib.on_device(x.device):
            y = self.run(x)
        _lib.range_check(x.device)
        return y


class SEANetEncoder(nn.Module):
    def __init__(self, channels: int = 1, dimension: int = 128, n_filters: int = 32, n_residual_layers: int = 1,
                 ratios: tp.List[int] = [8, 5, 4, 2], activation: str = "ELU", activation_params: dict = {"alpha": 1.0},
                 norm: str = "weight_norm", norm_params: tp.Dict[str, tp.Any] = {}, kernel_size: int = 7, last_kernel_size: int = 7,
                 residual_kernel_size: int = 3, dilation_base: int = 2, causal: bool = False, pad_mode: str = "reflect",
                 true_skip: bool = False, compress: int = 2, lstm: int = 2, bidirectional: bool = False):
        super().__init__()
        self.channels = channels
        self.dimension = dimension
        self.n_filters = n_filters
        self.ratios = list(reversed(ratios))
        del ratios
        self.n_residual_layers = n_residual_layers
        self.hop_length = np.prod(self.ratios)

        mult = 1
        model: tp.List[nn.Module] = [SConv1d(channels, mult * n_filters, kernel_size, norm=norm, norm_kwargs=norm_params, causal=causal,
                                             pad_mode=pad_mode)]
        for i, ratio in enumerate(self.ratios):
            for j in range(n_residual_layers):
                model += [SEANetResnetBlock(mult * n_filters, kernel_sizes=[residual_kernel_size, 1], dilations=[dilation_base ** j, 1], norm=norm,
                                            norm_params=norm_params, activation=activation, activation_params=activation_params, causal=causal,
                                            pad_mode=pad_mode, compress=compress, true_skip=true_skip)]
            model += [_elu(activation, activation_params, "SEANetEncoder"),
                      SConv1d(mult * n_filters, mult * n_filters * 2, kernel_size=ratio * 2, stride=ratio, norm=norm, norm_kwargs=norm_params,
                              causal=causal, pad_mode=pad_mode)]
            mult *= 2
        if lstm:
            model += [SLSTM(mult * n_filters, num_layers=lstm, bidirectional=bidirectional)]
        mult = mult * 2 if bidirectional else mult
        model += [_elu(activation, activation_params, "SEANetEncoder"),
                  SConv1d(mult * n_filters, dimension, last_kernel_size, norm=norm, norm_kwargs=norm_params, causal=causal, pad_mode=pad_mode)]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        """x [B, channels, T] -> [B, dimension, ceil(T / hop_length)]"""
        _eval_only(self, "SEANetEncoder")
        x = _check_channels(x, self.channels, "SEANetEncoder")
        dev = x.device
        _check_tensors(self, dev, "SEANetEncoder")
        with _lib.on_device(dev):
            y = _run_sequence(self.model, x)
        _lib.range_check(dev)
        return y


class SEANetDecoder(nn.Module):
    def __init__(self, channels: int = 1, dimension: int = 128, n_filters: int = 32, n_residual_layers: int = 1,
                 ratios: tp.List[int] = [8, 5, 4, 2], activation: str = "ELU", activation_params: dict = {"alpha": 1.0},
                 final_activation: tp.Optional[str] = None, final_activation_params: tp.Optional[dict] = None, norm: str = "weight_norm",
                 norm_params: tp.Dict[str, tp.Any] = {}, kernel_size: int = 7, last_kernel_size: int = 7, residual_kernel_size: int = 3,
                 dilation_base: int = 2, causal: bool = False, pad_mode: str = "reflect", true_skip: bool = False, compress: int = 2,
                 lstm: int = 2, trim_right_ratio: float = 1.0, bidirectional: bool = False):
        super().__init__()
        self.dimension = dimension
        self.channels = channels
        self.n_filters = n_filters
        self.ratios = ratios
        del ratios
        self.n_residual_layers = n_residual_layers
        self.hop_length = np.prod(self.ratios)
        if final_activation is not None:
            raise NotImplementedError(f"SEANetDecoder: final_activation={final_activation!r} is not on the HIP path (SpeechTokenizer has none)")

        mult = int(2 ** len(self.ratios))
        model: tp.List[nn.Module] = [SConv1d(dimension, mult * n_filters, kernel_size, norm=norm, norm_kwargs=norm_params, causal=causal,
                                             pad_mode=pad_mode)]
        if lstm:
            model += [SLSTM(mult * n_filters, num_layers=lstm, bidirectional=bidirectional)]
        for i, ratio in enumerate(self.ratios):
            model += [_elu(activation, activation_params, "SEANetDecoder"),
                      SConvTranspose1d(mult * n_filters, mult * n_filters // 2, kernel_size=ratio * 2, stride=ratio, norm=norm,
                                       norm_kwargs=norm_params, causal=causal, trim_right_ratio=trim_right_ratio)]
            for j in range(n_residual_layers):
                model += [SEANetResnetBlock(mult * n_filters // 2, kernel_sizes=[residual_kernel_size, 1], dilations=[dilation_base ** j, 1],
                                            activation=activation, activation_params=activation_params, norm=norm, norm_params=norm_params,
                                            causal=causal, pad_mode=pad_mode, compress=compress, true_skip=true_skip)]
            mult //= 2
        model += [_elu(activation, activation_params, "SEANetDecoder"),
                  SConv1d(n_filters, channels, last_kernel_size, norm=norm, norm_kwargs=norm_params, causal=causal, pad_mode=pad_mode)]
        self.model = nn.Sequential(*model)

    def forward(self, z):
        """z [B, dimension, T] -> [B, channels, T * hop_length]"""
        _eval_only(self, "SEANetDecoder")
        z = _check_channels(z, self.dimension, "SEANetDecoder")
        dev = z.device
        _check_tensors(self, dev, "SEANetDecoder")
        with _lib.on_device(dev):
            y = _run_sequence(self.model, z)
        _lib.range_check(dev)
        return y
