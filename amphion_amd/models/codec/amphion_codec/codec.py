"""Amphion acoustic codec drop-in (models/codec/amphion_codec/codec.py:34-428) on the gfx950 kernels: what MaskGCT / DebaTTS / Metis build as
``CodecEncoder`` + ``CodecDecoder`` (models/tts/maskgct/maskgct_utils.py:66-72).  Same constructors (``cfg=`` form included), ``state_dict`` keys
(weight-normed ``weight_g`` / ``weight_v`` or folded ``weight``) and call contracts.

    CodecEncoder   first conv (1 -> d_model, k = 7)              implicit-GEMM conv kernel (HipConv1d)
                   per EncoderBlock: 3 x ResidualUnit            ONE fused launch each up to C = 96 (csrc/codec_unit_f16x3.hip; built to C = 192),
                                                                 else amp_snake -> conv -> amp_snake -> conv + residual (amp_codec_unit_forward)
                                     Snake -> strided conv       Snake + space-to-depth, then a k = 2 conv (amp_sconv_forward)
                   Snake -> last conv (k = 3) [-> tanh]          amp_snake, HipConv1d (tanh on store)
    DecoderBlock   Snake -> ConvTranspose1d(k = 2 s, stride s)   ONE fused launch (csrc/tconv_f16x3.hip; built to cin = 384, s = 2 .. 8), else amp_snake ->
                                                                 the polyphase transposed conv (amp_tconv_forward); then 3 x ResidualUnit as above
    CodecDecoder   quantizer (ResidualVQ, "fvq")                 exact-fp32 quantizer kernels (csrc/fvq.hip): quantize / vq2emb one launch each
                   model (use_vocos=True)                        the Vocos of this package

After an encoder forward the op-level f16x3 range flag is checked (``_lib.range_check``): an activation beyond the split-f16 operand range raises
``AmpError`` (AMP_ERR_RANGE) -- re-run with ``_lib.set_precision("f32")``.  Not on the HIP path (``NotImplementedError``): the quantizer's
training mode, ``quantizer_type`` "vq" / "lfq", and the convolutional decoder (``use_vocos=False``)."""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.quantize import FactorizedVectorQuantize, ResidualVQ  # noqa: F401
from amphion_amd.models.codec.amphion_codec.vocos import Vocos, _check_input, _check_tensors
from amphion_amd.models.vocoders.gan.generator._engine import ConvParams
from amphion_amd.modules.hip_ops import HipConv1d


def WNConv1d(*args, **kwargs):
    return HipConv1d(*args, **kwargs)


def snake(x, alpha):
    """x + (alpha + 1e-9)^-1 sin^2(alpha x) over [B, C, ...] (codec.py:34-39) on the element-wise kernel"""
    x = _lib.require_device_tensor(x, "snake input")
    shape = x.shape
    x3 = x.reshape(shape[0], shape[1], -1)
    y = torch.empty_like(x3)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().amp_snake(_p(x3), x3.shape[0], x3.shape[1], x3.shape[2], _p(alpha.detach().reshape(-1).contiguous()), None, 0, _p(y),
                                        _lib.current_stream_ptr(x.device)))
    return y.reshape(shape)


class Snake1d(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.alpha = nn.Parameter(torch.ones(1, channels, 1))

    def forward(self, x):
        return snake(x, self.alpha)


def init_weights(m):
    """codec.py:51-57.  Under weight-norm the reference's draw lands on the derived ``weight`` attribute and leaves g / v as they are."""
    if isinstance(m, (nn.Conv1d, nn.Linear)) or (isinstance(m, ConvParams) and not m.has_weight_norm):
        nn.init.trunc_normal_(m.weight, std=0.02)
    if isinstance(m, (nn.Conv1d, nn.Linear, ConvParams)) and m.bias is not None:
        nn.init.constant_(m.bias, 0)


class ResidualUnit(nn.Module):
    """codec.py:60-76; ``block`` only holds the parameters under the reference's keys, ``forward`` is ``amp_codec_unit_forward``."""

    def __init__(self, dim: int = 16, dilation: int = 1):
        super().__init__()
        pad = ((7 - 1) * dilation) // 2
        self.dim, self.dilation = dim, dilation
        self.block = nn.Sequential(Snake1d(dim), WNConv1d(dim, dim, 7, dilation=dilation, padding=pad), Snake1d(dim), WNConv1d(dim, dim, 1))
        self._cache = HandleCache("amp_codec_unit_destroy")

    def _handle(self, device):
        return self._cache.get(param_sig(self.parameters(), str(device), _lib.get_precision()), self._build, device)

    def _build(self, device):
        a1, c1, a2, c2 = self.block
        t = [host_f32(a1.alpha).reshape(-1), host_f32(c1.folded_weight()), host_f32(c1.bias), host_f32(a2.alpha).reshape(-1),
             host_f32(c2.folded_weight()), host_f32(c2.bias)]
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_codec_unit_create(self.dim, self.dilation, *[_p(v) for v in t], ctypes.byref(h)))
        return h

    def fused(self, device):
        return bool(_lib.lib().amp_codec_unit_fused(self._handle(device)))

    def run(self, x, out=None):
        B, C, T = x.shape
        dev = x.device
        L = _lib.lib()
        h = self._handle(dev)
        if out is None:
            out = torch.empty_like(x)
        need = L.amp_codec_unit_workspace_bytes(h, B, T)
        ws = torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None
        _lib.check(L.amp_codec_unit_forward(h, _p(x), B, T, _p(out), _p(ws), need, _lib.current_stream_ptr(dev)))
        return out

    def forward(self, x):
        x = _check_input(x, self.dim, "ResidualUnit")
        _check_tensors(self, x.device, "ResidualUnit")
        with _lib.on_device(x.device):
            return self.run(x)


class _StridedConv(ConvParams):
    """WNConv1d(cin, cout, 2 * stride, stride, padding) under the reference's keys; ``forward(x, alpha)`` = conv(snake(x)) (``amp_sconv_forward``)"""

    def __init__(self, cin, cout, stride, padding):
        super().__init__(cin, cout, 2 * stride, stride=stride, padding=padding)
        self._cache = HandleCache("amp_sconv_destroy")

    def _handle(self, device):
        return self._cache.get(param_sig(self._parameters.values(), str(device), _lib.get_precision()), self._build, device)

    def _build(self, device):
        w, b = host_f32(self.folded_weight()), host_f32(self.bias)
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_sconv_create(self.cin, self.cout, self.stride, self.padding, _p(w), _p(b), ctypes.byref(h)))
        return h

    def forward(self, x, alpha=None):
        x = _check_input(x, self.cin, "strided conv")
        B, _, T = x.shape
        dev = x.device
        L = _lib.lib()
        with _lib.on_device(dev):
            h = self._handle(dev)
            Tout = L.amp_sconv_out_len(h, T)
            if Tout < 1:
                raise ValueError(f"strided conv: {T} input samples are fewer than the kernel (k = {self.k}, padding {self.padding}) covers")
            need = L.amp_sconv_workspace_bytes(h, B, T)
            ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
            out = torch.empty((B, self.cout, Tout), dtype=torch.float32, device=dev)
            a = None if alpha is None else alpha.detach().reshape(-1).contiguous()
            _lib.check(L.amp_sconv_forward(h, _p(x), B, T, _p(a), _p(ws), need, _p(out), _lib.current_stream_ptr(dev)))
        return out


class _TransposedConv(ConvParams):
    """WNConvTranspose1d(cin, cout, 2 * stride, stride, padding, output_padding) under the reference's keys (weight-norm over dim 0 = the INPUT
    channels: ``weight_g`` [cin, 1, 1], ``weight_v`` [cin, cout, 2 * stride]); ``forward(x, alpha)`` = conv_transpose(snake(x))
    (``amp_tconv_forward``)"""

    def __init__(self, cin, cout, stride, padding, output_padding=0):
        super().__init__(cin, cout, 2 * stride, transposed=True, stride=stride, padding=padding)
        self.output_padding = output_padding
        self._cache = HandleCache("amp_tconv_destroy")

    def _handle(self, device):
        return self._cache.get(param_sig(self._parameters.values(), str(device), _lib.get_precision()), self._build, device)

    def _build(self, device):
        w, b = host_f32(self.folded_weight()), host_f32(self.bias)
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_tconv_create(self.cin, self.cout, self.stride, self.padding, self.output_padding, _p(w), _p(b), ctypes.byref(h)))
        return h

    def fused(self, device):
        return bool(_lib.lib().amp_tconv_fused(self._handle(device)))

    def out_len(self, T):
        return (T - 1) * self.stride - 2 * self.padding + 2 * self.stride + self.output_padding

    def forward(self, x, alpha=None):
        x = _check_input(x, self.cin, "transposed conv")
        B, _, T = x.shape
        dev = x.device
        L = _lib.lib()
        with _lib.on_device(dev):
            h = self._handle(dev)
            Tout = L.amp_tconv_out_len(h, T)
            if Tout < 1:
                raise ValueError(f"transposed conv: {T} input samples give no output (k = {self.k}, stride {self.stride}, padding {self.padding})")
            need = L.amp_tconv_workspace_bytes(h, B, T)
            ws = torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None
            out = torch.empty((B, self.cout, Tout), dtype=torch.float32, device=dev)
            a = None if alpha is None else alpha.detach().reshape(-1).contiguous()
            _lib.check(L.amp_tconv_forward(h, _p(x), B, T, _p(a), _p(ws), need, _p(out), _lib.current_stream_ptr(dev)))
        return out


def _check_channels(x, channels, who):
    """the shape first (a host tensor of the wrong width is a ValueError), then the device"""
    if isinstance(x, torch.Tensor) and (x.dim() != 3 or x.shape[1] != channels):
        raise ValueError(f"{who}: expected a [B, {channels}, T] input, got {tuple(x.shape)}")
    return _check_input(x, channels, who)


class DecoderBlock(nn.Module):
    """codec.py:146-165: Snake1d -> WNConvTranspose1d(k = 2 s, stride s, padding s // 2 + s % 2, output_padding s % 2) -> 3 x ResidualUnit.
    ``output_padding=0`` is DualCodec's form of the same block (model_codec/dac_model.py:119-137)."""

    def __init__(self, input_dim: int = 16, output_dim: int = 8, stride: int = 1, output_padding=None):
        super().__init__()
        op = stride % 2 if output_padding is None else output_padding
        self.input_dim = input_dim
        self.block = nn.Sequential(Snake1d(input_dim), _TransposedConv(input_dim, output_dim, stride, stride // 2 + stride % 2, op),
                                   ResidualUnit(output_dim, dilation=1), ResidualUnit(output_dim, dilation=3), ResidualUnit(output_dim, dilation=9))

    def run(self, x):
        x = self.block[1](x, self.block[0].alpha)
        for unit in list(self.block)[2:]:
            x = unit.run(x)
        return x

    def forward(self, x):
        x = _check_channels(x, self.input_dim, "DecoderBlock")
        _check_tensors(self, x.device, "DecoderBlock")
        with _lib.on_device(x.device):
            y = self.run(x)
        _lib.range_check(x.device)
        return y


class EncoderBlock(nn.Module):
    def __init__(self, dim: int = 16, stride: int = 1):
        super().__init__()
        self.block = nn.Sequential(ResidualUnit(dim // 2, dilation=1), ResidualUnit(dim // 2, dilation=3), ResidualUnit(dim // 2, dilation=9),
                                   Snake1d(dim // 2), _StridedConv(dim // 2, dim, stride, math.ceil(stride / 2)))

    def run(self, x):
        for unit in list(self.block)[:3]:
            x = unit.run(x)
        return self.block[4](x, self.block[3].alpha)

    def forward(self, x):
        x = _check_input(x, self.block[0].dim, "EncoderBlock")
        _check_tensors(self, x.device, "EncoderBlock")
        with _lib.on_device(x.device):
            return self.run(x)


class CodecEncoder(nn.Module):
    def __init__(self, d_model: int = 64, up_ratios: list = [4, 5, 5, 6], out_channels: int = 256, use_tanh: bool = False, cfg=None):
        super().__init__()
        d_model = cfg.d_model if cfg is not None else d_model
        up_ratios = cfg.up_ratios if cfg is not None else up_ratios
        out_channels = cfg.out_channels if cfg is not None else out_channels
        use_tanh = cfg.use_tanh if cfg is not None else use_tanh
        block = [WNConv1d(1, d_model, 7, padding=3)]
        for stride in up_ratios:
            d_model *= 2
            block += [EncoderBlock(d_model, stride=stride)]
        block += [Snake1d(d_model), WNConv1d(d_model, out_channels, 3, padding=1, tanh=bool(use_tanh))]
        if use_tanh:
            block += [nn.Tanh()]           # holds the reference's module index; the tanh itself is the last conv's store
        self.block = nn.Sequential(*block)
        self.enc_dim = d_model
        self.n_blocks = len(up_ratios)
        self.reset_parameters()

    def forward(self, x):
        """x [B, 1, T] waveform -> latent [B, out_channels, T']"""
        x = _check_input(x, 1, "CodecEncoder")
        dev = x.device
        _check_tensors(self, dev, "CodecEncoder")
        with _lib.on_device(dev):
            h = self.block[0](x)
            for i in range(self.n_blocks):
                h = self.block[1 + i].run(h)
            h = self.block[2 + self.n_blocks](self.block[1 + self.n_blocks](h))
        _lib.range_check(dev)
        return h

    def reset_parameters(self):
        self.apply(init_weights)


class CodecDecoder(nn.Module):
    def __init__(self, in_channels: int = 256, upsample_initial_channel: int = 1536, up_ratios: list = [5, 5, 4, 2], num_quantizers: int = 8,
                 codebook_size: int = 1024, codebook_dim: int = 256, quantizer_type: str = "vq", quantizer_dropout: float = 0.5,
                 commitment: float = 0.25, codebook_loss_weight: float = 1.0, use_l2_normlize: bool = False, codebook_type: str = "euclidean",
                 kmeans_init: bool = False, kmeans_iters: int = 10, decay: float = 0.8, eps: float = 1e-5, threshold_ema_dead_code: int = 2,
                 weight_init: bool = False, use_vocos: bool = False, vocos_dim: int = 384, vocos_intermediate_dim: int = 1152,
                 vocos_num_layers: int = 8, n_fft: int = 800, hop_size: int = 200, padding: str = "same", cfg=None):
        super().__init__()

        def pick(name, default):
            return getattr(cfg, name) if cfg is not None and hasattr(cfg, name) else default

        in_channels = pick("in_channels", in_channels)
        num_quantizers = pick("num_quantizers", num_quantizers)
        codebook_size = pick("codebook_size", codebook_size)
        codebook_dim = pick("codebook_dim", codebook_dim)
        quantizer_type = pick("quantizer_type", quantizer_type)
        quantizer_dropout = pick("quantizer_dropout", quantizer_dropout)
        commitment = pick("commitment", commitment)
        codebook_loss_weight = pick("codebook_loss_weight", codebook_loss_weight)
        use_l2_normlize = pick("use_l2_normlize", use_l2_normlize)
        use_vocos = pick("use_vocos", use_vocos)
        vocos_dim = pick("vocos_dim", vocos_dim)
        vocos_intermediate_dim = pick("vocos_intermediate_dim", vocos_intermediate_dim)
        vocos_num_layers = pick("vocos_num_layers", vocos_num_layers)
        n_fft = pick("n_fft", n_fft)
        hop_size = pick("hop_size", hop_size)
        padding = pick("padding", padding)

        if quantizer_type in ("vq", "lfq"):
            raise NotImplementedError(f"CodecDecoder quantizer_type={quantizer_type!r} is not on the HIP path: the shipped codec configs use 'fvq'")
        if quantizer_type != "fvq":
            raise ValueError(f"Unknown quantizer type {quantizer_type}")
        if not use_vocos:
            raise NotImplementedError("CodecDecoder with use_vocos=False (the convolutional decoder) is not on the HIP path: no shipped config "
                                      "uses it")
        self.quantizer = ResidualVQ(input_dim=in_channels, num_quantizers=num_quantizers, codebook_size=codebook_size, codebook_dim=codebook_dim,
                                    quantizer_type=quantizer_type, quantizer_dropout=quantizer_dropout, commitment=commitment,
                                    codebook_loss_weight=codebook_loss_weight, use_l2_normlize=use_l2_normlize)
        self.model = Vocos(input_channels=in_channels, dim=vocos_dim, intermediate_dim=vocos_intermediate_dim, num_layers=vocos_num_layers,
                           adanorm_num_embeddings=None, n_fft=n_fft, hop_size=hop_size, padding=padding)
        self.reset_parameters()

    def forward(self, x=None, vq=False, eval_vq=False, n_quantizers=None):
        """vq=True: x is the encoder output, returns the quantizer's 5-tuple; else x is the quantized latent, returns the waveform"""
        if vq is True:
            if eval_vq:
                self.quantizer.eval()
            return self.quantizer(x, n_quantizers=n_quantizers)
        return self.model(x)

    def quantize(self, x, n_quantizers=None):
        self.quantizer.eval()
        quantized_out, vq, _ = self.quantizer.encode(x, n_quantizers=n_quantizers)
        return quantized_out, vq

    def vq2emb(self, vq, n_quantizers=None):
        return self.quantizer.vq2emb(vq, n_quantizers=n_quantizers)

    def decode(self, x):
        return self.model(x)

    def latent2dist(self, x, n_quantizers=None):
        return self.quantizer.latent2dist(x, n_quantizers=n_quantizers)

    def reset_parameters(self):
        self.apply(init_weights)
