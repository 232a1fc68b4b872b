"""VevoRepCodec drop-in (models/codec/vevo/vevo_repcodec.py:19-592), Vevo's 32-entry content tokenizer over HuBERT features, in eval mode on
the gfx950 kernels.  Same classes, constructor arguments, submodule names and ``state_dict`` keys; every module works on its own, as
vevo_utils calls them (``encoder(x)``, ``projector(x)``, ``quantizer.codebook.forward_index(z.transpose(2, 1))``):

    Conv1d (.conv)            stride 1, 'same' padding: the implicit-GEMM conv kernels (HipConv1d)
    ResidualUnit              amp_elu_pad (zero pads: the plain ELU) -> conv (k = 3) -> amp_elu_pad in place -> amp_pw_forward with the
                              residual epilogue (gamma = 1, no bias)
    VectorQuantize (.embed)   [dim, K], transposed once when the amp_evq handle is made; all levels of ResidualVQ are ONE amp_evq_encode
    lookup / decode           amp_evq_decode + amp_evq_check: an index outside its level's K entries raises ``AmpError``

The two scalars of ``forward`` (vqloss, perplexity) are torch ops on the kernel's codes and rows.  Only stride 1 is built -- all the shipped
hubert_large_l18_c32.yaml uses; other strides, activations other than ELU and training mode raise ``NotImplementedError``.  Covered by
amp_evq: dim <= 1024, codebook_size <= 4096."""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32_array, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.vocos import _check_input, _check_tensors, _PwHandle, pw_forward
from amphion_amd.models.codec.kmeans.repcodec_model import no_training
from amphion_amd.modules.hip_ops import HipConv1d


class _Stage(nn.Module):
    """a module of the codec that runs alone: ``forward`` checks its [B, C, T] input, ``run`` is the launches"""

    def forward(self, x):
        who = type(self).__name__
        no_training(self, who)
        x = _check_input(x, self.in_channels, who)
        _check_tensors(self, x.device, who)
        with _lib.on_device(x.device):
            y = self.run(x)
        _lib.range_check(x.device)
        return y


def elu(x, alpha, out=None):
    """nn.ELU on [B, C, T] (``amp_elu_pad`` with zero pads); ``out`` may be ``x``"""
    out = torch.empty_like(x) if out is None else out
    B, C, T = x.shape
    _lib.check(_lib.lib().amp_elu_pad(_p(x), B, C, T, 0, 0, 1, float(alpha), _p(out), _lib.current_stream_ptr(x.device)))
    return out


# ---- the quantizer -----------------------------------------------------------------------------------------------------------------
class _EvqHandle:
    """the device copy of the levels' codebooks for ``amp_evq_*``: each ``embed`` [dim, K] transposed once, rebuilt when a buffer or the device
    changes"""

    def __init__(self):
        self._cache = HandleCache("amp_evq_destroy")

    def get(self, layers, device):
        return self._cache.get(param_sig([q.embed for q in layers], str(device), len(layers)), self._build, layers, device)

    def _build(self, layers, device):
        D, K = layers[0].embed.shape
        if any(tuple(q.embed.shape) != (D, K) for q in layers):
            raise NotImplementedError("ResidualVQ: levels whose codebooks differ in shape are not on the HIP path")
        arr = host_f32_array([q.embed.t() for q in layers])      # [K, dim] rows
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_evq_create(D, K, len(layers), arr, ctypes.byref(h)))
        return h


def _time_major(x, dim, who):
    """[..., dim] as the quantizer takes it -> (checked [B, dim, T] copy, the leading shape)"""
    if not isinstance(x, torch.Tensor) or x.dim() < 2 or x.shape[-1] != dim:
        raise ValueError(f"{who}: expected a [..., {dim}] input, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
    lead = tuple(x.shape[:-1])
    x3 = x.reshape(1, -1, dim) if x.dim() != 3 else x
    return _check_input(x3.transpose(1, 2), dim, who), lead


def _evq_encode(handle, layers, x, who, want_all=False):
    """x [..., dim] -> (codes [N, ...], the sum of the levels' rows [..., dim], every level's rows [N, ..., dim] or None)"""
    for q in layers:
        no_training(q, who)
    dim = layers[0].dim
    z, lead = _time_major(x, dim, who)
    B, _, T = z.shape
    dev = z.device
    for q in layers:
        _check_tensors(q, dev, who)
    n = len(layers)
    h = handle.get(layers, dev)
    codes = torch.empty((n, B, T), dtype=torch.int64, device=dev)
    zq = torch.empty((B, dim, T), dtype=torch.float32, device=dev)
    allq = torch.empty((n, B, dim, T), dtype=torch.float32, device=dev) if want_all else None
    with _lib.on_device(dev):
        _lib.check(_lib.lib().amp_evq_encode(h, _p(z), B, T, 0, n, _p(codes), _p(zq), _p(allq), _lib.current_stream_ptr(dev)))
    return (codes.reshape(n, *lead), zq.transpose(1, 2).reshape(*lead, dim),
            allq.transpose(2, 3).reshape(n, *lead, dim) if want_all else None)


def _perplexity(codes, n_embed):
    avg_probs = torch.bincount(codes.flatten(), minlength=n_embed).float() / codes.numel()
    return torch.exp(-torch.sum(avg_probs * torch.log(avg_probs + 1e-10)))


class VectorQuantize(nn.Module):
    """One level: the nearest column of ``embed`` [dim, n_embed] in the Euclidean distance (the EMA codebook update is training only)"""

    def __init__(self, dim: int, codebook_size: int, decay=0.8, commitment=1.0, eps=1e-5, n_embed=None):
        super().__init__()
        n_embed = codebook_size if n_embed is None else n_embed
        self.dim = dim
        self.n_embed = n_embed
        self.decay = decay
        self.eps = eps
        self.commitment = commitment
        embed = torch.randn(dim, n_embed)
        self.register_buffer("embed", embed)
        self.register_buffer("cluster_size", torch.zeros(n_embed))
        self.register_buffer("embed_avg", embed.clone())
        self._handle = _EvqHandle()

    @property
    def codebook(self):
        return self.embed.transpose(0, 1)

    def forward(self, input):
        """-> (quantize like input, loss, perplexity)"""
        codes, quantize, _ = _evq_encode(self._handle, [self], input, "VectorQuantize")
        loss = F.mse_loss(quantize, input) * self.commitment
        return quantize, loss, _perplexity(codes, self.n_embed)

    def forward_index(self, input):
        """-> (quantize like input, embed_ind input.shape[:-1])"""
        codes, quantize, _ = _evq_encode(self._handle, [self], input, "VectorQuantize")
        return quantize, codes[0]


class ResidualVQ(nn.Module):
    """``num_quantizers`` VectorQuantize levels, each quantizing what the levels before it left"""

    def __init__(self, *, num_quantizers, **kwargs):
        super().__init__()
        self.layers = nn.ModuleList([VectorQuantize(**kwargs) for _ in range(num_quantizers)])
        self._handle = _EvqHandle()

    def forward(self, x):
        """x [B, T, C] -> (quantized_out [B, T, C], all_losses [N], all_perplexities [N])"""
        layers = list(self.layers)
        codes, zq, allq = _evq_encode(self._handle, layers, x, "ResidualVQ", want_all=True)
        residual, losses, perps = x, [], []
        for i, layer in enumerate(layers):
            losses.append(F.mse_loss(allq[i], residual) * layer.commitment)
            perps.append(_perplexity(codes[i], layer.n_embed))
            residual = residual - allq[i]
        return zq, torch.stack(losses), torch.stack(perps)

    def forward_index(self, x, flatten_idx=False):
        """-> (quantized_out like x, all_indices [N, B, T]); flatten_idx: level i's indices moved on by i * codebook_size (after ``initial``)"""
        codes, zq, _ = _evq_encode(self._handle, list(self.layers), x, "ResidualVQ")
        if flatten_idx:
            codes = codes + self.codebook_size * torch.arange(codes.shape[0], device=codes.device).reshape(-1, *([1] * (codes.dim() - 1)))
        return zq, codes

    def initial(self):
        """``codebook`` [N K, dim]: every level's rows one under the other, and ``codebook_size`` = K, for the flattened indices"""
        rows = torch.stack([layer.codebook for layer in self.layers])
        self.codebook_size = rows.shape[1]
        self.codebook = rows.reshape(-1, rows.shape[-1])

    def lookup(self, indices):
        """flattened indices [N, ...] (``forward_index(flatten_idx=True)``) -> [1, ..., C].  Row i must hold level i's indices, i.e. lie in
        [i K, (i + 1) K): anything else raises ``AmpError`` (the reference would read another level's row)."""
        layers = list(self.layers)
        if not hasattr(self, "codebook_size"):
            raise RuntimeError("ResidualVQ.lookup: call initial() first")
        if not isinstance(indices, torch.Tensor) or indices.dim() < 2 or indices.shape[0] != len(layers) or indices.numel() < 1:
            raise ValueError(f"ResidualVQ.lookup: expected indices [{len(layers)}, ...]")
        if indices.dtype.is_floating_point or indices.dtype == torch.bool:
            raise TypeError(f"ResidualVQ.lookup: the indices must be integers, got {indices.dtype}")
        if not indices.is_cuda:
            raise RuntimeError("ResidualVQ.lookup: the indices must be a tensor on a ROCm device (there is no CPU fallback)")
        for q in layers:
            no_training(q, "ResidualVQ")
            _check_tensors(q, indices.device, "ResidualVQ")
        n, rest = indices.shape[0], tuple(indices.shape[1:])
        dev = indices.device
        level0 = self.codebook_size * torch.arange(n, device=dev).reshape(n, 1, 1)
        codes = (indices.to(torch.int64).reshape(n, 1, -1) - level0).contiguous()
        out = torch.empty((1, layers[0].dim, codes.shape[2]), dtype=torch.float32, device=dev)
        h = self._handle.get(layers, dev)
        with _lib.on_device(dev):
            s = _lib.current_stream_ptr(dev)
            _lib.check(_lib.lib().amp_evq_decode(h, _p(codes), n, 0, 1, codes.shape[2], _p(out), s))
            _lib.check(_lib.lib().amp_evq_check(h, s))
        return out.transpose(1, 2).reshape(1, *rest, layers[0].dim)


class Quantizer(nn.Module):
    def __init__(self, code_dim: int, codebook_num: int, codebook_size: int):
        super().__init__()
        self.codebook = ResidualVQ(dim=code_dim, num_quantizers=codebook_num, codebook_size=codebook_size)

    def initial(self):
        self.codebook.initial()

    def forward(self, z):
        """z [B, C, T] -> (zq [B, C, T], vqloss [N], perplexity [N])"""
        zq, vqloss, perplexity = self.codebook(z.transpose(2, 1))
        return zq.transpose(2, 1), vqloss, perplexity

    def inference(self, z):
        """z [B, C, T] -> (zq [B, C, T], indices [N, B, T])"""
        zq, indices = self.codebook.forward_index(z.transpose(2, 1))
        return zq.transpose(2, 1), indices

    def encode(self, z):
        """z [B, C, T] -> (zq [B, T, C] -- time-major, as the reference leaves it -- flattened indices [N, B, T])"""
        return self.codebook.forward_index(z.transpose(2, 1), flatten_idx=True)

    def decode(self, indices):
        return self.codebook.lookup(indices)


# ---- the conv stacks ---------------------------------------------------------------------------------------------------------------
class Conv1d1x1(nn.Conv1d):
    """1x1 Conv1d, run as the pointwise GEMM (``amp_pw_forward``)"""

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__(in_channels, out_channels, kernel_size=1, bias=bias)
        self._pw = _PwHandle()

    @property
    def in_features(self):
        return self.in_channels

    @property
    def out_features(self):
        return self.out_channels

    def forward(self, x):
        x = _check_input(x, self.in_channels, "Conv1d1x1")
        with _lib.on_device(x.device):
            return pw_forward(self._pw, self, x, _lib.AMP_PW_BIAS, x.new_empty((x.shape[0], self.out_channels, x.shape[2])))


class Conv1d(_Stage):
    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int = 1, padding: int = -1, dilation: int = 1,
                 groups: int = 1, bias: bool = True):
        super().__init__()
        if stride != 1 or groups != 1:
            raise NotImplementedError("VevoRepCodec Conv1d: only stride 1, groups 1 are on the HIP path (all that hubert_large_l18_c32.yaml uses)")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = kernel_size
        if padding < 0:
            padding = (kernel_size - 1) // 2 * dilation
        self.dilation = dilation
        self.conv = HipConv1d(in_channels, out_channels, kernel_size, padding=padding, dilation=dilation, weight_norm=False, bias=bias)

    def run(self, x):
        return self.conv(x)


class ConvTranspose1d(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError("VevoRepCodec ConvTranspose1d: up-sampling decoder blocks (stride > 1) are not on the HIP path")


class ResidualUnit(_Stage):
    def __init__(self, in_channels: int, out_channels: int, kernel_size=3, dilation=1, bias=False, nonlinear_activation="ELU",
                 nonlinear_activation_params={}):
        super().__init__()
        if nonlinear_activation != "ELU" or in_channels != out_channels:
            raise NotImplementedError("VevoRepCodec ResidualUnit: only ELU and in_channels == out_channels are on the HIP path")
        self.in_channels = in_channels
        self.activation = getattr(nn, nonlinear_activation)(**nonlinear_activation_params)
        self.conv1 = Conv1d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=1, dilation=dilation, bias=bias)
        self.conv2 = Conv1d1x1(out_channels, out_channels, bias)
        self._ones = {}

    def run(self, x):
        dev = x.device
        ones = self._ones.get(str(dev))
        if ones is None:
            ones = self._ones[str(dev)] = torch.ones(self.conv2.out_channels, device=dev)
        alpha = self.activation.alpha
        y = self.conv1.run(elu(x, alpha))
        elu(y, alpha, out=y)
        return pw_forward(self.conv2._pw, self.conv2, y, _lib.AMP_PW_SCALE_RES, torch.empty_like(x), gamma=ones, res=x)


class Projector(_Stage):
    def __init__(self, input_channels: int, code_dim: int, kernel_size=3, stride=1, bias=False):
        super().__init__()
        self.in_channels = input_channels
        self.project = Conv1d(input_channels, code_dim, kernel_size=kernel_size, stride=stride, bias=bias)

    def run(self, x):
        return self.project.run(x)


class EncoderBlock(_Stage):
    def __init__(self, in_channels: int, out_channels: int, stride: int, dilations=(1, 1), unit_kernel_size=3, bias=True):
        super().__init__()
        self.in_channels = in_channels
        self.res_units = nn.ModuleList([ResidualUnit(in_channels, in_channels, kernel_size=unit_kernel_size, dilation=d) for d in dilations])
        self.num_res = len(self.res_units)
        # k = 2 stride for a strided block (refused by Conv1d here), k = 3 at stride 1
        self.conv = Conv1d(in_channels, out_channels, 3 if stride == 1 else 2 * stride, stride=stride, bias=bias)

    def run(self, x):
        for idx in range(self.num_res):
            x = self.res_units[idx].run(x)
        return self.conv.run(x)


class Encoder(_Stage):
    def __init__(self, input_channels: int, encode_channels: int, channel_ratios=(1, 1), strides=(1, 1), kernel_size=3, bias=True,
                 block_dilations=(1, 1), unit_kernel_size=3):
        super().__init__()
        assert len(channel_ratios) == len(strides)
        self.in_channels = input_channels
        self.conv = Conv1d(input_channels, encode_channels, kernel_size, stride=1, bias=False)
        widths = [encode_channels] + [int(encode_channels * r) for r in channel_ratios]          # a ratio may be fractional
        self.conv_blocks = nn.ModuleList([EncoderBlock(cin, cout, stride, dilations=block_dilations, unit_kernel_size=unit_kernel_size, bias=bias)
                                          for cin, cout, stride in zip(widths[:-1], widths[1:], strides)])
        self.num_blocks = len(self.conv_blocks)
        self.out_channels = widths[-1]

    def run(self, x):
        x = self.conv.run(x)
        for i in range(self.num_blocks):
            x = self.conv_blocks[i].run(x)
        return x


class DecoderBlock(_Stage):
    """conv (k = 3 at stride 1; the transposed conv of a strided block is refused here), then the residual units"""

    def __init__(self, in_channels: int, out_channels: int, stride: int, dilations=(1, 1), unit_kernel_size=3, bias=True):
        super().__init__()
        self.in_channels = in_channels
        if stride == 1:
            self.conv = Conv1d(in_channels, out_channels, 3, stride=1, bias=bias)
        else:
            self.conv = ConvTranspose1d(in_channels, out_channels, 2 * stride, stride=stride, bias=bias)
        self.res_units = nn.ModuleList([ResidualUnit(out_channels, out_channels, kernel_size=unit_kernel_size, dilation=d) for d in dilations])
        self.num_res = len(self.res_units)

    def run(self, x):
        x = self.conv.run(x)
        for idx in range(self.num_res):
            x = self.res_units[idx].run(x)
        return x


class Decoder(_Stage):
    def __init__(self, code_dim: int, output_channels: int, decode_channels: int, channel_ratios=(1, 1), strides=(1, 1), kernel_size=3,
                 bias=True, block_dilations=(1, 1), unit_kernel_size=3):
        super().__init__()
        assert len(channel_ratios) == len(strides)
        self.in_channels = code_dim
        # block i runs ratio i -> ratio i + 1 of decode_channels, the last one to decode_channels itself
        widths = [int(decode_channels * r) for r in channel_ratios] + [decode_channels]
        self.conv1 = Conv1d(code_dim, widths[0], kernel_size, stride=1, bias=False)
        self.conv_blocks = nn.ModuleList([DecoderBlock(cin, cout, stride, dilations=block_dilations, unit_kernel_size=unit_kernel_size, bias=bias)
                                          for cin, cout, stride in zip(widths[:-1], widths[1:], strides)])
        self.num_blocks = len(self.conv_blocks)
        self.conv2 = Conv1d(widths[-1], output_channels, kernel_size, 1, bias=False)

    def run(self, z):
        x = self.conv1.run(z)
        for i in range(self.num_blocks):
            x = self.conv_blocks[i].run(x)
        return self.conv2.run(x)


class VevoRepCodec(nn.Module):
    def __init__(self, input_channels=768, output_channels=768, encode_channels=768, decode_channels=768, code_dim=768, codebook_num=1,
                 codebook_size=1024, bias=True, enc_ratios=(1, 1), dec_ratios=(1, 1), enc_strides=(1, 1), dec_strides=(1, 1), enc_kernel_size=3,
                 dec_kernel_size=3, enc_block_dilations=(1, 1), enc_block_kernel_size=3, dec_block_dilations=(1, 1), dec_block_kernel_size=3):
        super().__init__()
        self.input_channels = input_channels
        self.encoder = Encoder(input_channels=input_channels, encode_channels=encode_channels, channel_ratios=enc_ratios, strides=enc_strides,
                               kernel_size=enc_kernel_size, bias=bias, block_dilations=enc_block_dilations, unit_kernel_size=enc_block_kernel_size)
        self.decoder = Decoder(code_dim=code_dim, output_channels=output_channels, decode_channels=decode_channels, channel_ratios=dec_ratios,
                               strides=dec_strides, kernel_size=dec_kernel_size, bias=bias, block_dilations=dec_block_dilations,
                               unit_kernel_size=dec_block_kernel_size)
        self.projector = Projector(input_channels=self.encoder.out_channels, code_dim=code_dim, kernel_size=3, stride=1, bias=False)
        self.quantizer = Quantizer(code_dim=code_dim, codebook_num=codebook_num, codebook_size=codebook_size)

    def forward(self, x):
        """x [B, input_channels, T] -> (y [B, output_channels, T], zq [B, code_dim, T], z [B, code_dim, T], vqloss [N], perplexity [N])"""
        no_training(self, "VevoRepCodec")
        x = _check_input(x, self.input_channels, "VevoRepCodec")
        _check_tensors(self, x.device, "VevoRepCodec")
        with _lib.on_device(x.device):
            z = self.projector.run(self.encoder.run(x))
        zq, vqloss, perplexity = self.quantizer(z)
        with _lib.on_device(x.device):
            y = self.decoder.run(zq.contiguous())
        _lib.range_check(x.device)
        return y, zq, z, vqloss, perplexity
