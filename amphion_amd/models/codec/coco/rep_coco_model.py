"""Coco drop-ins (models/codec/coco/rep_coco_model.py:33-411), VevoSing's content / style tokenizers, in eval mode on the gfx950 kernels.
Built from ``cfg`` (any object with the reference's attributes); same submodule names and ``state_dict`` keys:

    whisper_input_layer, chromagram_input_layer     nn.Linear on amp_pw_forward; their sum is the second call's residual epilogue (gamma = 1)
    downsample_layers (.0, .2, ..)                  Conv1d(k = 3, stride 2, padding 1) -> GELU: amp_dsconv_forward with the GELU epilogue
    encoder / decoder                               nn.Sequential(VocosBackbone, nn.Linear) (kmeans.repcodec_model.BackboneLinear)
    quantizer                                       the ResidualVQ of amphion_codec.quantize (amp_fvq_*)
    upsample_layers (.0, .2, ..)                    ConvTranspose1d(k = 4, stride 2, padding 1) on the conv kernels, then amp_gelu
    *_output_layer                                  nn.Linear on amp_pw_forward, after the crop / last-frame padding to T

``forward`` and ``quantize`` keep the reference's signatures and return shapes.  Training mode raises ``NotImplementedError``; every public
forward ends with ``_lib.range_check``."""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.quantize import ResidualVQ
from amphion_amd.models.codec.amphion_codec.vocos import _check_input, _check_tensors, _PwHandle, pw_forward
from amphion_amd.models.codec.kmeans.repcodec_model import BackboneLinear, init_weights, no_training, time_major_input
from amphion_amd.modules.hip_ops import HipConv1d


def gelu_(x):
    """exact-erf GELU in place (``amp_gelu``)"""
    dev = x.device
    with _lib.on_device(dev):
        _lib.check(_lib.lib().amp_gelu(_p(x), x.numel(), _p(x), _lib.current_stream_ptr(dev)))
    return x


class DownsampleConv1d(nn.Conv1d):
    """Conv1d(C, C, kernel_size = 3, stride = 2, padding = 1) on ``amp_dsconv_forward``; ``gelu`` folds the nn.GELU behind it into the launch.
    The handle is rebuilt when the parameters, the device or the precision change."""

    def __init__(self, cin, cout):
        super().__init__(cin, cout, kernel_size=3, stride=2, padding=1)
        self._cache = HandleCache("amp_dsconv_destroy")

    def _ensure(self, device):
        return self._cache.get(param_sig((self.weight, self.bias), str(device), _lib.get_precision()), self._build, device)

    def _build(self, device):
        w, b = host_f32(self.weight), host_f32(self.bias)
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_dsconv_create(self.in_channels, self.out_channels, _p(w), _p(b), ctypes.byref(h)))
        return h

    def forward(self, x, gelu=False):
        x = _check_input(x, self.in_channels, "DownsampleConv1d")
        dev = x.device
        B, _, T = x.shape
        L = _lib.lib()
        h = self._ensure(dev)
        with _lib.on_device(dev):
            out = torch.empty((B, self.out_channels, L.amp_dsconv_out_len(h, T)), dtype=torch.float32, device=dev)
            need = L.amp_dsconv_workspace_bytes(h, B, T)
            ws = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=dev) if need else None
            _lib.check(L.amp_dsconv_forward(h, _p(x), B, T, int(bool(gelu)), _p(ws), need, _p(out), _lib.current_stream_ptr(dev)))
        return out


class _ConvGeluStack(nn.Sequential):
    """[conv, nn.GELU(), conv, nn.GELU(), ..] under the reference's indices; the GELU modules hold no state and are run by the convs' side"""

    def forward(self, x):
        for conv in list(self)[0::2]:
            x = self.step(conv, x)
        return x


class DownsampleLayers(_ConvGeluStack):
    def step(self, conv, x):
        return conv(x, gelu=True)


class UpsampleLayers(_ConvGeluStack):
    def step(self, conv, x):
        return gelu_(conv(x))


class CocoContentStyle(nn.Module):
    def __init__(self, codebook_size=8192, hidden_size=1024, codebook_dim=8, num_quantizers=1, quantizer_type="fvq", use_whisper=True,
                 use_chromagram=True, construct_only_for_quantizer=False, cfg=None):
        super().__init__()
        assert cfg is not None
        self.cfg = cfg

        codebook_size = getattr(cfg, "codebook_size", codebook_size)
        hidden_size = getattr(cfg, "hidden_size", hidden_size)
        codebook_dim = getattr(cfg, "codebook_dim", codebook_dim)
        num_quantizers = getattr(cfg, "num_quantizers", num_quantizers)
        quantizer_type = getattr(cfg, "quantizer_type", quantizer_type)

        self.codebook_size = codebook_size
        self.codebook_dim = codebook_dim
        self.hidden_size = hidden_size
        self.num_quantizers = num_quantizers
        self.quantizer_type = quantizer_type
        self.use_whisper, self.use_chromagram = bool(use_whisper), bool(use_chromagram)
        if not (self.use_whisper or self.use_chromagram):
            raise ValueError("Coco: at least one of use_whisper / use_chromagram")

        if use_whisper:
            self.whisper_input_layer = nn.Linear(self.cfg.whisper_dim, hidden_size)
        if use_chromagram:
            self.chromagram_input_layer = nn.Linear(self.cfg.chromagram_dim, hidden_size)

        downsample_rate = getattr(cfg, "downsample_rate", 1)
        if downsample_rate > 1:
            self.do_downsample = True
            assert np.log2(downsample_rate).is_integer()
            down_layers, up_layers = [], []
            for _ in range(int(np.log2(downsample_rate))):
                down_layers.extend([DownsampleConv1d(hidden_size, hidden_size), nn.GELU()])
                up_layers.extend([HipConv1d(hidden_size, hidden_size, 4, transposed=True, stride=2, padding=1, weight_norm=False), nn.GELU()])
            self.downsample_layers = DownsampleLayers(*down_layers)
            self.upsample_layers = UpsampleLayers(*up_layers)
        else:
            self.do_downsample = False

        enc = self.cfg.encoder
        self.encoder = BackboneLinear(self.hidden_size, enc.vocos_dim, enc.vocos_intermediate_dim, enc.vocos_num_layers, self.hidden_size)
        self.quantizer = ResidualVQ(input_dim=hidden_size, num_quantizers=num_quantizers, codebook_size=codebook_size, codebook_dim=codebook_dim,
                                    quantizer_type=quantizer_type, quantizer_dropout=0.0, commitment=0.15, codebook_loss_weight=1.0,
                                    use_l2_normlize=True)

        self.has_decoder = not construct_only_for_quantizer
        if self.has_decoder:
            dec = self.cfg.decoder
            self.decoder = BackboneLinear(self.hidden_size, dec.vocos_dim, dec.vocos_intermediate_dim, dec.vocos_num_layers, self.hidden_size)
            if use_whisper:
                self.whisper_output_layer = nn.Linear(self.hidden_size, self.cfg.whisper_dim)
            if use_chromagram:
                self.chromagram_output_layer = nn.Linear(self.hidden_size, self.cfg.chromagram_dim)

        self._pw = {name: _PwHandle() for name in ("whisper_in", "chroma_in", "whisper_out", "chroma_out")}
        self._ones = {}
        self.reset_parameters()

    # ---- the two halves, channel-first --------------------------------------------------------------------------------------------
    def input_projection(self, *feats):
        """feats: the time-major inputs of the layers this model has, whisper first -> their projections' sum [B, hidden, T], channel-first"""
        who = type(self).__name__
        no_training(self, who)
        if len(feats) != int(self.use_whisper) + int(self.use_chromagram):
            raise ValueError(f"{who}: expected {int(self.use_whisper) + int(self.use_chromagram)} input tensors, got {len(feats)}")
        layers = [(self.whisper_input_layer, "whisper_in")] if self.use_whisper else []
        layers += [(self.chromagram_input_layer, "chroma_in")] if self.use_chromagram else []
        xs = [time_major_input(f, lin.in_features, who) for f, (lin, _) in zip(feats, layers)]
        dev = xs[0].device
        B, _, T = xs[0].shape
        if any(x.device != dev or x.shape[0] != B or x.shape[2] != T for x in xs):
            raise ValueError(f"{who}: the inputs must share their device, batch and length")
        _check_tensors(self, dev, who)
        with _lib.on_device(dev):
            x = torch.empty((B, self.hidden_size, T), dtype=torch.float32, device=dev)
            pw_forward(self._pw[layers[0][1]], layers[0][0], xs[0], _lib.AMP_PW_BIAS, x)
            if len(layers) == 2:
                ones = self._ones.get(str(dev))
                if ones is None:
                    ones = self._ones[str(dev)] = torch.ones(self.hidden_size, device=dev)
                pw_forward(self._pw[layers[1][1]], layers[1][0], xs[1], _lib.AMP_PW_SCALE_RES, x, gamma=ones, res=x)
        return x

    def _encode(self, feats):
        """-> (T, quantized_out [B, D, T'], all_indices [N, B, T'])"""
        x = self.input_projection(*feats)
        T = x.shape[2]
        with _lib.on_device(x.device):
            if self.do_downsample:
                x = self.downsample_layers(x)
            z = self.encoder.forward_cf(x)
            zq, codes, _ = self.quantizer.encode(z)
        return T, zq, codes

    def _for_quantizer(self, zq, codes):
        _lib.range_check(zq.device)
        return (codes.squeeze(0) if codes.shape[0] == 1 else codes), zq.transpose(1, 2)

    def _decode(self, T, zq):
        """-> the outputs of the layers this model has, whisper first, each [B, T, dim]"""
        if not self.has_decoder:
            raise RuntimeError(f"{type(self).__name__}: built with construct_only_for_quantizer, there is no decoder")
        dev = zq.device
        with _lib.on_device(dev):
            x = self.decoder.forward_cf(zq)
            if self.do_downsample:
                x = self.upsample_layers(x)
            # the output length is the input's: crop, or repeat the last frame
            if x.shape[2] >= T:
                x = x[:, :, :T].contiguous()
            else:
                x = torch.cat([x, x[:, :, -1:].expand(-1, -1, T - x.shape[2])], dim=2).contiguous()
            outs = []
            for on, lin, key in ((self.use_whisper, "whisper_output_layer", "whisper_out"), (self.use_chromagram, "chromagram_output_layer", "chroma_out")):
                if on:
                    lin = getattr(self, lin)
                    y = torch.empty((x.shape[0], lin.out_features, T), dtype=torch.float32, device=dev)
                    outs.append(pw_forward(self._pw[key], lin, x, _lib.AMP_PW_BIAS, y).transpose(1, 2))
        _lib.range_check(dev)
        return outs

    def _forward(self, feats, return_for_quantizer):
        T, zq, codes = self._encode(feats)
        if return_for_quantizer:
            return self._for_quantizer(zq, codes)
        return (*self._decode(T, zq), torch.zeros((), device=zq.device), codes)

    # ---- the reference's interface ------------------------------------------------------------------------------------------------
    def forward(self, whisper_feats, chromagram_feats, return_for_quantizer=False):
        """whisper_feats [B, T, whisper_dim], chromagram_feats [B, T, chromagram_dim] -> (whisper_rec, chromagram_rec, codebook_loss = 0,
        all_indices [N, B, T']), or quantize()'s pair"""
        return self._forward((whisper_feats, chromagram_feats), return_for_quantizer)

    def quantize(self, whisper_feats, chromagram_feats):
        """-> (all_indices [N, B, T'] or [B, T'] when num_quantizers == 1, quantized_out [B, T', D])"""
        return self.forward(whisper_feats, chromagram_feats, return_for_quantizer=True)

    def reset_parameters(self):
        self.apply(init_weights)


class CocoContent(CocoContentStyle):
    def __init__(self, cfg, use_whisper=True, use_chromagram=False, construct_only_for_quantizer=False):
        super().__init__(cfg=cfg, use_whisper=use_whisper, use_chromagram=use_chromagram, construct_only_for_quantizer=construct_only_for_quantizer)

    def forward(self, whisper_feats, return_for_quantizer=False):
        """-> (whisper_rec [B, T, whisper_dim], codebook_loss = 0, all_indices [N, B, T']), or quantize()'s pair"""
        return self._forward((whisper_feats,), return_for_quantizer)

    def quantize(self, whisper_feats):
        return self.forward(whisper_feats, return_for_quantizer=True)


class CocoStyle(CocoContentStyle):
    def __init__(self, cfg, use_whisper=False, use_chromagram=True, construct_only_for_quantizer=False):
        super().__init__(cfg=cfg, use_whisper=use_whisper, use_chromagram=use_chromagram, construct_only_for_quantizer=construct_only_for_quantizer)

    def forward(self, chromagram_feats, return_for_quantizer=False):
        """-> (chromagram_rec [B, T, chromagram_dim], codebook_loss = 0, all_indices [N, B, T']), or quantize()'s pair"""
        return self._forward((chromagram_feats,), return_for_quantizer)

    def quantize(self, chromagram_feats):
        return self.forward(chromagram_feats, return_for_quantizer=True)
