"""RepCodec drop-in (models/codec/kmeans/repcodec_model.py:34-199), the semantic tokenizer of MaskGCT, Metis and Vevo, in eval mode on the
gfx950 kernels.  Same constructor (keyword arguments or ``cfg``), submodule names and ``state_dict`` keys:

    encoder / decoder     nn.Sequential(VocosBackbone, nn.Linear): the backbone of amphion_codec.vocos, the Linear on amp_pw_forward
    quantizer             the ResidualVQ of amphion_codec.quantize (amp_fvq_*)
    down / up             plain parameters when downsample_scale > 1; never run, as in the reference (its down-sampling is commented out)

``quantize(x [B, T, H]) -> (codes [B, T] when num_quantizers == 1 else [N, B, T], quantized [B, T, H])``
``forward(x [B, T, H]) -> (x_rec [B, T, H], codebook_loss = 0, all_indices [N, B, T])``
Inputs arrive time-major; the transposition to [B, C, T] is a torch copy.  Training mode raises ``NotImplementedError``; every public forward
ends with ``_lib.range_check``."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.codec.amphion_codec.quantize import ResidualVQ
from amphion_amd.models.codec.amphion_codec.vocos import VocosBackbone, _check_input, _check_tensors, _PwHandle, pw_forward
from amphion_amd.modules.hip_ops import HipConv1d


def init_weights(m):
    """repcodec_model.py:18-24; on a weight-normed conv (the quantizer's projections) the reference's draw lands on the derived ``weight``
    and leaves g / v as they are"""
    if isinstance(m, (nn.Conv1d, nn.Linear, HipConv1d)):
        if "weight" in m._parameters:
            nn.init.trunc_normal_(m.weight, std=0.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)


def no_training(module, who):
    if module.training:
        raise NotImplementedError(f"{who}: training mode is not on the HIP path (the kernels have no backward): call .eval()")


class BackboneLinear(nn.Sequential):
    """``nn.Sequential(VocosBackbone, nn.Linear)`` under the reference's keys (``0.*``, ``1.*``): [B, C, T] -> [B, T, out] like the
    reference's pair; ``forward_cf`` stays channel-first for the models that chain it."""

    def __init__(self, input_channels, dim, intermediate_dim, num_layers, out_features):
        super().__init__(VocosBackbone(input_channels=input_channels, dim=dim, intermediate_dim=intermediate_dim, num_layers=num_layers,
                                       adanorm_num_embeddings=None),
                         nn.Linear(dim, out_features))
        self._pw = _PwHandle()

    def forward_cf(self, x):
        """x [B, C, T], checked, on the current device -> [B, out, T]"""
        bb, lin = self[0], self[1]
        B, _, T = x.shape
        C = bb.norm.normalized_shape[0]
        inter = bb.convnext[0].pwconv1.out_features if len(bb.convnext) else 1
        bufs = {"a": x.new_empty((B, C, T)), "y": x.new_empty((B, C, T)), "h": x.new_empty((B, inter, T))}
        y = bb.forward_cf(x, bufs)
        return pw_forward(self._pw, lin, y, _lib.AMP_PW_BIAS, x.new_empty((B, lin.out_features, T)))

    def forward(self, x):
        x = _check_input(x, self[0].input_channels, "BackboneLinear")
        _check_tensors(self, x.device, "BackboneLinear")
        with _lib.on_device(x.device):
            out = self.forward_cf(x)
        _lib.range_check(x.device)
        return out.transpose(1, 2)


def time_major_input(x, channels, who):
    """[B, T, C] as the tokenizers take their features -> a checked, contiguous [B, C, T] copy"""
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError(f"{who}: expected a [B, T, {channels}] input")
    return _check_input(x.transpose(1, 2), channels, who)


class RepCodec(nn.Module):
    def __init__(self, codebook_size=8192, hidden_size=1024, codebook_dim=8, vocos_dim=384, vocos_intermediate_dim=2048, vocos_num_layers=12,
                 num_quantizers=1, downsample_scale=1, cfg=None):
        super().__init__()

        def pick(name, default, gate=None):
            return getattr(cfg, name) if cfg is not None and hasattr(cfg, gate or name) else default

        codebook_size = pick("codebook_size", codebook_size)
        codebook_dim = pick("codebook_dim", codebook_dim)
        hidden_size = pick("hidden_size", hidden_size)
        vocos_dim = pick("vocos_dim", vocos_dim)
        # the reference reads these two whenever cfg has vocos_dim (repcodec_model.py:68-77)
        vocos_intermediate_dim = pick("vocos_intermediate_dim", vocos_intermediate_dim, gate="vocos_dim")
        vocos_num_layers = pick("vocos_num_layers", vocos_num_layers, gate="vocos_dim")
        num_quantizers = pick("num_quantizers", num_quantizers)
        downsample_scale = pick("downsample_scale", downsample_scale)

        self.codebook_size = codebook_size
        self.codebook_dim = codebook_dim
        self.hidden_size = hidden_size
        self.vocos_dim = vocos_dim
        self.vocos_intermediate_dim = vocos_intermediate_dim
        self.vocos_num_layers = vocos_num_layers
        self.num_quantizers = num_quantizers
        self.downsample_scale = downsample_scale

        if self.downsample_scale is not None and self.downsample_scale > 1:
            self.down = nn.Conv1d(self.hidden_size, self.hidden_size, kernel_size=3, stride=2, padding=1)
            self.up = nn.Conv1d(self.hidden_size, self.hidden_size, kernel_size=3, stride=1, padding=1)

        self.encoder = BackboneLinear(self.hidden_size, self.vocos_dim, self.vocos_intermediate_dim, self.vocos_num_layers, self.hidden_size)
        self.decoder = BackboneLinear(self.hidden_size, self.vocos_dim, self.vocos_intermediate_dim, self.vocos_num_layers, self.hidden_size)
        self.quantizer = ResidualVQ(input_dim=hidden_size, num_quantizers=num_quantizers, codebook_size=codebook_size, codebook_dim=codebook_dim,
                                    quantizer_type="fvq", quantizer_dropout=0.0, commitment=0.15, codebook_loss_weight=1.0, use_l2_normlize=True)
        self.reset_parameters()

    def _encode(self, x):
        no_training(self, "RepCodec")
        x = time_major_input(x, self.hidden_size, "RepCodec")
        _check_tensors(self, x.device, "RepCodec")
        with _lib.on_device(x.device):
            z = self.encoder.forward_cf(x)
            return self.quantizer.encode(z)

    def forward(self, x):
        zq, codes, _ = self._encode(x)
        with _lib.on_device(zq.device):
            x_rec = self.decoder.forward_cf(zq)
        _lib.range_check(zq.device)
        return x_rec.transpose(1, 2), torch.zeros((), device=zq.device), codes

    def quantize(self, x):
        zq, codes, _ = self._encode(x)
        _lib.range_check(zq.device)
        return (codes.squeeze(0) if codes.shape[0] == 1 else codes), zq.transpose(1, 2)

    def reset_parameters(self):
        self.apply(init_weights)
