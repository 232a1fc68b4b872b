"""SpeechTokenizer drop-in (models/codec/speechtokenizer/model.py:14-184) on the gfx950 kernels, eval mode only.  Same constructor (a config
mapping), ``state_dict`` keys and call contracts.

    encoder     SEANetEncoder: ELU + reflect-pad staging (amp_elu_pad) in front of the implicit-GEMM / strided conv kernels, a bidirectional
                2-layer LSTM (amp_lstm_forward: one GEMM per layer for the input projection, one exact-fp32 launch per time step)
    quantizer   ResidualVectorQuantizer: all levels in one exact-fp32 launch (amp_evq_encode), decode one gather-sum launch
    transform   nn.Linear(dimension, semantic_dimension) on the first requested level's output: amp_pw_forward in the conv layout, returned
                as the [B, T, semantic_dimension] view
    decoder     SEANetDecoder: conv, unidirectional LSTM, ELU -> amp_tconv_forward -> residual blocks per ratio, last conv

``encode`` and ``decode`` end with the op-level range check (``_lib.range_check``): an activation beyond the split-f16 operand range raises
``AmpError`` (AMP_ERR_RANGE) -- re-run under ``_lib.set_precision("f32")`` (AMP_PRECISION=f32), the exact-fp32 route.  The only torch ops on
the path are allocations, one zero fill (the levels' losses, which eval mode leaves at 0) and views.  ``.train()`` forwards raise ``NotImplementedError``."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle, pw_forward

from .modules.quantization import ResidualVectorQuantizer
from .modules.seanet import SEANetDecoder, SEANetEncoder


def _kw(config, **names):
    """the constructor arguments the config sets (a key that is absent or None keeps the class's default, where the reference would pass None)"""
    return {arg: config.get(key) for arg, key in names.items() if config.get(key) is not None}


class SpeechTokenizer(nn.Module):
    def __init__(self, config):
        super().__init__()
        common = _kw(config, n_filters="n_filters", dimension="dimension", ratios="strides", lstm="lstm_layers", dilation_base="dilation_base",
                     residual_kernel_size="residual_kernel_size", n_residual_layers="n_residual_layers", activation="activation")
        self.encoder = SEANetEncoder(bidirectional=bool(config.get("bidirectional")), **common)
        self.sample_rate = config.get("sample_rate")
        self.n_q = config.get("n_q")
        self.downsample_rate = np.prod(config.get("strides"))
        if config.get("dimension") != config.get("semantic_dimension"):
            self.transform = nn.Linear(config.get("dimension"), config.get("semantic_dimension"))
        else:
            self.transform = nn.Identity()
        self.quantizer = ResidualVectorQuantizer(dimension=config.get("dimension"), n_q=config.get("n_q"), bins=config.get("codebook_size"))
        self.decoder = SEANetDecoder(bidirectional=False, **common)
        self._pw = _PwHandle()

    @classmethod
    def load_from_checkpoint(cls, config_path: str, ckpt_path: str):
        import json

        with open(config_path) as f:
            cfg = json.load(f)
        model = cls(cfg)
        params = torch.load(ckpt_path, map_location="cpu")
        model.load_state_dict(params)
        return model

    def _feature(self, q):
        """transform(q as [B, T, D]) -> [B, T, semantic_dimension]"""
        if isinstance(self.transform, nn.Identity):
            return q.transpose(1, 2)
        out = torch.empty((q.shape[0], self.transform.out_features, q.shape[2]), dtype=torch.float32, device=q.device)
        pw_forward(self._pw, self.transform, q.contiguous(), _lib.AMP_PW_BIAS, out)
        return out.transpose(1, 2)

    def forward(self, x: torch.tensor, n_q: int = None, layers: list = [0]):
        """-> (o [B, 1, T'], commit_loss (the zero scalar of eval mode), feature [B, frames, semantic_dimension])"""
        n_q = n_q if n_q else self.n_q
        e = self.encoder(x)
        quantized, codes, commit_loss, quantized_list = self.quantizer(e, n_q=n_q, layers=layers)
        feature = self._feature(quantized_list[0])
        o = self.decoder(quantized)
        return o, commit_loss, feature

    def forward_feature(self, x: torch.tensor, layers: list = None):
        e = self.encoder(x)
        layers = layers if layers else list(range(self.n_q))
        quantized, codes, commit_loss, quantized_list = self.quantizer(e, layers=layers)
        return quantized_list

    def encode(self, x: torch.tensor, n_q: int = None, st: int = None):
        """-> codes [n_q - st, B, frames]"""
        e = self.encoder(x)
        if st is None:
            st = 0
        n_q = n_q if n_q else self.n_q
        codes = self.quantizer.encode(e, n_q=n_q, st=st)
        _lib.range_check(x.device)
        return codes

    def decode(self, codes: torch.tensor, st: int = 0):
        """codes [n, B, frames] -> wave [B, 1, frames * hop]"""
        quantized = self.quantizer.decode(codes, st=st)
        o = self.decoder(quantized)
        _lib.range_check(o.device)
        return o
