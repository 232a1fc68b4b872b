"""ResidualVectorQuantizer drop-in (models/codec/speechtokenizer/modules/quantization/vq.py:34-125), eval mode, on csrc/evq.hip."""
from __future__ import annotations

import typing as tp

import torch
from torch import nn

from .core_vq import ResidualVectorQuantization


class ResidualVectorQuantizer(nn.Module):
    def __init__(self, dimension: int = 256, n_q: int = 8, bins: int = 1024, decay: float = 0.99, kmeans_init: bool = True,
                 kmeans_iters: int = 50, threshold_ema_dead_code: int = 2):
        super().__init__()
        self.n_q = n_q
        self.dimension = dimension
        self.bins = bins
        self.decay = decay
        self.kmeans_init = kmeans_init
        self.kmeans_iters = kmeans_iters
        self.threshold_ema_dead_code = threshold_ema_dead_code
        self.vq = ResidualVectorQuantization(dim=self.dimension, codebook_size=self.bins, num_quantizers=self.n_q, decay=self.decay,
                                             kmeans_init=self.kmeans_init, kmeans_iters=self.kmeans_iters,
                                             threshold_ema_dead_code=self.threshold_ema_dead_code)

    def forward(self, x: torch.Tensor, n_q: tp.Optional[int] = None, layers: tp.Optional[list] = None):
        """-> (quantized [B, D, T], codes [n_q, B, T], commit_loss = the zero scalar of eval mode, the quantized of the levels in ``layers``)"""
        n_q = n_q if n_q else self.n_q
        if layers and max(layers) >= n_q:
            raise ValueError(f"ResidualVectorQuantizer: layers asks for level {max(layers)}, but only levels 0 .. {n_q - 1} are run")
        quantized, codes, commit_loss, quantized_list = self.vq(x, n_q=n_q, layers=layers)
        # torch.mean of the levels' zero losses: a scalar view of them, no kernel
        return quantized, codes, commit_loss[0, 0], quantized_list

    def encode(self, x: torch.Tensor, n_q: tp.Optional[int] = None, st: tp.Optional[int] = None) -> torch.Tensor:
        n_q = n_q if n_q else self.n_q
        st = st or 0
        return self.vq.encode(x, n_q=n_q, st=st)

    def decode(self, codes: torch.Tensor, st: int = 0) -> torch.Tensor:
        return self.vq.decode(codes, st=st)
