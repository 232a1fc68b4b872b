"""ResidualVQ drop-in (models/codec/amphion_codec/quantize/residual_vq.py:22-177) for ``quantizer_type="fvq"`` in eval mode: all levels of
``forward`` are ONE launch of the exact-fp32 kernel (csrc/fvq.hip), the residual never leaves the chip; ``vq2emb`` is one gather-sum launch."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd.models.codec.amphion_codec.quantize.factorized_vector_quantize import (FactorizedVectorQuantize, FvqHandle, _no_training,
                                                                                        fvq_decode, fvq_encode)


class ResidualVQ(nn.Module):
    def __init__(self, input_dim: int = 256, num_quantizers: int = 8, codebook_size: int = 1024, codebook_dim: int = 256,
                 quantizer_type: str = "vq", quantizer_dropout: float = 0.5, **kwargs):
        super().__init__()
        self.input_dim = input_dim
        self.num_quantizers = num_quantizers
        self.codebook_size = codebook_size
        self.codebook_dim = codebook_dim
        self.quantizer_type = quantizer_type
        self.quantizer_dropout = quantizer_dropout
        if quantizer_type in ("vq", "lfq"):
            raise NotImplementedError(f"ResidualVQ quantizer_type={quantizer_type!r} is not on the HIP path: the shipped codec configs use 'fvq'")
        if quantizer_type != "fvq":
            raise ValueError(f"Unknown quantizer type {quantizer_type}")
        self.quantizers = nn.ModuleList([FactorizedVectorQuantize(input_dim=input_dim, codebook_size=codebook_size, codebook_dim=codebook_dim,
                                                                  **kwargs) for _ in range(num_quantizers)])
        self._handle = FvqHandle(True)

    def _levels(self, n_quantizers):
        n = self.num_quantizers if n_quantizers is None else min(int(n_quantizers), self.num_quantizers)
        if n < 1:
            raise ValueError(f"ResidualVQ: n_quantizers={n_quantizers} leaves no quantizer")
        return n

    def encode(self, z, n_quantizers=None, want_all=False):
        """-> (quantized_out [B, D, T], all_indices [n, B, T], all_quantized [n, B, D, T] or None): the hot path of ``quantize``"""
        _no_training(self, "ResidualVQ")
        n = self._levels(n_quantizers)
        codes, zq, allq = fvq_encode(self._handle, list(self.quantizers), z, n, want_all=want_all)
        return zq, codes, allq

    def forward(self, z, n_quantizers: int = None):
        """-> (quantized_out, all_indices [n, B, T], all_commit_losses [n] = 0, all_codebook_losses [n] = 0, all_quantized [n, B, D, T])"""
        zq, codes, allq = self.encode(z, n_quantizers, want_all=True)
        zero = torch.zeros(codes.shape[0], device=z.device)
        return zq, codes, zero, zero.clone(), allq

    def vq2emb(self, vq, n_quantizers=None):
        n = self._levels(n_quantizers)
        return fvq_decode(self._handle, list(self.quantizers), vq, n)

    def latent2dist(self, z, n_quantizers=None):
        """As the reference writes it (each level's ``latent2dist`` on the running residual); torch ops, not on the hot path."""
        residual = z
        all_dists, all_indices = [], []
        n = self._levels(n_quantizers)
        for quantizer in list(self.quantizers)[:n]:
            dist_i, indices_i, z_q_i = quantizer.latent2dist(residual)
            all_dists.append(dist_i)
            all_indices.append(indices_i)
            residual = residual - z_q_i
        return torch.stack(all_dists), torch.stack(all_indices)
