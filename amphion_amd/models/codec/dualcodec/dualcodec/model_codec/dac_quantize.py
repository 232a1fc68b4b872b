"""DualCodec's DAC quantizers (model_codec/dac_quantize.py:23-262) in eval mode on the exact-fp32 quantizer kernels (csrc/fvq.hip).  Same
constructor arguments and ``state_dict`` keys (``quantizers.i.{in_proj,out_proj}.{weight_g,weight_v,bias}`` weight-normed or folded,
``quantizers.i.codebook.weight``).

``ResidualVectorQuantize.forward`` is ONE launch of ``amp_fvq_encode_ex`` for all levels: z_q, the codes, every level's projected latent
``z_e`` and the first level's z_q come out of it; the two losses are torch ops on those latents and codes (not a hot path).  ``from_codes`` is
one launch of ``amp_fvq_decode_add``; a code outside the codebook raises ``AmpError`` (``amp_fvq_check``).  ``run_encode`` / ``run_decode`` take
the tensor that ``DAC`` subtracts before and adds after the quantizer, folded into the same launches.

Not on the HIP path (``NotImplementedError``): training mode, and a ``codebook_dim`` list whose entries differ."""
from __future__ import annotations

import ctypes
from typing import Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32_array, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.quantize.factorized_vector_quantize import _no_training

from .dac_layers import WNConv1d


class _Handle:
    """The device copy of a stack of ``VectorQuantize`` levels for ``amp_fvq_*`` (always with projections, l2-normalised look-up), rebuilt when
    a parameter or the device changes."""

    def __init__(self):
        self._cache = HandleCache("amp_fvq_destroy")

    def get(self, levels, device):
        return self._cache.get(param_sig([p for q in levels for p in q.parameters()], str(device), len(levels)), self._build, levels, device)

    def _build(self, levels, device):
        q0 = levels[0]
        cb = host_f32_array([q.codebook.weight for q in levels])
        wi = host_f32_array([q.in_proj.folded_weight() for q in levels])
        bi = host_f32_array([q.in_proj.bias for q in levels])
        wo = host_f32_array([q.out_proj.folded_weight() for q in levels])
        bo = host_f32_array([q.out_proj.bias for q in levels])
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_fvq_create(q0.input_dim, q0.codebook_dim, q0.codebook_size, len(levels), 1, wi, bi, cb, wo, bo, ctypes.byref(h)))
        return h


def _encode(handle, levels, z, n, sub=None, want_sum=True, want_all=False, want_latents=False):
    """z [B, D, Tz] (columns [0, T) are read; T = sub's length when given) -> (codes int64 [n, B, T], z_q (+ sub) [B, D, T] or None,
    every level's z_q [n, B, D, T] or None, latents [B, n * d, T] or None)"""
    q0 = levels[0]
    D, d = q0.input_dim, q0.codebook_dim
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.shape[0] < 1 or z.shape[2] < 1:
        raise ValueError(f"quantizer: expected a non-empty [B, {D}, T] tensor, got {tuple(z.shape) if isinstance(z, torch.Tensor) else type(z)}")
    if z.shape[1] != D:
        raise ValueError(f"quantizer: expected {D} input channels, got {z.shape[1]}")
    z = _lib.require_device_tensor(z, "quantizer input")
    B, _, Tz = z.shape
    T = Tz
    if sub is not None:
        if not isinstance(sub, torch.Tensor) or sub.dim() != 3 or sub.shape[0] != B or sub.shape[1] != D or sub.shape[2] < 1:
            raise ValueError(f"quantizer: the subtracted latent must be [{B}, {D}, T], got {tuple(sub.shape) if isinstance(sub, torch.Tensor) else type(sub)}")
        sub = _lib.require_device_tensor(sub, "subtracted latent")
        T = sub.shape[2]
        if not 0 <= Tz - T <= 2:
            raise ValueError(f"quantizer: the latent has {Tz} frames, the subtracted latent {T}: at most 2 more are cropped")
    dev = z.device
    h = handle.get(levels, dev)
    codes = torch.empty((n, B, T), dtype=torch.int64, device=dev)
    zq = torch.empty((B, D, T), dtype=torch.float32, device=dev) if want_sum else None
    allq = torch.empty((n, B, D, T), dtype=torch.float32, device=dev) if want_all else None
    lat = torch.empty((B, n * d, T), dtype=torch.float32, device=dev) if want_latents else None
    with _lib.on_device(dev):
        _lib.check(_lib.lib().amp_fvq_encode_ex(h, _p(z), Tz, _p(sub), B, T, n, _p(codes), _p(zq), _p(allq), _p(lat), _lib.current_stream_ptr(dev)))
    return codes, zq, allq, lat


def _decode(handle, levels, codes, add=None):
    """codes [B, n, T] integers on the device -> sum of the levels' out_proj(codebook[code]) (+ add) [B, D, T]"""
    if not isinstance(codes, torch.Tensor) or codes.dim() != 3 or not 1 <= codes.shape[1] <= len(levels) or codes.shape[0] < 1 or codes.shape[2] < 1:
        raise ValueError(f"from_codes: expected codes [B, 1..{len(levels)}, T], got {tuple(codes.shape) if isinstance(codes, torch.Tensor) else type(codes)}")
    if codes.dtype.is_floating_point or codes.dtype == torch.bool:
        raise TypeError(f"from_codes: the codes must be integers, got {codes.dtype}")
    if not codes.is_cuda:
        raise RuntimeError("from_codes: the codes must be a tensor on a ROCm device (there is no CPU fallback)")
    B, n, T = codes.shape
    dev = codes.device
    D = levels[0].input_dim
    if add is not None:
        if not isinstance(add, torch.Tensor) or tuple(add.shape) != (B, D, T):
            raise ValueError(f"from_codes: the added latent must be [{B}, {D}, {T}], got {tuple(add.shape) if isinstance(add, torch.Tensor) else type(add)}")
        add = _lib.require_device_tensor(add, "added latent")
    nbt = codes.to(torch.int64).transpose(0, 1).contiguous()
    h = handle.get(levels, dev)
    out = torch.empty((B, D, T), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        st = _lib.current_stream_ptr(dev)
        _lib.check(_lib.lib().amp_fvq_decode_add(h, _p(nbt), n, B, T, _p(add), _p(out), st))
        _lib.check(_lib.lib().amp_fvq_check(h, st))
    return out


class VectorQuantize(nn.Module):
    """dac_quantize.py:23-104: in_proj -> nearest l2-normalised codebook row -> out_proj"""

    def __init__(self, input_dim: int, codebook_size: int, codebook_dim: int):
        super().__init__()
        self.input_dim = input_dim
        self.codebook_size = codebook_size
        self.codebook_dim = codebook_dim
        self.in_proj = WNConv1d(input_dim, codebook_dim, kernel_size=1)
        self.out_proj = WNConv1d(codebook_dim, input_dim, kernel_size=1)
        self.codebook = nn.Embedding(codebook_size, codebook_dim)
        self._handle = _Handle()

    def forward(self, z):
        """-> (z_q [B, D, T], commitment_loss [B], codebook_loss [B], indices [B, T], z_e [B, d, T])"""
        _no_training(self, "VectorQuantize")
        codes, z_q, _, z_e = _encode(self._handle, [self], z, 1, want_latents=True)
        loss = _level_loss(z_e, codes[0], self.codebook.weight)
        _lib.range_check(z.device)
        return z_q, loss, loss.clone(), codes[0], z_e

    def embed_code(self, embed_id):
        return F.embedding(embed_id, self.codebook.weight)

    def decode_code(self, embed_id):
        return self.embed_code(embed_id).transpose(1, 2)


def _level_loss(z_e, idx, codebook):
    """F.mse_loss(z_e, codebook[idx], reduction="none").mean([1, 2]) -> [B]: the commitment and the codebook loss have this one forward value"""
    z_q = F.embedding(idx, codebook.detach()).transpose(1, 2)
    return (z_e - z_q).pow(2).mean([1, 2])


class ResidualVectorQuantize(nn.Module):
    """dac_quantize.py:134-262"""

    def __init__(self, input_dim: int = 512, n_codebooks: int = 9, codebook_size: int = 1024, codebook_dim: Union[int, list] = 8,
                 quantizer_dropout: float = 0.0):
        super().__init__()
        if isinstance(codebook_dim, int):
            codebook_dim = [codebook_dim for _ in range(n_codebooks)]
        codebook_dim = list(codebook_dim)
        if len(codebook_dim) != n_codebooks:
            raise ValueError(f"ResidualVectorQuantize: {len(codebook_dim)} codebook_dim entries for {n_codebooks} codebooks")
        if len(set(codebook_dim)) > 1:
            raise NotImplementedError("ResidualVectorQuantize: per-level codebook_dim values that differ are not on the HIP path "
                                      "(one kernel walks all levels with one width)")
        self.input_dim = input_dim
        self.n_codebooks = n_codebooks
        self.codebook_dim = codebook_dim
        self.codebook_size = codebook_size
        self.quantizers = nn.ModuleList([VectorQuantize(input_dim, codebook_size, codebook_dim[i]) for i in range(n_codebooks)])
        self.quantizer_dropout = quantizer_dropout
        self._handle = _Handle()

    def _levels(self, n_quantizers):
        n = self.n_codebooks if n_quantizers is None else min(int(n_quantizers), self.n_codebooks)
        if n < 1:
            raise ValueError(f"ResidualVectorQuantize: n_quantizers={n_quantizers} leaves no quantizer")
        return n

    def run_encode(self, z, n_quantizers=None, sub=None, want_sum=True, want_all=False, want_latents=False):
        """the launch behind ``forward``: (codes [n, B, T], z_q + sub, every level's z_q, latents), see ``_encode``"""
        _no_training(self, "ResidualVectorQuantize")
        return _encode(self._handle, list(self.quantizers), z, self._levels(n_quantizers), sub, want_sum, want_all, want_latents)

    def run_decode(self, codes, add=None):
        return _decode(self._handle, list(self.quantizers), codes, add)

    def losses(self, latents, codes):
        """(commitment_loss, codebook_loss) of ``forward`` from its latents [B, n * d, T] and codes [B, n, T]: per level the mean over the
        batch of mse(z_e, codebook[code]), summed over the levels"""
        d = self.codebook_dim[0]
        total = latents.new_zeros(())
        for i in range(codes.shape[1]):
            total = total + _level_loss(latents[:, i * d:(i + 1) * d], codes[:, i], self.quantizers[i].codebook.weight).mean()
        return total, total.clone()

    def forward(self, z, n_quantizers: int = None, possibly_no_quantizer=False, subtracted_latent=None):
        """-> (z_q, codes [B, n, T] int64, latents [B, n * d, T], commitment_loss, codebook_loss, z_q_1).  ``subtracted_latent`` (not in the
        reference's signature): quantize z[..., :T] - it and return z_q + it, as ``DAC.encode`` does around this call."""
        codes, z_q, allq, latents = self.run_encode(z, n_quantizers, subtracted_latent, want_all=True, want_latents=True)
        codes = codes.transpose(0, 1).contiguous()
        commitment_loss, codebook_loss = self.losses(latents, codes)
        _lib.range_check(z.device)
        return z_q, codes, latents, commitment_loss, codebook_loss, allq[0]

    def from_codes(self, codes: torch.Tensor):
        """codes [B, n, T] -> (z_q [B, D, T], z_p [B, n * d, T] the codebook rows, codes)"""
        z_q = self.run_decode(codes)                              # raises on a code outside the codebook before anything indexes with it
        z_p = torch.cat([self.quantizers[i].decode_code(codes[:, i, :]) for i in range(codes.shape[1])], dim=1)
        _lib.range_check(codes.device)
        return z_q, z_p, codes
