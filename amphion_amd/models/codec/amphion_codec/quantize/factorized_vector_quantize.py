"""FactorizedVectorQuantize drop-in (models/codec/amphion_codec/quantize/factorized_vector_quantize.py:22-150), eval mode, on the
exact-fp32 quantizer kernels (csrc/fvq.hip).  Same constructor, ``state_dict`` keys (``in_project`` / ``out_project`` weight-normed or
folded, ``codebook.weight``) and call contracts.  Training mode raises ``NotImplementedError``: the kernels have no backward."""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32_array, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.modules.hip_ops import HipConv1d


def _no_training(module, who):
    if module.training:
        raise NotImplementedError(f"{who}: training mode is not on the HIP path (the quantizer kernels have no backward): call .eval()")


class FvqHandle:
    """The device copy of a stack of quantizer levels for ``amp_fvq_*``, rebuilt when a parameter, the device or the projection form
    changes.  ``project=False`` builds the identity form over the codebook space (``decode_latents``, ``vq2emb(out_proj=False)``)."""

    def __init__(self, project=True):
        self.project = project
        self._cache = HandleCache("amp_fvq_destroy")

    def get(self, levels, device):
        return self._cache.get(param_sig([p for q in levels for p in q.parameters()], str(device), len(levels)), self._build, levels, device)

    def _build(self, levels, device):
        q0 = levels[0]
        cb = host_f32_array([q.codebook.weight for q in levels])
        if self.project and q0.input_dim != q0.codebook_dim:
            wi = host_f32_array([q.in_project.folded_weight() for q in levels])
            bi = host_f32_array([q.in_project.bias for q in levels])
            wo = host_f32_array([q.out_project.folded_weight() for q in levels])
            bo = host_f32_array([q.out_project.bias for q in levels])
        else:
            wi = bi = wo = bo = None
        h = ctypes.c_void_p()
        D = q0.input_dim if self.project else q0.codebook_dim
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_fvq_create(D, q0.codebook_dim, q0.codebook_size, len(levels), int(bool(q0.use_l2_normlize)), wi, bi, cb, wo, bo,
                                                 ctypes.byref(h)))
        return h


def fvq_encode(handle, levels, z, n, want_sum=True, want_all=False):
    """-> (codes int64 [n, B, T], quantized_out [B, D, T] or None, all_quantized [n, B, D, T] or None)"""
    q0 = levels[0]
    want = q0.input_dim if handle.project else q0.codebook_dim      # the width the kernel indexes z, zq and all_zq with
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.shape[0] < 1 or z.shape[2] < 1:
        raise ValueError(f"quantizer: expected a non-empty [B, {want}, T] tensor, got {tuple(z.shape) if isinstance(z, torch.Tensor) else type(z)}")
    if z.shape[1] != want:
        raise ValueError(f"quantizer: expected {want} input channels, got {z.shape[1]}")
    z = _lib.require_device_tensor(z, "quantizer input")
    B, D, T = z.shape
    dev = z.device
    h = handle.get(levels, dev)
    codes = torch.empty((n, B, T), dtype=torch.int64, device=dev)
    zq = torch.empty_like(z) if want_sum else None
    allq = torch.empty((n, B, D, T), dtype=torch.float32, device=dev) if want_all else None
    with _lib.on_device(dev):
        _lib.check(_lib.lib().amp_fvq_encode(h, _p(z), B, T, n, _p(codes), _p(zq), _p(allq), _lib.current_stream_ptr(dev)))
    return codes, zq, allq


def fvq_decode(handle, levels, codes, n):
    """codes int64 [n.., B, T] on the device -> [B, D, T]; an index outside the codebook raises ``AmpError`` (AMP_ERR_INVALID)"""
    if not isinstance(codes, torch.Tensor) or codes.dim() != 3 or codes.shape[0] < n or codes.shape[1] < 1 or codes.shape[2] < 1:
        raise ValueError(f"vq2emb: expected codes [>= {n}, B, T], got {tuple(codes.shape) if isinstance(codes, torch.Tensor) else type(codes)}")
    if codes.dtype.is_floating_point or codes.dtype == torch.bool:
        raise TypeError(f"vq2emb: the codes must be integers, got {codes.dtype}")
    if not codes.is_cuda:
        raise RuntimeError("vq2emb: the codes must be a tensor on a ROCm device (there is no CPU fallback)")
    codes = codes[:n].to(torch.int64).contiguous()
    _, B, T = codes.shape
    dev = codes.device
    h = handle.get(levels, dev)
    q0 = levels[0]
    D = q0.input_dim if handle.project else q0.codebook_dim
    out = torch.empty((B, D, T), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        st = _lib.current_stream_ptr(dev)
        _lib.check(_lib.lib().amp_fvq_decode(h, _p(codes), n, B, T, _p(out), st))
        _lib.check(_lib.lib().amp_fvq_check(h, st))
    return out


class FactorizedVectorQuantize(nn.Module):
    def __init__(self, input_dim, codebook_size, codebook_dim, commitment=0.005, codebook_loss_weight=1.0, use_l2_normlize=True):
        super().__init__()
        self.input_dim = input_dim
        self.codebook_size = codebook_size
        self.codebook_dim = codebook_dim
        self.commitment = commitment
        self.codebook_loss_weight = codebook_loss_weight
        self.use_l2_normlize = use_l2_normlize
        if self.input_dim != self.codebook_dim:
            self.in_project = HipConv1d(self.input_dim, self.codebook_dim, 1)
            self.out_project = HipConv1d(self.codebook_dim, self.input_dim, 1)
        else:
            self.in_project = nn.Identity()
            self.out_project = nn.Identity()
        self.codebook = nn.Embedding(self.codebook_size, self.codebook_dim)
        self._full, self._latent = FvqHandle(True), FvqHandle(False)

    def forward(self, z):
        """z [B, D, T] -> (z_q [B, D, T], commit_loss [B] = 0, codebook_loss [B] = 0, indices [B, T], z_e [B, d, T]).  z_q and the
        indices come from the exact-fp32 kernel; z_e, which the eval path only hands back, from ``in_project`` on the conv kernels."""
        _no_training(self, "FactorizedVectorQuantize")
        codes, z_q, _ = fvq_encode(self._full, [self], z, 1)
        z_e = self.in_project(z)
        zero = torch.zeros(z.shape[0], device=z.device)
        return z_q, zero, zero.clone(), codes[0], z_e

    def embed_code(self, embed_id):
        return self.decode_code(embed_id).transpose(1, 2)

    def decode_code(self, embed_id):
        return fvq_decode(self._latent, [self], embed_id[None], 1)

    def decode_latents(self, latents):
        codes, _, _ = fvq_encode(self._latent, [self], latents, 1, want_sum=False)
        return self.decode_code(codes[0]), codes[0]

    def vq2emb(self, vq, out_proj=True):
        return fvq_decode(self._full if out_proj else self._latent, [self], vq[None], 1)

    def latent2dist(self, latents):
        """The [B, T, K] distance tensor is formed with torch ops on the device, like the reference (not on the hot path)."""
        B, d, T = latents.shape
        encodings = latents.transpose(1, 2).reshape(B * T, d)
        codebook = self.codebook.weight
        if self.use_l2_normlize:
            encodings = F.normalize(encodings)
            codebook = F.normalize(codebook)
        dist = encodings.pow(2).sum(1, keepdim=True) - 2 * encodings @ codebook.t() + codebook.pow(2).sum(1, keepdim=True).t()
        indices = (-dist).max(1)[1].reshape(B, T)
        z_q = F.embedding(indices, self.codebook.weight).transpose(1, 2)
        return -dist.reshape(B, T, -1), indices, z_q
