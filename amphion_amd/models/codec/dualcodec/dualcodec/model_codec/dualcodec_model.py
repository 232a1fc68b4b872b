"""DualCodec (model_codec/dualcodec_model.py:30-214) in eval mode on the gfx950 kernels: wave + semantic features -> codes, codes -> wave.

    prepare_semantic_features   w2v-BERT hidden states [B, T, 1024] -> [B, 1024, T / f]       one launch (amp_semantic_prepare)
    convnext_encoder            WNConv1d(1024, dim, 1) -> ConvNeXt blocks                     1 + 3 per block
    semantic_vq                 one-level residual VQ                                         one launch (amp_fvq_encode_ex)
    convnext_decoder            ConvNeXt blocks -> WNConv1d(dim, 1024, 1)                     3 per block + 1
    dac.encoder / dac.quantizer the DAC encoder stack, then all acoustic levels in one launch with the crop to the semantic length, the
                                subtraction of the semantic latent and its re-addition folded in (amp_fvq_encode_ex)
    decode_from_codes           semantic_vq.from_codes (amp_fvq_decode_add), convnext_decoder, the acoustic levels + the semantic latent in one
                                launch (amp_fvq_decode_add), the DAC decoder stack

Same constructor arguments, submodule names and ``state_dict`` keys as the reference.  ``forward`` returns its two result objects as
``AttrDict`` (a dict with attribute access).  Training mode raises ``NotImplementedError``.  Every forward ends with ``_lib.range_check``."""
from __future__ import annotations

from typing import List, Union

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.codec import _check_channels
from amphion_amd.models.codec.amphion_codec.vocos import _check_tensors

from .cnn import ConvNeXtBlock, run_blocks
from .dac_layers import WNConv1d
from .dac_model import DAC, AttrDict
from .dac_quantize import ResidualVectorQuantize

SEMANTIC_DIM = 1024          # width of the w2v-BERT features and of the DAC latent the semantic branch is subtracted from
CONVNEXT_INTERMEDIATE = 2048


def prepare_semantic_features(hidden, mean=None, std=None, factor=2):
    """hidden [B, T, C] (time-major hidden states) -> [B, C, T // factor] = avg_pool1d(((hidden - mean) / std).transpose(1, 2), factor, factor)
    in one launch; ``mean`` / ``std`` [C] or None (skip that step)"""
    if not isinstance(hidden, torch.Tensor) or hidden.dim() != 3 or min(hidden.shape) < 1:
        raise ValueError(f"prepare_semantic_features: expected a non-empty [B, T, C] tensor, got {tuple(hidden.shape) if isinstance(hidden, torch.Tensor) else type(hidden)}")
    factor = int(factor)
    B, T, C = hidden.shape
    if factor < 1 or T < factor:
        raise ValueError(f"prepare_semantic_features: T = {T} frames do not fill one pooling window of {factor}")
    hidden = _lib.require_device_tensor(hidden, "semantic hidden states")
    dev = hidden.device
    stats = []
    for name, v in (("mean", mean), ("std", std)):
        if v is not None:
            v = torch.as_tensor(v)
            if v.numel() != C:
                raise ValueError(f"prepare_semantic_features: {name} must have {C} entries, got {tuple(v.shape)}")
            v = v.detach().to(device=dev, dtype=torch.float32).reshape(C).contiguous()
        stats.append(v)
    out = torch.empty((B, C, T // factor), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.check(_lib.lib().amp_semantic_prepare(_p(hidden), _p(stats[0]), _p(stats[1]), B, T, C, factor, _p(out), _lib.current_stream_ptr(dev)))
    return out


class DualCodec(nn.Module):
    def __init__(self, encoder_dim: int = 64, encoder_rates: List[int] = [2, 4, 8, 8], latent_dim: int = None, decoder_dim: int = 1536,
                 decoder_rates: List[int] = [8, 8, 4, 2], n_codebooks: int = 9, codebook_size: int = 1024, semantic_codebook_size: int = 16384,
                 codebook_dim: Union[int, list] = 8, semantic_codebook_dim=8, quantizer_dropout: bool = False, sample_rate: int = 44100,
                 distill_projection_out_dim=1024, convnext_dim=768, convnext_layers=4, decode_semantic_for_codec=True, is_causal=False,
                 semantic_downsample_factor=2):
        super().__init__()
        self.semantic_downsample_factor = semantic_downsample_factor
        self.dac = DAC(encoder_dim, encoder_rates, latent_dim, decoder_dim, decoder_rates, n_codebooks, codebook_size, codebook_dim,
                       quantizer_dropout, sample_rate, distill_projection_out_dim, distill=False)
        self.decode_semantic_for_codec = decode_semantic_for_codec
        self.encoder_rates = encoder_rates
        self.convnext_dim = convnext_dim
        self.convnext_layers = convnext_layers
        self.convnext_encoder = nn.Sequential(
            WNConv1d(SEMANTIC_DIM, convnext_dim, kernel_size=1),
            *[ConvNeXtBlock(dim=convnext_dim, intermediate_dim=CONVNEXT_INTERMEDIATE, is_causal=is_causal) for _ in range(convnext_layers)])
        self.semantic_vq = ResidualVectorQuantize(convnext_dim, n_codebooks=1, codebook_size=semantic_codebook_size,
                                                  codebook_dim=semantic_codebook_dim)
        self.convnext_decoder = nn.Sequential(
            *[ConvNeXtBlock(dim=convnext_dim, intermediate_dim=CONVNEXT_INTERMEDIATE, is_causal=is_causal) for _ in range(convnext_layers)],
            WNConv1d(convnext_dim, SEMANTIC_DIM, kernel_size=1))
        if not self.decode_semantic_for_codec:
            assert convnext_dim == 1024

    # ---- the two ConvNeXt stacks: the blocks of a stack share one set of scratch buffers ----
    def _prepare(self, who, semantic_repr=None):
        if self.training:
            raise NotImplementedError(f"DualCodec.{who}: training mode is not on the HIP path (the kernels have no backward): call .eval()")
        if semantic_repr is None:
            return None
        x = _check_channels(semantic_repr, SEMANTIC_DIM, f"DualCodec.{who} semantic_repr")
        _check_tensors(self, x.device, "DualCodec")
        return x

    def run_convnext_encoder(self, x):
        """semantic features [B, 1024, T] -> [B, convnext_dim, T] (a fresh tensor)"""
        with _lib.on_device(x.device):
            return run_blocks(list(self.convnext_encoder)[1:], self.convnext_encoder[0](x))

    def run_convnext_decoder(self, x, owned=False):
        """[B, convnext_dim, T] -> [B, 1024, T]; the blocks work in place on x when it is `owned`, else on a copy"""
        with _lib.on_device(x.device):
            x = run_blocks(list(self.convnext_decoder)[:-1], x if owned else x.clone())
            return self.convnext_decoder[-1](x)

    def _semantic(self, x, want_latents=False):
        """-> (semantic latent as the DAC takes it, codes [B, 1, T], latents or None)"""
        codes, zq, _, latents = self.semantic_vq.run_encode(self.run_convnext_encoder(x), want_latents=want_latents)
        semantic = self.run_convnext_decoder(zq, owned=True) if self.decode_semantic_for_codec else zq
        return semantic, codes.transpose(0, 1).contiguous(), latents

    # ---- the reference's methods ----
    def semantic_quantize(self, semantic_repr):
        """semantic_repr [B, 1024, T] -> codes [B, T] int64"""
        x = self._prepare("semantic_quantize", semantic_repr)
        codes, _, _, _ = self.semantic_vq.run_encode(self.run_convnext_encoder(x), want_sum=False)
        _lib.range_check(x.device)
        return codes[0]

    def encode(self, audio_data, num_quantizers=None, sample_rate=24000, semantic_repr=None):
        """-> (semantic_codes [B, 1, T], acoustic_codes [B, n - 1, T] or None when num_quantizers == 1)"""
        x = self._prepare("encode", semantic_repr)
        if x is None:
            raise ValueError("DualCodec.encode: semantic_repr is required")
        if num_quantizers == 1:
            return self.semantic_quantize(x)[:, None, :], None
        semantic, semantic_codes, _ = self._semantic(x)
        if num_quantizers is not None:
            num_quantizers -= 1
        acoustic_codes = self.dac.encode_codes(audio_data, sample_rate=sample_rate, n_quantizers=num_quantizers, subtracted_latent=semantic)
        return semantic_codes, acoustic_codes

    @torch.no_grad()
    def decode_from_codes(self, semantic_codes, acoustic_codes):
        """semantic_codes [B, 1, T], acoustic_codes [B, n, T] or None -> wave [B, 1, T * hop (less what odd rates drop)]"""
        self._prepare("decode_from_codes")
        if isinstance(semantic_codes, torch.Tensor) and semantic_codes.is_cuda:
            _check_tensors(self, semantic_codes.device, "DualCodec")
        semantic = self.semantic_vq.run_decode(semantic_codes)
        if self.decode_semantic_for_codec:
            semantic = self.run_convnext_decoder(semantic, owned=True)
        return self.dac.decode_from_codes(acoustic_codes, semantic)

    def forward(self, audio_data, sample_rate: int = 24000, n_quantizers: int = None, semantic_repr=None, bypass_quantize_rate=0.125,
                possibly_no_quantizer=False):
        """eval mode: -> (acoustic result, semantic result), two ``AttrDict``; n_quantizers == 1 bypasses the acoustic quantizer"""
        x = self._prepare("forward", semantic_repr)
        if x is None:
            raise ValueError("DualCodec.forward: semantic_repr is required")
        semantic, codes, latents = self._semantic(x, want_latents=True)
        commitment_loss, codebook_loss = self.semantic_vq.losses(latents, codes)
        bypass_quantize = n_quantizers == 1
        if n_quantizers is not None:
            n_quantizers = n_quantizers - 1
        acoustic = self.dac(audio_data, sample_rate, n_quantizers, subtracted_latent=semantic, bypass_quantize=bypass_quantize,
                            possibly_no_quantizer=possibly_no_quantizer)
        if not self.decode_semantic_for_codec:
            semantic = self.run_convnext_decoder(semantic)
        _lib.range_check(x.device)
        return acoustic, AttrDict({"x": semantic, "codes": codes, "latents": latents, "penalty": commitment_loss,
                                   "vq/codebook_loss": codebook_loss, "metrics": {}, "bypassed_quantize": bypass_quantize})
