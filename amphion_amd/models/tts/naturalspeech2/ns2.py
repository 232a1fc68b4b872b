"""models/tts/naturalspeech2/ns2.py on the HIP kernels: NaturalSpeech2 zero-shot TTS, inference only.

    prompt        ``code_to_latent`` (``amp_evq_decode`` over the EnCodec codebooks) -> ``prompt_lin`` -> the prompt encoder, which runs DENSE over
                  the padded prompt (plain LayerNorm and convs over the full length; only its attention sees ``ref_mask``), as the reference does
    query tokens  the 32 learned queries attend to the prompt: q GEMM on the embedding table, the stacked k | v GEMM on the prompt,
                  ``amp_cross_attention`` with the prompt's key mask, ``out_proj``
    prior         PriorEncoder (prior_encoder.py)
    solver        Diffusion / DiffusionFlow ``reverse_diffusion`` (diffusion.py, diffusion_flow.py, wavenet.py)

The quantizer is kept as buffers under the names the ``encodec`` package gives them, ``quantizer.vq.layers.{i}._codebook.{inited,cluster_size,
embed,embed_avg}``, so a checkpoint of the reference loads and saves under its own keys; the package itself is not needed.  Its size is
EnCodec's at 24 kHz (32 codebooks of 1024 x 128) unless ``cfg.codec`` (``n_q``, ``codebook_size``, ``dim``) says otherwise.

``forward`` (training), ``latent_to_code`` and ``reverse_diffusion_from_t`` raise NotImplementedError.  ``latent_dim == encoder_hidden`` is
refused: the reference builds no ``prompt_lin`` then and calls it anyway."""
from __future__ import annotations

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle
from amphion_amd.models.codec.speechtokenizer.modules.quantization.core_vq import EuclideanCodebook, EvqHandle, evq_decode
from amphion_amd.models.tts.naturalspeech2.diffusion import Diffusion
from amphion_amd.models.tts.naturalspeech2.diffusion_flow import DiffusionFlow
from amphion_amd.models.tts.naturalspeech2.prior_encoder import PriorEncoder
from amphion_amd.models.vc.flow_matching_transformer.llama_nar import _pw
from amphion_amd.modules.hip_ops import cross_attention
from amphion_amd.modules.naturalpseech2.transformers import TransformerEncoder, _check_mha, _key_mask, _RowsHandle, mha_rows


class _VqLayer(nn.Module):
    def __init__(self, dim, codebook_size):
        super().__init__()
        self._codebook = EuclideanCodebook(dim, codebook_size, kmeans_init=True)


class _Rvq(nn.Module):
    def __init__(self, n_q, dim, codebook_size):
        super().__init__()
        self.layers = nn.ModuleList([_VqLayer(dim, codebook_size) for _ in range(n_q)])


class Quantizer(nn.Module):
    """the buffers of EnCodec's ResidualVectorQuantizer under its names; ``decode`` is the sum of the look-ups"""

    def __init__(self, n_q=32, dim=128, codebook_size=1024):
        super().__init__()
        self.vq = _Rvq(n_q, dim, codebook_size)
        self._handle = EvqHandle()
        self.requires_grad_(False)

    def decode(self, codes):
        """codes [n, B, T] integers on the device, n <= n_q -> [B, dim, T]"""
        books = [layer._codebook for layer in self.vq.layers]
        return evq_decode(self._handle, books, codes, 0)


class NaturalSpeech2(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.latent_dim = cfg.latent_dim
        self.query_emb_num = cfg.query_emb.query_token_num
        if self.latent_dim == cfg.prompt_encoder.encoder_hidden:
            raise NotImplementedError("NaturalSpeech2: latent_dim == prompt_encoder.encoder_hidden builds no prompt_lin, which the reference's "
                                      "inference then calls: not supported")
        self.prior_encoder = PriorEncoder(cfg.prior_encoder)
        kind = getattr(cfg.diffusion, "diffusion_type", "diffusion")
        if kind == "diffusion":
            self.diffusion = Diffusion(cfg.diffusion)
        elif kind == "flow":
            self.diffusion = DiffusionFlow(cfg.diffusion)
        else:
            raise ValueError(f"NaturalSpeech2: diffusion_type must be 'diffusion' or 'flow', got {kind!r}")
        self.prompt_encoder = TransformerEncoder(cfg=cfg.prompt_encoder)
        self.prompt_lin = nn.Linear(self.latent_dim, cfg.prompt_encoder.encoder_hidden)
        self.prompt_lin.weight.data.normal_(0.0, 0.02)
        self.query_emb = nn.Embedding(self.query_emb_num, cfg.query_emb.hidden_size)
        self.query_attn = nn.MultiheadAttention(cfg.query_emb.hidden_size, cfg.query_emb.head_num, batch_first=True)
        codec = getattr(cfg, "codec", None)
        self.quantizer = Quantizer(getattr(codec, "n_q", 32), getattr(codec, "dim", 128), getattr(codec, "codebook_size", 1024))
        self._lin, self._q, self._kv, self._o = _PwHandle(), _RowsHandle(), _RowsHandle(), _PwHandle()

    @torch.no_grad()
    def code_to_latent(self, code):
        """code [B, n_q, T] -> latent [B, dim, T]"""
        return self.quantizer.decode(code.transpose(0, 1))

    def latent_to_code(self, latent, nq=16):
        raise NotImplementedError("NaturalSpeech2.latent_to_code is not on the HIP path")

    def forward(self, *args, **kwargs):
        raise NotImplementedError("NaturalSpeech2.forward is the training path: not on the HIP path (use .inference)")

    def reverse_diffusion_from_t(self, *args, **kwargs):
        raise NotImplementedError("NaturalSpeech2.reverse_diffusion_from_t (the reference's debugging entry) is not on the HIP path")

    def _speaker(self, ref_latent, key_mask):
        """ref_latent [B, latent, T'] -> (the prompt encoder's output [B, d, T'], the query tokens after their attention [B, d, Q])"""
        C, H = self.query_attn.embed_dim, self.query_attn.num_heads
        _check_mha(self.query_attn, "NaturalSpeech2.query_attn")
        B = ref_latent.shape[0]
        spk_emb = self.prompt_encoder.forward_cf(_pw(self._lin, self.prompt_lin, ref_latent), key_mask, None)
        q = _pw(self._q, mha_rows(self.query_attn, 0, 1), self.query_emb.weight.detach().t().contiguous()[None])       # [1, d, Q]: the same for every item
        kv = _pw(self._kv, mha_rows(self.query_attn, 1, 3), spk_emb)
        att = cross_attention(q.expand(B, -1, -1).contiguous(), kv[:, :C], kv[:, C:], H, key_mask)
        return spk_emb, _pw(self._o, self.query_attn.out_proj, att)

    @torch.no_grad()
    def inference(self, ref_code=None, phone_id=None, ref_mask=None, inference_steps=1000, *, ref_latent=None, noise=None):
        """ref_code [B, n_q, T'] (or ``ref_latent`` [B, latent, T'] in its place); phone_id [B, N]; ref_mask [B, T'], 0 = padded;
        ``noise``: a callable shape -> tensor that replaces ``torch.randn`` -> (x0 [B, latent, T], prior_out)"""
        if self.training:
            raise NotImplementedError("NaturalSpeech2.inference: call .eval() first (dropout is not on the HIP path)")
        if (ref_code is None) == (ref_latent is None):
            raise ValueError("NaturalSpeech2.inference: give ref_code or ref_latent, not both")
        if ref_mask is None or phone_id is None:
            raise ValueError("NaturalSpeech2.inference: phone_id and ref_mask are required")
        dev = self.prompt_lin.weight.device
        with _lib.on_device(dev):
            if ref_latent is None:
                ref_latent = self.code_to_latent(ref_code.to(dev))
            ref_latent = _lib.require_device_tensor(ref_latent, "NaturalSpeech2 prompt latent")
            key_mask = _key_mask(ref_mask.to(dev))
            if ref_latent.dim() != 3 or ref_latent.shape[1] != self.latent_dim or tuple(key_mask.shape) != (ref_latent.shape[0], ref_latent.shape[2]):
                raise ValueError(f"NaturalSpeech2.inference: expected a prompt latent [B, {self.latent_dim}, T'] and ref_mask [B, T'], got "
                                 f"{tuple(ref_latent.shape)} and {tuple(key_mask.shape)}")
            spk_emb, spk_query = self._speaker(ref_latent, key_mask)
            prior_out = self.prior_encoder.forward_cf(phone_id.to(dev), spk_emb, key_mask)
            cond = prior_out["prior_out"]                                     # [B, T, d]
            shape = (cond.shape[0], self.latent_dim, cond.shape[1])
            z = (torch.randn(*shape) if noise is None else noise(shape)).to(dev) / 1.20
            x0 = self.diffusion.reverse_diffusion(z, None, cond, inference_steps, spk_query.transpose(1, 2))
        return x0, prior_out
