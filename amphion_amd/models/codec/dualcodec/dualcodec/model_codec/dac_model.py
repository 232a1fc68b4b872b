"""DualCodec's DAC stacks (model_codec/dac_model.py:49-169) as drop-ins: same constructor arguments, module indices and ``state_dict`` keys
(``block.N...`` for the encoder, ``model.N...`` for the decoder; weight-normed or folded).  They compose the classes of
``amphion_codec/codec.py`` and differ from them only in argument names and in ``output_padding = 0`` of the decoder's ConvTranspose1d.

    Encoder   = CodecEncoder(d_model, up_ratios=strides, out_channels=d_latent)
    Decoder     first conv (k = 7)                            implicit-GEMM conv kernel (HipConv1d)
                per DecoderBlock: Snake -> ConvTranspose1d    ONE fused launch where built (csrc/tconv_f16x3.hip), else amp_snake -> transposed conv
                                  3 x ResidualUnit            amp_codec_unit_forward
                Snake -> last conv (k = 7) -> tanh            amp_snake, HipConv1d with tanh on store

``DAC`` (dac_model.py:172-413, eval mode) puts the residual quantizer of ``dac_quantize.py`` between them.  What ``encode`` does around the
quantizer -- crop the latent to the semantic latent's length, subtract it, add it back to z_q -- and what ``decode_from_codes`` adds after
``from_codes`` ride in the quantizer launches (``amp_fvq_encode_ex`` / ``amp_fvq_decode_add``), with the bits of the separate passes.
``distill=True`` (a training-time head) is refused.

After a forward the op-level f16x3 range flag is checked (``_lib.range_check``)."""
from __future__ import annotations

import math
from typing import List, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from amphion_amd import _lib
from amphion_amd.models.codec.amphion_codec import codec as _codec
from amphion_amd.models.codec.amphion_codec.codec import EncoderBlock, ResidualUnit, _check_channels  # noqa: F401
from amphion_amd.models.codec.amphion_codec.vocos import _check_tensors

from .dac_layers import Snake1d, WNConv1d
from .dac_quantize import ResidualVectorQuantize


class AttrDict(dict):
    """the result object of ``DAC.forward`` / ``DualCodec.forward``: a dict whose items read as attributes too"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name, value):
        self[name] = value


def pad_to_length(x, length, pad_value=0):
    """dac_model.py:33-46: right-pad or crop the last axis to `length`"""
    if length > x.shape[-1]:
        return F.pad(x, (0, length - x.shape[-1]), value=pad_value)
    return x[..., :length]


class Encoder(_codec.CodecEncoder):
    def __init__(self, d_model: int = 64, strides: list = [2, 4, 8, 8], d_latent: int = 64):
        super().__init__(d_model=d_model, up_ratios=list(strides), out_channels=d_latent, use_tanh=False)

    def forward(self, x):
        return super().forward(_check_channels(x, 1, "Encoder"))

    def reset_parameters(self):
        pass                                   # dac_model.py's Encoder keeps torch's default initialisation


class DecoderBlock(_codec.DecoderBlock):
    def __init__(self, input_dim: int = 16, output_dim: int = 8, stride: int = 1):
        super().__init__(input_dim, output_dim, stride, output_padding=0)


class Decoder(nn.Module):
    def __init__(self, input_channel, channels, rates, d_out: int = 1):
        super().__init__()
        layers = [WNConv1d(input_channel, channels, kernel_size=7, padding=3)]
        output_dim = channels
        for i, stride in enumerate(rates):
            input_dim = channels // 2 ** i
            output_dim = channels // 2 ** (i + 1)
            layers += [DecoderBlock(input_dim, output_dim, stride)]
        layers += [Snake1d(output_dim), WNConv1d(output_dim, d_out, kernel_size=7, padding=3, tanh=True), nn.Tanh()]
        self.model = nn.Sequential(*layers)    # nn.Tanh holds the reference's module index; the tanh itself is the last conv's store
        self.input_channel = input_channel
        self.n_blocks = len(rates)

    def forward(self, x):
        """x [B, input_channel, T] latent -> [B, d_out, T * prod(rates) (less what odd rates drop)] waveform"""
        x = _check_channels(x, self.input_channel, "Decoder")
        dev = x.device
        _check_tensors(self, dev, "Decoder")
        n = self.n_blocks
        with _lib.on_device(dev):
            h = self.model[0](x)
            for i in range(n):
                h = self.model[1 + i].run(h)
            h = self.model[2 + n](self.model[1 + n](h))
        _lib.range_check(dev)
        return h


class DAC(nn.Module):
    def __init__(self, encoder_dim: int = 64, encoder_rates: List[int] = [2, 4, 8, 8], latent_dim: int = None, decoder_dim: int = 1536,
                 decoder_rates: List[int] = [8, 8, 4, 2], n_codebooks: int = 9, codebook_size: int = 1024, codebook_dim: Union[int, list] = 8,
                 quantizer_dropout: bool = False, sample_rate: int = 44100, distill_projection_out_dim=1024, distill=False, convnext=True,
                 is_causal=False):
        super().__init__()
        if distill:
            raise NotImplementedError("DAC(distill=True) is not on the HIP path: the distillation head is a training-time branch "
                                      "(DualCodec builds its DAC with distill=False)")
        self.encoder_dim = encoder_dim
        self.encoder_rates = encoder_rates
        self.decoder_dim = decoder_dim
        self.decoder_rates = decoder_rates
        self.sample_rate = sample_rate
        if latent_dim is None:
            latent_dim = encoder_dim * (2 ** len(encoder_rates))
        self.latent_dim = latent_dim
        self.hop_length = int(math.prod(encoder_rates))
        self.encoder = Encoder(encoder_dim, encoder_rates, latent_dim)
        self.n_codebooks = n_codebooks
        self.codebook_size = codebook_size
        self.codebook_dim = codebook_dim
        self.quantizer = ResidualVectorQuantize(input_dim=latent_dim, n_codebooks=n_codebooks, codebook_size=codebook_size,
                                                codebook_dim=codebook_dim, quantizer_dropout=quantizer_dropout)
        self.decoder = Decoder(latent_dim, decoder_dim, decoder_rates)
        self.distill = False

    def preprocess(self, audio_data, sample_rate):
        if sample_rate is None:
            sample_rate = self.sample_rate
        assert sample_rate == self.sample_rate
        length = audio_data.shape[-1]
        right_pad = math.ceil(length / self.hop_length) * self.hop_length - length
        return F.pad(audio_data, (0, right_pad)) if right_pad else audio_data

    def _no_training(self, who):
        if self.training:
            raise NotImplementedError(f"DAC.{who}: training mode is not on the HIP path (the kernels have no backward): call .eval()")

    def encode_codes(self, audio_data, sample_rate=24000, n_quantizers: int = None, subtracted_latent=None):
        """``encode`` for a caller that keeps the codes only: -> codes [B, n, T] int64 (no z_q, latents or losses are formed)"""
        self._no_training("encode")
        z = self.encoder(self.preprocess(audio_data, sample_rate))
        codes, _, _, _ = self.quantizer.run_encode(z, n_quantizers, subtracted_latent, want_sum=False)
        _lib.range_check(z.device)
        return codes.transpose(0, 1).contiguous()

    def encode(self, audio_data, sample_rate=24000, n_quantizers: int = None, subtracted_latent=None):
        """-> (z [B, D, T], codes [B, n, T], latents [B, n * d, T], commitment_loss, codebook_loss, first_layer_quantized)"""
        self._no_training("encode")
        z = self.encoder(self.preprocess(audio_data, sample_rate))
        return self.quantizer(z, n_quantizers, possibly_no_quantizer=False, subtracted_latent=subtracted_latent)

    def decode_from_codes(self, acoustic_codes, semantic_latent):
        """acoustic_codes [B, n, T] or None (the semantic latent alone goes to the decoder); semantic_latent [B, D, T]"""
        self._no_training("decode_from_codes")
        z = semantic_latent if acoustic_codes is None else self.quantizer.run_decode(acoustic_codes, add=semantic_latent)
        return self.decoder(z)

    def forward(self, audio_data, sample_rate: int = None, n_quantizers: int = None, subtracted_latent=None, bypass_quantize=False,
                possibly_no_quantizer=False):
        self._no_training("forward")
        length = audio_data.shape[-1]
        if bypass_quantize:
            if subtracted_latent is None:
                raise ValueError("DAC.forward: bypass_quantize without a subtracted latent leaves nothing to decode")
            # the reference still runs its encoder here and drops the result; only its length check is kept
            frames = math.ceil(length / self.hop_length)
            assert frames - subtracted_latent.shape[-1] <= 2
            codes, latents, commitment_loss, codebook_loss, first = None, None, 0.0, 0.0, None
            z = subtracted_latent
        else:
            z, codes, latents, commitment_loss, codebook_loss, first = self.encode(audio_data, sample_rate, n_quantizers, subtracted_latent)
        x = pad_to_length(self.decoder(z), length)
        return AttrDict({"x": x, "z": z, "codes": codes, "latents": latents, "penalty": commitment_loss, "vq/codebook_loss": codebook_loss,
                         "metrics": {}, "first_layer_quantized": first})
