"""DualCodec's DAC stacks (model_codec/dac_model.py:49-169) as drop-ins: same constructor arguments, module indices and ``state_dict`` keys
(``block.N...`` for the encoder, ``model.N...`` for the decoder; weight-normed or folded).  They compose the classes of
``amphion_codec/codec.py`` and differ from them only in argument names and in ``output_padding = 0`` of the decoder's ConvTranspose1d.

    Encoder   = CodecEncoder(d_model, up_ratios=strides, out_channels=d_latent)
    Decoder     first conv (k = 7)                            implicit-GEMM conv kernel (HipConv1d)
                per DecoderBlock: Snake -> ConvTranspose1d    ONE fused launch where built (csrc/tconv_f16x3.hip), else amp_snake -> transposed conv
                                  3 x ResidualUnit            amp_codec_unit_forward
                Snake -> last conv (k = 7) -> tanh            amp_snake, HipConv1d with tanh on store

After a forward the op-level f16x3 range flag is checked (``_lib.range_check``)."""
from __future__ import annotations

import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.codec.amphion_codec import codec as _codec
from amphion_amd.models.codec.amphion_codec.codec import EncoderBlock, ResidualUnit, _check_channels  # noqa: F401
from amphion_amd.models.codec.amphion_codec.vocos import _check_tensors

from .dac_layers import Snake1d, WNConv1d


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
