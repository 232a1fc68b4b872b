"""DualCodec's DAC encoder / decoder stacks (models/codec/dualcodec/dualcodec/model_codec/dac_model.py:49-169) on the gfx950 kernels.  The DAC and
DualCodec model classes, their quantizers and the semantic branch are not on the HIP path."""
from .dac_model import Decoder, DecoderBlock, Encoder, EncoderBlock, ResidualUnit  # noqa: F401
