"""DualCodec (models/codec/dualcodec/dualcodec/model_codec/) in eval mode on the gfx950 kernels: the DAC encoder / decoder stacks, the DAC
residual quantizer, the (causal) ConvNeXt block, and the ``DAC`` and ``DualCodec`` models with ``encode`` / ``decode_from_codes``.  Not here:
``get_model`` and the hydra configs, checkpoint download, w2v-BERT itself, resampling and the TTS models under ``model_tts/``."""
from .cnn import ConvNeXtBlock  # noqa: F401
from .dac_model import DAC, AttrDict, Decoder, DecoderBlock, Encoder, EncoderBlock, ResidualUnit  # noqa: F401
from .dac_quantize import ResidualVectorQuantize, VectorQuantize  # noqa: F401
from .dualcodec_model import DualCodec, prepare_semantic_features  # noqa: F401
