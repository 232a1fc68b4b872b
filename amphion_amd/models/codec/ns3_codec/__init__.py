"""FACodec, NaturalSpeech 3's factorized codec (models/codec/ns3_codec): the encoder, the three-group factorized quantizer, the timbre path and
the decoder on the gfx950 kernels.  Eval mode only."""
from .facodec import FACodecDecoder, FACodecEncoder  # noqa: F401
