"""FACodec, NaturalSpeech 3's factorized codec (models/codec/ns3_codec): the encoder, the three-group factorized quantizer, the timbre path and
the decoder on the gfx950 kernels, and the zero-shot voice-conversion classes (FACodecEncoderV2, FACodecDecoderV2, FACodecRedecoder).  Eval mode
only."""
from .facodec import FACodecDecoder, FACodecDecoderV2, FACodecEncoder, FACodecEncoderV2, FACodecRedecoder  # noqa: F401
from .melspec import MelSpectrogram  # noqa: F401
