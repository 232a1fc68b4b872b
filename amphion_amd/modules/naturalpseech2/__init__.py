"""modules/naturalpseech2 (the reference spells it so) on the HIP kernels: the encoders and predictors of NaturalSpeech2."""
from .transformers import (DurationPredictor, LengthRegulator, PitchPredictor, PositionalEncoding, StyleAdaptiveLayerNorm,  # noqa: F401
                           TransformerEncoder, TransformerEncoderLayer, TransformerFFNLayer)
