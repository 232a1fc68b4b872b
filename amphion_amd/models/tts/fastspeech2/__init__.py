"""FastSpeech2 text -> mel inference on the HIP kernels (models/tts/fastspeech2/fs2.py)."""
from .fs2 import FastSpeech2, LengthRegulator, VarianceAdaptor, VariancePredictor, get_mask_from_lengths  # noqa: F401
