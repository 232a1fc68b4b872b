"""VALL-E zero-shot TTS inference on the HIP kernels (models/tts/valle)."""
from .valle import VALLE  # noqa: F401
