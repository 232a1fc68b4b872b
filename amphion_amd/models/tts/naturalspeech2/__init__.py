"""NaturalSpeech2 zero-shot TTS inference on the HIP kernels (models/tts/naturalspeech2)."""
from .diffusion import Diffusion  # noqa: F401
from .diffusion_flow import DiffusionFlow  # noqa: F401
from .ns2 import NaturalSpeech2  # noqa: F401
from .prior_encoder import PriorEncoder  # noqa: F401
from .wavenet import WaveNet  # noqa: F401
