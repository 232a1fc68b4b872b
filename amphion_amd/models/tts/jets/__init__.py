"""JETS text -> wave inference on the HIP kernels (models/tts/jets/jets.py)."""
from .jets import Jets  # noqa: F401
