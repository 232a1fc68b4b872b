"""Residual vector quantizer of SpeechTokenizer (models/codec/speechtokenizer/modules/quantization) on the exact-fp32 kernels of csrc/evq.hip."""
# flake8: noqa
from .core_vq import EuclideanCodebook, ResidualVectorQuantization, VectorQuantization
from .vq import ResidualVectorQuantizer
