"""Vevo's flow-matching transformer (models/vc/flow_matching_transformer): content-style codes plus a timbre-prompt mel -> the target mel, on
the gfx950 kernels.  Eval mode only."""
from .fmt_model import FlowMatchingTransformer  # noqa: F401
from .llama_nar import DiffLlama, LlamaAdaptiveRMSNorm, SinusoidalPosEmb  # noqa: F401
