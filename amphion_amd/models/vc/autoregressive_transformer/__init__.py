"""Vevo's autoregressive transformer (models/vc/autoregressive_transformer): content or phone tokens plus a content-style prompt -> content-style
tokens, a causal Llama with a KV cache on the gfx950 kernels.  Eval mode only."""
from .ar_model import AutoregressiveTransformer, LlamaRMSNorm  # noqa: F401
