"""MaskGCT (models/tts/maskgct): the text-to-semantic and semantic-to-acoustic models and their two estimators, eval mode, on the gfx950
kernels.  Same class names, constructor arguments and ``state_dict`` keys as the reference."""
from .llama_nar import DiffLlama, DiffLlamaPrefix  # noqa: F401
from .maskgct_s2a import MaskGCT_S2A  # noqa: F401
from .maskgct_t2s import MaskGCT_T2S  # noqa: F401
