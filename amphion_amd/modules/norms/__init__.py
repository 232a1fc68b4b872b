from .norm import AdaptiveLayerNorm, LayerNorm  # noqa: F401
