from .token_encoder import TokenEmbedding  # noqa: F401
