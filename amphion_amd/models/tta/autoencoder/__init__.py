"""AudioLDM's AutoencoderKL (models/tta/autoencoder): the decoder that turns latents into a mel."""
from .autoencoder import AutoencoderKL, Decoder2d, ResnetBlock, Upsample2d  # noqa: F401
