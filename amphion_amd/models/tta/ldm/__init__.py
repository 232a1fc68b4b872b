"""AudioLDM's latent diffusion model (models/tta/ldm): the UNet, its spatial transformer and the sampling loop."""
from .attention import BasicTransformerBlock, CrossAttention, FeedForward, GEGLU, SpatialTransformer  # noqa: F401
from .audioldm import AudioLDM, Downsample, ResBlock, TimestepEmbedSequential, UNetModel, Upsample, timestep_embedding  # noqa: F401
from .audioldm_inference import generate_latents, text_to_mel  # noqa: F401
