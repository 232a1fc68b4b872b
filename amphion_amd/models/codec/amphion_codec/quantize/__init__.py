from amphion_amd.models.codec.amphion_codec.quantize.factorized_vector_quantize import FactorizedVectorQuantize
from amphion_amd.models.codec.amphion_codec.quantize.residual_vq import ResidualVQ

__all__ = ["FactorizedVectorQuantize", "ResidualVQ"]
