"""RepCodec, the semantic tokenizer of MaskGCT, Metis and Vevo (models/codec/kmeans), on the gfx950 kernels.  Eval mode only."""
from .repcodec_model import RepCodec  # noqa: F401
