"""VevoRepCodec, Vevo's content tokenizer over HuBERT features (models/codec/vevo), on the gfx950 kernels.  Eval mode only."""
from .vevo_repcodec import VevoRepCodec  # noqa: F401
