"""Coco, VevoSing's content / style tokenizers (models/codec/coco), on the gfx950 kernels.  Eval mode only."""
from .rep_coco_model import CocoContent, CocoContentStyle, CocoStyle  # noqa: F401
