"""SpeechTokenizer (models/codec/speechtokenizer): SEANet encoder / decoder with their LSTM stacks and the Euclidean residual quantizer on the
gfx950 kernels.  Eval mode only."""
from .model import SpeechTokenizer  # noqa: F401
