"""SEANet building blocks of SpeechTokenizer (models/codec/speechtokenizer/modules) on the gfx950 kernels."""
# flake8: noqa
from .conv import SConv1d, SConvTranspose1d, elu_pad, get_extra_padding_for_conv1d
from .lstm import SLSTM
from .seanet import SEANetDecoder, SEANetEncoder, SEANetResnetBlock
