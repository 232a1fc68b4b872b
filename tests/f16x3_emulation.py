"""CPU emulation of the split-f16 contraction of the f16x3 conv kernels (conv_f16x3.hip and the forms that share its arithmetic).

The kernels stage an activation as hi + lo f16 after an exact x16 (f16x3_device.h: split_f16, stage4_f16; leaky ReLU on load is
max(16 x, 16 slope x)), pack each weight as hi + lo f16 after a power-of-two scale that puts max|w| in (2^12, 2^13]
(amp_host.h: pow2_weight_scale, pack_a_f16x3), and accumulate three MFMA products in fp32: W_hi X_hi + W_hi X_lo + W_lo X_hi.  W_lo X_lo is dropped.
Each f16 x f16 product is exact in fp32, so fp32 convolutions of the hi / lo parts emulate the products exactly and the
accumulation's rounding roughly (the order of the sums differs from the MFMA's).

`terms` selects the ablation: 3 the kernels' arithmetic; "no_wh_xlo" drops W_hi X_lo (activations rounded to one f16);
"no_wlo_xhi" drops W_lo X_hi (weights rounded to one f16).  A kernel that lost one correction term computes the latter two.
"""
import math

import torch
import torch.nn.functional as F

XS = 16.0
_conv1d, _conv_transpose1d = F.conv1d, F.conv_transpose1d     # bound at import: a caller may patch F.* with this emulation
TERMS = (3, "no_wh_xlo", "no_wlo_xhi")


def weight_scale(w):
    """conv_build: 2^s with max|w| * 2^s in (2^12, 2^13]"""
    m = w.abs().max().item()
    if m == 0.0:
        return 1.0
    mant, e2 = math.frexp(m)                    # m = mant * 2^e2, mant in [0.5, 1): m <= 2^e2
    if mant == 0.5:
        e2 -= 1
    return 2.0 ** (13 - e2)


def split(v):
    """fp32 v -> (hi, lo) f16 parts as fp32 tensors: hi = f16(v), lo = f16(v - hi)"""
    v = v.float()
    hi = v.half().float()
    return hi, (v - hi).half().float()


def conv(x, w, b=None, *, transposed=False, stride=1, dilation=1, padding=0, slope_in=1.0, res=None, slope_out=1.0, terms=3,
         output_padding=0):
    """y = lrelu(conv(lrelu(x, slope_in), w) + b + res, slope_out) in the kernels' split-f16 arithmetic (fp32 in and out);
    output_padding: ConvTranspose1d's (transposed only)"""
    xl = x.float() * XS
    if slope_in != 1.0:
        xl = torch.maximum(xl, xl * slope_in)
    S = weight_scale(w)
    xh, xlo = split(xl)
    wh, wlo = split(w.float() * S)
    if transposed:
        op = lambda a, ww: _conv_transpose1d(a, ww, stride=stride, padding=padding, output_padding=output_padding)
    else:
        op = lambda a, ww: _conv1d(a, ww, dilation=dilation, padding=padding)
    acc = op(xh, wh)
    if terms in (3, "no_wlo_xhi"):
        acc = acc + op(xlo, wh)
    if terms in (3, "no_wh_xlo"):
        acc = acc + op(xh, wlo)
    y = acc * (1.0 / (XS * S))
    if b is not None:
        y = y + b.float().view(1, -1, 1)
    if res is not None:
        y = y + res.float()
    return torch.where(y >= 0, y, y * slope_out) if slope_out != 1.0 else y
