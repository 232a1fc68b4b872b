"""fp64 predictor of the f16x3 range guard: the largest |operand| each conv of an op stages.

The f16x3 kernels stage every conv operand as hi + lo f16 after an exact x16 (f16x3_device.h: stage4_f16, seam4_f16; the
Activation1d outputs of ampb_f16x3.hip): |x| <= 4094 fits (x16 = 65504, the largest finite f16), anything beyond, and any
infinity, raises the range flag.  A NaN operand is not flagged (it reaches the output as it does through the reference).
The operand of a conv is what the kernel stages, not what the layer receives: the value AFTER the on-load leaky ReLU, the
leaky-ReLU'd seam between the two convs of a fused pair, or the output of Activation1d in BigVGAN's AMPBlock1.  Outputs,
residuals and the running MRF sum are fp32 in every kernel and never staged.

Each ``*_ops`` function returns ``(y, maxima)``: the op's output in fp64 and one max |staged operand| per conv, in launch order.
``flagged(maxima)`` is the guard's decision; ``margin(maxima)`` how far the op sits from that decision (tests keep >= 1.5)."""
import torch
import torch.nn.functional as F

THRESHOLD = 4094.0     # 65504 / 16 (4094 x 16 = 65504 exactly)


def lrelu(x, slope):
    return torch.where(x > 0, x, x * slope) if slope != 1.0 else x


def staged_max(t):
    """max |t| over the non-NaN entries (NaN is not the guard's business); 0 for an all-NaN tensor"""
    a = t.detach().double().abs()
    a = a[~torch.isnan(a)]
    return a.max().item() if a.numel() else 0.0


def flagged(maxima):
    return any(m > THRESHOLD for m in maxima)       # inf > 4094 too


def margin(maxima):
    """factor between the decisive operand and the threshold: >= 1 on the side the op is on (inf: infinite)"""
    m = max(maxima)
    if m > THRESHOLD:
        return m / THRESHOLD
    return THRESHOLD / m if m > 0 else float("inf")


def conv_ops(x, w, b, *, padding, dilation=1, slope_in=1.0, res=None, transposed=False, stride=1):
    x = x.double()
    a = lrelu(x, slope_in)
    bb = b.double() if b is not None else None
    if transposed:
        y = F.conv_transpose1d(a, w.double(), bb, stride=stride, padding=padding)
    else:
        y = F.conv1d(a, w.double(), bb, padding=padding, dilation=dilation)
    if res is not None:
        y = y + res.double()
    return y, [staged_max(a)]


def pair_ops(x, w1, b1, w2, b2, *, dilation, slope=0.1):
    """y = x + c2(lrelu(c1(lrelu(x)))): operands lrelu(x) and the seam lrelu(c1(.))"""
    k = w1.shape[2]
    x = x.double()
    a = lrelu(x, slope)
    s = lrelu(F.conv1d(a, w1.double(), b1.double(), dilation=dilation, padding=(k * dilation - dilation) // 2), slope)
    y = x + F.conv1d(s, w2.double(), b2.double(), padding=(k - 1) // 2)
    return y, [staged_max(a), staged_max(s)]


def resblock_ops(x, ws1, bs1, ws2, bs2, *, dilations, slope=0.1):
    """ResBlock1: the pairs in sequence, each one's input the previous one's output (rb_f16x3.hip keeps it in registers)"""
    maxima = []
    for w1, b1, w2, b2, d in zip(ws1, bs1, ws2, bs2, dilations):
        x, m = pair_ops(x, w1, b1, w2, b2, dilation=d, slope=slope)
        maxima += m
    return x, maxima


def ampblock_ops(x, ws1, bs1, ws2, bs2, alphas, betas, logscale, *, dilations):
    """AMPBlock1 (bigvgan.py:137-146): every conv stages its Activation1d output (betas None: Snake)"""
    from oracle import vocoder_oracle as vo

    x = x.double()
    maxima = []
    for i, (w1, b1, w2, b2, d) in enumerate(zip(ws1, bs1, ws2, bs2, dilations)):
        k = w1.shape[2]
        be = lambda j: betas[j].double() if betas is not None else None
        a = vo.activation1d(x, alphas[2 * i].double(), be(2 * i), logscale)
        xt = F.conv1d(a, w1.double(), b1.double(), dilation=d, padding=(k * d - d) // 2)
        a2 = vo.activation1d(xt, alphas[2 * i + 1].double(), be(2 * i + 1), logscale)
        maxima += [staged_max(a), staged_max(a2)]
        x = x + F.conv1d(a2, w2.double(), b2.double(), padding=(k - 1) // 2)
    return x, maxima


def nonfinite_equal(y, ref, *, nan=False):
    """the positions of the non-finite values agree (nan=True: and those of the NaNs -- an infinite operand becomes NaN in
    the split form, hi = inf, lo = inf - inf, where the reference may keep +-inf, so only the non-finite set is compared there)"""
    y, ref = y.double(), ref.double()
    same = torch.equal(~torch.isfinite(y), ~torch.isfinite(ref))
    return same and (not nan or torch.equal(torch.isnan(y), torch.isnan(ref)))
