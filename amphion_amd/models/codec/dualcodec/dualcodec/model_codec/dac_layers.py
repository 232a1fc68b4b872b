"""model_codec/dac_layers.py on the gfx950 kernels: the Snake activation and the weight-normed conv holders, under the reference's names."""
from __future__ import annotations

from amphion_amd.models.codec.amphion_codec.codec import Snake1d, _TransposedConv, snake  # noqa: F401
from amphion_amd.modules.hip_ops import HipConv1d


def _take(args, kwargs, names):
    """nn.Conv1d's leading arguments, positional or by keyword, in torch's order"""
    vals = dict(zip(names, args))
    for n in names[len(args):]:
        if n in kwargs:
            vals[n] = kwargs.pop(n)
    if len(args) > len(names):
        raise TypeError(f"at most {len(names)} positional arguments")
    return vals


def WNConv1d(*args, **kwargs):
    """weight_norm(nn.Conv1d(in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1)) as a ``HipConv1d``; ``tanh=True``
    applies tanh on store.  A strided conv is not this holder's: EncoderBlock builds its own."""
    v = _take(args, kwargs, ("in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation"))
    if v.get("stride", 1) != 1:
        raise NotImplementedError("WNConv1d with stride != 1 is not on the HIP path outside EncoderBlock")
    return HipConv1d(v["in_channels"], v["out_channels"], v["kernel_size"], dilation=v.get("dilation", 1), padding=v.get("padding", 0), **kwargs)


def WNConvTranspose1d(*args, **kwargs):
    """weight_norm(nn.ConvTranspose1d(in_channels, out_channels, kernel_size = 2 * stride, stride, padding, output_padding)) as the decoder
    blocks' up-sampling holder; ``forward(x, alpha=None)`` applies Snake first when ``alpha`` is given."""
    v = _take(args, kwargs, ("in_channels", "out_channels", "kernel_size", "stride", "padding", "output_padding"))
    stride = v.get("stride", 1)
    if kwargs:
        raise NotImplementedError(f"WNConvTranspose1d: {sorted(kwargs)} not on the HIP path")
    if v["kernel_size"] != 2 * stride:
        raise NotImplementedError(f"WNConvTranspose1d: kernel_size {v['kernel_size']} != 2 * stride {stride} is not on the HIP path")
    return _TransposedConv(v["in_channels"], v["out_channels"], stride, v.get("padding", 0), v.get("output_padding", 0))
