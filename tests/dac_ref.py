"""fp64 / fp32 torch restatement of the DAC-style decoder stacks (DualCodec model_codec/dac_model.py:119-169; the ``output_padding`` form of
models/codec/amphion_codec/codec.py:146-165), computed from a state_dict, with key / shape lists, seeded synthetic state_dicts and the derived
bound of the fused Snake -> ConvTranspose1d op.

The decoder has its OWN draw: codec_ref._synth makes unit-gain layers, under which the decoder's residual stream grows block by block and its
final tanh saturates on most samples -- the fp32 restatement's own error then reaches 3.5e-4 and hides everything.  synth_decoder_state_dict
scales the weight_g of every unit's 1 x 1 conv and of the last conv by 0.25: no sample beyond 0.99, rms 0.1 - 0.3, fp32 error <= 1e-6."""
from __future__ import annotations

import torch
import torch.nn.functional as Fn

import codec_ref as C


# ---- hyperparameters -------------------------------------------------------------------------------------------------------------
def recipe_decoder_hp():
    """conf/model/dualcodec_25hz_16384_1024_12vq.yaml: latent 1024 there; the tests use a narrower latent in front of the same stack"""
    return dict(input_channel=256, channels=1536, rates=[8, 6, 5, 4], d_out=1)


def small_decoder_hp():
    return dict(input_channel=64, channels=256, rates=[2, 3, 5], d_out=1)


def even_decoder_hp():
    return dict(input_channel=64, channels=128, rates=[4, 8], d_out=1)


def small_dac_encoder_hp():
    return dict(d_model=32, strides=[2, 3], d_latent=64)


# ---- state_dict layouts -----------------------------------------------------------------------------------------------------------
def _wnT(s, prefix, cin, cout, k):
    """weight_norm(ConvTranspose1d): the norm is over dim 0 = the INPUT channels"""
    s[prefix + "bias"] = (cout,)
    s[prefix + "weight_g"] = (cin, 1, 1)
    s[prefix + "weight_v"] = (cin, cout, k)


def decoder_block_shapes(cin, cout, stride, prefix="block."):
    s = {prefix + "0.alpha": (1, cin, 1)}
    _wnT(s, prefix + "1.", cin, cout, 2 * stride)
    for u in range(3):
        p = f"{prefix}{2 + u}.block."
        s[p + "0.alpha"] = (1, cout, 1)
        C._wn(s, p + "1.", cout, cout, 7)
        s[p + "2.alpha"] = (1, cout, 1)
        C._wn(s, p + "3.", cout, cout, 1)
    return s


def decoder_param_shapes(hp):
    """state_dict key -> shape of Decoder(input_channel, channels, rates, d_out), in the reference's order (weight-normed form)"""
    s = {}
    ch = hp["channels"]
    C._wn(s, "model.0.", ch, hp["input_channel"], 7)
    out = ch
    for i, stride in enumerate(hp["rates"]):
        cin, out = ch // 2 ** i, ch // 2 ** (i + 1)
        s.update(decoder_block_shapes(cin, out, stride, f"model.{1 + i}.block."))
    n = len(hp["rates"])
    s[f"model.{1 + n}.alpha"] = (1, out, 1)
    C._wn(s, f"model.{2 + n}.", hp["d_out"], out, 7)
    return s


def dac_encoder_param_shapes(hp):
    return C.encoder_param_shapes(dict(d_model=hp["d_model"], up_ratios=hp["strides"], out_channels=hp["d_latent"]))


def _calm(sd, last=None):
    """the decoder's draw: weight_g of every unit's 1 x 1 conv (...block.{2,3,4}.block.3.weight_g) and of the last conv x 0.25"""
    out = {}
    for k, v in sd.items():
        parts = k.split(".")
        unit_1x1 = k.endswith(".block.3.weight_g") and len(parts) >= 5 and parts[-5] == "block" and parts[-4] in ("2", "3", "4")
        out[k] = v * 0.25 if unit_1x1 or (last is not None and k == last + "weight_g") else v
    return out


def synth_decoder_state_dict(hp, seed):
    return _calm(C._synth(decoder_param_shapes(hp), seed), last=f"model.{2 + len(hp['rates'])}.")


def synth_block_state_dict(cin, cout, stride, seed):
    return _calm(C._synth(decoder_block_shapes(cin, cout, stride), seed))


def synth_dac_encoder_state_dict(hp, seed):
    return C._synth(dac_encoder_param_shapes(hp), seed)


def fold_state_dict(sd):
    """the same weights with weight-norm removed: `weight` in place of weight_g / weight_v"""
    out = {}
    for k, v in sd.items():
        if k.endswith("weight_g"):
            out[k[:-2]] = C.folded(sd, k[:-8])
        elif not k.endswith("weight_v"):
            out[k] = v
    return out


# ---- the forward passes -----------------------------------------------------------------------------------------------------------
def block_padding(stride):
    return stride // 2 + stride % 2


def tconv(P, p_alpha, p_conv, x, stride, output_padding=0, padding=None):
    """[Snake1d ->] ConvTranspose1d(k = 2 stride, stride, padding, output_padding)"""
    if p_alpha is not None:
        x = C.snake(x, P[p_alpha])
    padding = block_padding(stride) if padding is None else padding
    return Fn.conv_transpose1d(x, C.folded(P, p_conv), P[p_conv + "bias"], stride=stride, padding=padding, output_padding=output_padding)


def decoder_block_forward(P, prefix, x, stride, output_padding=0):
    h = tconv(P, prefix + "0.alpha", prefix + "1.", x, stride, output_padding)
    for u, dil in enumerate((1, 3, 9)):
        h = C.residual_unit(P, f"{prefix}{2 + u}.block.", h, dil)
    return h


def decoder_forward(sd, hp, x, dtype=torch.float64, pre_tanh=False, output_padding=False):
    """Decoder.forward; output_padding=True: the Amphion form of the blocks (output_padding = stride % 2)"""
    P = {k: v.to(dtype) for k, v in sd.items()}
    h = Fn.conv1d(x.to(dtype), C.folded(P, "model.0."), P["model.0.bias"], padding=3)
    for i, stride in enumerate(hp["rates"]):
        h = decoder_block_forward(P, f"model.{1 + i}.block.", h, stride, stride % 2 if output_padding else 0)
    n = len(hp["rates"])
    h = Fn.conv1d(C.snake(h, P[f"model.{1 + n}.alpha"]), C.folded(P, f"model.{2 + n}."), P[f"model.{2 + n}.bias"], padding=3)
    return h if pre_tanh else torch.tanh(h)


def tconv_out_len(T, stride, padding, output_padding):
    return (T - 1) * stride - 2 * padding + 2 * stride + output_padding


# ---- the fused op's bound ---------------------------------------------------------------------------------------------------------
def d_snake(v, a):
    """tests/test_gpu_codec.py: error of the library's snake on an exact fp32 argument"""
    return (3.3e-7 + 1.2e-7 * (a * v).abs()) / a + 2.4e-7 * C.snake(v, a).abs()


def tconv_bound(w, b, alpha, x, stride, padding, output_padding):
    """fp64 output of [snake ->] conv_transpose1d and the derived bound of each element: the strided-conv op's bound of tests/test_gpu_codec.py
    with conv_transpose1d in place of conv1d:  2e-6 (|w| * |snake(x)| + |b|) + 3e-7 |ref| + |w| * d_snake(x)"""
    kw = dict(stride=stride, padding=padding, output_padding=output_padding)
    s1 = x if alpha is None else C.snake(x, alpha)
    ref = Fn.conv_transpose1d(s1, w, b, **kw)
    tol = 2e-6 * (Fn.conv_transpose1d(s1.abs(), w.abs(), **kw) + b.abs()[None, :, None]) + 3e-7 * ref.abs()
    if alpha is not None:
        tol = tol + Fn.conv_transpose1d(d_snake(x, alpha), w.abs(), **kw)
    return ref, tol
