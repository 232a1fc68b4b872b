"""fp64 restatement of the reference Vocos forward (models/codec/amphion_codec/vocos.py:84-167,319-359,470-526,720-783,824-881),
computed from a state_dict, plus the shapes, hyperparameters and a seeded synthetic state_dict for the tests.

The ISTFT is the reference's own form: irfft, fold (overlap-add), fold of window^2 (the envelope), crop (win - hop) / 2 per side.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as Fn


def recipe_hp():
    """egs/vocoder/vocos/emilia_singnet.json (model.vocos; the same net: models/svc/vevosing/config/vocoder.json:17-25)"""
    return dict(input_channels=128, dim=1024, intermediate_dim=4096, num_layers=30, n_fft=1920, hop_size=480, padding="same")


def maskgct_decoder_hp():
    """the MaskGCT acoustic codec decoder's Vocos (models/codec/amphion_codec/codec.py:372-382, sizes from
    models/tts/maskgct/config/maskgct.json:71-77)"""
    return dict(input_channels=256, dim=512, intermediate_dim=4096, num_layers=30, n_fft=1920, hop_size=480, padding="same")


def class_default_hp():
    """Vocos.__init__'s defaults (vocos.py:824-835)"""
    return dict(input_channels=256, dim=384, intermediate_dim=1152, num_layers=8, n_fft=800, hop_size=200, padding="same")


def small_hp(n_fft=256, hop=64):
    """the golden nets (tests/golden/make_golden_vocos.py): small enough for a fixture of tens of KB"""
    return dict(input_channels=24, dim=64, intermediate_dim=192, num_layers=3, n_fft=n_fft, hop_size=hop, padding="same")


def vocos_param_shapes(hp):
    """state_dict key -> shape, in the reference's order"""
    C, I, L = hp["dim"], hp["intermediate_dim"], hp["num_layers"]
    s = {"backbone.embed.weight": (C, hp["input_channels"], 7), "backbone.embed.bias": (C,),
         "backbone.norm.weight": (C,), "backbone.norm.bias": (C,)}
    for i in range(L):
        p = f"backbone.convnext.{i}."
        s[p + "gamma"] = (C,)
        s[p + "dwconv.weight"] = (C, 1, 7)
        s[p + "dwconv.bias"] = (C,)
        s[p + "norm.weight"] = (C,)
        s[p + "norm.bias"] = (C,)
        s[p + "pwconv1.weight"] = (I, C)
        s[p + "pwconv1.bias"] = (I,)
        s[p + "pwconv2.weight"] = (C, I)
        s[p + "pwconv2.bias"] = (C,)
    s["backbone.final_layer_norm.weight"] = (C,)
    s["backbone.final_layer_norm.bias"] = (C,)
    s["head.out.weight"] = (hp["n_fft"] + 2, C)
    s["head.out.bias"] = (hp["n_fft"] + 2,)
    s["head.istft.window"] = (hp["n_fft"],)
    return s


def synth_vocos_state_dict(hp, seed):
    """Realistic scales: layer scale ~ 1/num_layers, LayerNorm weights 1 + N(0, 0.1), fan-in scaled Linear / conv weights; the
    head's log-magnitude rows put most values in [-6, 3] with a few bins above ln 100 (the clip), phases spread over a few
    radians up to ~|30|.  (oracle.synth's name heuristics would take the layer-scale gamma for a LayerNorm weight.)"""
    g = torch.Generator().manual_seed(seed)
    C, I, L, nf = hp["dim"], hp["intermediate_dim"], hp["num_layers"], hp["n_fft"]
    bins = nf // 2 + 1

    def n(*shape, std=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * std

    sd = {}
    for k, shp in vocos_param_shapes(hp).items():
        if k == "head.istft.window":
            sd[k] = torch.hann_window(nf, dtype=torch.float32)
        elif k.endswith("gamma"):
            sd[k] = (1.0 / L) * (1 + n(*shp, std=0.2))
        elif k.endswith("norm.weight") or k.endswith("final_layer_norm.weight"):
            sd[k] = 1 + n(*shp, std=0.1)
        elif k.endswith("norm.bias") or k.endswith("final_layer_norm.bias"):
            sd[k] = n(*shp, std=0.05)
        elif k == "backbone.embed.weight":
            sd[k] = n(*shp, std=1.0 / math.sqrt(shp[1] * 7))
        elif k.endswith("dwconv.weight"):
            sd[k] = n(*shp, std=1.0 / math.sqrt(7))
        elif k.endswith("pwconv1.weight") or k.endswith("pwconv2.weight"):
            sd[k] = n(*shp, std=1.0 / math.sqrt(shp[1]))
        elif k == "head.out.weight":
            w = n(*shp, std=1.0 / math.sqrt(shp[1]))
            w[:bins] *= 1.2              # log-magnitude rows: ~N(bias, 1.2) after the final LayerNorm
            w[bins:] *= 6.0              # phase rows
            sd[k] = w
        elif k == "head.out.bias":
            b = torch.zeros(shp, dtype=torch.float64)
            b[:bins] = -1.5 + n(bins, std=1.0)
            hot = torch.randperm(bins, generator=g)[: max(2, bins // 64)]
            b[hot] = 5.5                 # a few bins beyond ln 100 = 4.6: exercises the clip
            b[bins:] = n(bins, std=8.0)
            sd[k] = b
        else:                            # conv / Linear biases
            sd[k] = n(*shp, std=0.05)
    return {k: v.float().contiguous() for k, v in sd.items()}


def synth_features(B, C, F, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, C, F, generator=g) * scale).float()


def _ln_c(x, w, b, eps=1e-6):
    """LayerNorm over the channel axis of [B, C, T]"""
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w[None, :, None] + b[None, :, None]


def istft_same(spec, n_fft, hop, window):
    """vocos.py:138-167 on a complex [B, n_fft/2+1, F] spectrogram (fp64)"""
    B, N, T = spec.shape
    win = n_fft
    pad = (win - hop) // 2
    ifft = torch.fft.irfft(spec, n_fft, dim=1, norm="backward") * window[None, :, None]
    size = (T - 1) * hop + win
    y = Fn.fold(ifft, output_size=(1, size), kernel_size=(1, win), stride=(1, hop))[:, 0, 0, pad:-pad]
    wsq = window.square().expand(1, T, -1).transpose(1, 2)
    env = Fn.fold(wsq, output_size=(1, size), kernel_size=(1, win), stride=(1, hop)).squeeze()[pad:-pad]
    assert (env > 1e-11).all()
    return y / env


def head_spec(h, n_fft, clip=1e2):
    """ISTFTHead's polar step (vocos.py:346-359) on the Linear output [B, n_fft + 2, F] -> complex spectrogram"""
    mag, p = h.chunk(2, dim=1)
    mag = torch.clip(torch.exp(mag), max=clip)
    return mag * (torch.cos(p) + 1j * torch.sin(p))


def vocos_forward(sd, hp, x, dtype=torch.float64, return_head=False):
    """x [B, C_in, F] -> [B, 1, F * hop] in `dtype` (fp64: the oracle; fp32: the torch restatement the tests compare against)"""
    P = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    C = hp["dim"]
    h = Fn.conv1d(x, P["backbone.embed.weight"], P["backbone.embed.bias"], padding=3)
    h = _ln_c(h, P["backbone.norm.weight"], P["backbone.norm.bias"])
    for i in range(hp["num_layers"]):
        p = f"backbone.convnext.{i}."
        r = h
        y = Fn.conv1d(h, P[p + "dwconv.weight"], P[p + "dwconv.bias"], padding=3, groups=C)
        y = _ln_c(y, P[p + "norm.weight"], P[p + "norm.bias"])
        y = torch.einsum("oc,bct->bot", P[p + "pwconv1.weight"], y) + P[p + "pwconv1.bias"][None, :, None]
        y = Fn.gelu(y)
        y = torch.einsum("oc,bct->bot", P[p + "pwconv2.weight"], y) + P[p + "pwconv2.bias"][None, :, None]
        h = r + P[p + "gamma"][None, :, None] * y
    h = _ln_c(h, P["backbone.final_layer_norm.weight"], P["backbone.final_layer_norm.bias"])
    head = torch.einsum("oc,bct->bot", P["head.out.weight"], h) + P["head.out.bias"][None, :, None]
    wav = istft_same(head_spec(head, hp["n_fft"]), hp["n_fft"], hp["hop_size"], P["head.istft.window"])[:, None, :]
    return (wav, head) if return_head else wav
