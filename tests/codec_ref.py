"""fp64 / fp32 torch restatement of the Amphion acoustic codec (models/codec/amphion_codec/codec.py:34-143, quantize/residual_vq.py:68-152,
quantize/factorized_vector_quantize.py:52-127), computed from a state_dict, with seeded synthetic state_dicts and the margin helper of the
quantizer tests.  Eval mode, quantizer_type "fvq"."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as Fn


# ---- hyperparameters -------------------------------------------------------------------------------------------------------------
def recipe_encoder_hp():
    """models/tts/maskgct/config/maskgct.json: model.acoustic_codec.encoder"""
    return dict(d_model=96, up_ratios=[3, 4, 5, 8], out_channels=256, use_tanh=False)


def small_encoder_hp():
    return dict(d_model=32, up_ratios=[2, 3], out_channels=64, use_tanh=False)


def recipe_fvq_hp():
    return dict(D=256, d=8, K=1024, N=12, l2=True)


def small_fvq_hp():
    return dict(D=64, d=8, K=64, N=3, l2=True)


SMALL_VOCOS_HP = dict(input_channels=64, dim=64, intermediate_dim=192, num_layers=2, n_fft=256, hop_size=64, padding="same")


def decoder_kwargs(fhp, vhp=SMALL_VOCOS_HP):
    """CodecDecoder's keyword arguments for a quantizer `fhp` around a Vocos `vhp`"""
    return dict(in_channels=fhp["D"], num_quantizers=fhp["N"], codebook_size=fhp["K"], codebook_dim=fhp["d"], quantizer_type="fvq",
                use_l2_normlize=fhp["l2"], use_vocos=True, vocos_dim=vhp["dim"], vocos_intermediate_dim=vhp["intermediate_dim"],
                vocos_num_layers=vhp["num_layers"], n_fft=vhp["n_fft"], hop_size=vhp["hop_size"])


def decoder_state_dict(fhp, seed, vhp=SMALL_VOCOS_HP):
    """CodecDecoder's state_dict in the reference's order: quantizer.*, then model.* (Vocos, seed + 1)"""
    import vocos_ref as V

    sd = synth_fvq_state_dict(fhp, seed, prefix="quantizer.quantizers.")
    sd.update({"model." + k: v for k, v in V.synth_vocos_state_dict(vhp, seed + 1).items()})
    return sd


# ---- state_dict layouts -----------------------------------------------------------------------------------------------------------
def _wn(s, prefix, cout, cin, k):
    s[prefix + "bias"] = (cout,)
    s[prefix + "weight_g"] = (cout, 1, 1)
    s[prefix + "weight_v"] = (cout, cin, k)


def encoder_param_shapes(hp):
    """state_dict key -> shape, in the reference's order (weight-normed form)"""
    s = {}
    c = hp["d_model"]
    _wn(s, "block.0.", c, 1, 7)
    for i, stride in enumerate(hp["up_ratios"]):
        for u in range(3):
            p = f"block.{1 + i}.block.{u}.block."
            s[p + "0.alpha"] = (1, c, 1)
            _wn(s, p + "1.", c, c, 7)
            s[p + "2.alpha"] = (1, c, 1)
            _wn(s, p + "3.", c, c, 1)
        s[f"block.{1 + i}.block.3.alpha"] = (1, c, 1)
        _wn(s, f"block.{1 + i}.block.4.", 2 * c, c, 2 * stride)
        c *= 2
    n = len(hp["up_ratios"])
    s[f"block.{1 + n}.alpha"] = (1, c, 1)
    _wn(s, f"block.{2 + n}.", hp["out_channels"], c, 3)
    return s


def fvq_param_shapes(hp, prefix="quantizers."):
    s = {}
    for i in range(hp["N"]):
        p = f"{prefix}{i}."
        if hp["D"] != hp["d"]:
            _wn(s, p + "in_project.", hp["d"], hp["D"], 1)
            _wn(s, p + "out_project.", hp["D"], hp["d"], 1)
        s[p + "codebook.weight"] = (hp["K"], hp["d"])
    return s


def _synth(shapes, seed):
    """alpha in [0.5, 2]; weight_v ~ N(0, 1 / fan_in), weight_g = ||v|| (1 + N(0, 0.1)): unit-gain layers; biases N(0, 0.05); codebooks N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in shapes.items():
        if k.endswith("alpha"):
            sd[k] = 0.5 + 1.5 * torch.rand(shp, generator=g, dtype=torch.float64)
        elif k.endswith("weight_v"):
            sd[k] = torch.randn(shp, generator=g, dtype=torch.float64) / math.sqrt(shp[1] * shp[2])
        elif k.endswith("weight_g"):
            v = sd.get(k[:-1] + "v")
            assert v is None, "weight_g precedes weight_v in the reference's order"
            sd[k] = torch.randn(shp, generator=g, dtype=torch.float64)      # placeholder draw, fixed below
        elif k.endswith("codebook.weight"):
            sd[k] = torch.randn(shp, generator=g, dtype=torch.float64)
        else:
            sd[k] = 0.05 * torch.randn(shp, generator=g, dtype=torch.float64)
    for k in list(sd):
        if k.endswith("weight_g"):
            v = sd[k[:-1] + "v"]
            sd[k] = v.flatten(1).norm(dim=1).reshape(-1, 1, 1) * (1 + 0.1 * sd[k])
    return {k: v.float().contiguous() for k, v in sd.items()}


def synth_encoder_state_dict(hp, seed):
    return _synth(encoder_param_shapes(hp), seed)


def synth_fvq_state_dict(hp, seed, prefix="quantizers."):
    return _synth(fvq_param_shapes(hp, prefix), seed)


def synth_wave(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(B, 1, T, generator=g)).float()


def synth_latent(B, D, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, T, generator=g).float()


# ---- the forward passes -----------------------------------------------------------------------------------------------------------
def folded(P, prefix):
    """weight_norm: g * v / ||v|| over all but dim 0; a folded `weight` is taken as it is"""
    if prefix + "weight" in P:
        return P[prefix + "weight"]
    v, g = P[prefix + "weight_v"], P[prefix + "weight_g"]
    return g * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)


def snake(x, alpha):
    return x + (alpha + 1e-9).reciprocal() * torch.sin(alpha * x).pow(2)


def residual_unit(P, p, x, dilation):
    y = Fn.conv1d(snake(x, P[p + "0.alpha"]), folded(P, p + "1."), P[p + "1.bias"], dilation=dilation, padding=3 * dilation)
    y = Fn.conv1d(snake(y, P[p + "2.alpha"]), folded(P, p + "3."), P[p + "3.bias"])
    return x + y


def strided_conv(P, p_alpha, p_conv, x, stride):
    if p_alpha is not None:
        x = snake(x, P[p_alpha])
    return Fn.conv1d(x, folded(P, p_conv), P[p_conv + "bias"], stride=stride, padding=math.ceil(stride / 2))


def encoder_forward(sd, hp, x, dtype=torch.float64):
    P = {k: v.to(dtype) for k, v in sd.items()}
    h = Fn.conv1d(x.to(dtype), folded(P, "block.0."), P["block.0.bias"], padding=3)
    for i, stride in enumerate(hp["up_ratios"]):
        for u, dil in enumerate((1, 3, 9)):
            h = residual_unit(P, f"block.{1 + i}.block.{u}.block.", h, dil)
        h = strided_conv(P, f"block.{1 + i}.block.3.alpha", f"block.{1 + i}.block.4.", h, stride)
    n = len(hp["up_ratios"])
    h = Fn.conv1d(snake(h, P[f"block.{1 + n}.alpha"]), folded(P, f"block.{2 + n}."), P[f"block.{2 + n}.bias"], padding=1)
    return torch.tanh(h) if hp.get("use_tanh") else h


def fvq_distances(P, p, hp, residual):
    """-> (z_e [B, d, T], dist [B * T, K]) of one level, the reference's expression"""
    proj = hp["D"] != hp["d"]
    z_e = Fn.conv1d(residual, folded(P, p + "in_project."), P[p + "in_project.bias"]) if proj else residual
    enc = z_e.transpose(1, 2).reshape(-1, hp["d"])
    cb = P[p + "codebook.weight"]
    if hp["l2"]:
        enc, cb = Fn.normalize(enc), Fn.normalize(cb)
    dist = enc.pow(2).sum(1, keepdim=True) - 2 * enc @ cb.t() + cb.pow(2).sum(1, keepdim=True).t()
    return z_e, dist


def rvq_forward(sd, hp, z, dtype=torch.float64, n=None, codes=None, prefix="quantizers."):
    """ResidualVQ.forward in eval mode.  -> dict(zq, codes [n, B, T], margin [n, B, T] second-best minus best distance, dist: list of [B*T, K],
    all_q [n, B, D, T]).  `codes` given: follow THOSE indices instead of the arg-min (the trajectory of another implementation)."""
    P = {k: v.to(dtype) for k, v in sd.items()}
    B, D, T = z.shape
    n = hp["N"] if n is None else n
    residual = z.to(dtype)
    zq = torch.zeros_like(residual)
    out = dict(codes=[], margin=[], dist=[], all_q=[])
    for i in range(n):
        p = f"{prefix}{i}."
        z_e, dist = fvq_distances(P, p, hp, residual)
        idx = (-dist).max(1)[1] if codes is None else codes[i].reshape(-1)
        two = torch.topk(dist, 2, dim=1, largest=False).values if dist.shape[1] > 1 else torch.cat([dist, dist + 1], 1)
        q = Fn.embedding(idx, P[p + "codebook.weight"]).reshape(B, T, -1).transpose(1, 2)
        q = z_e + (q - z_e)
        if hp["D"] != hp["d"]:
            q = Fn.conv1d(q, folded(P, p + "out_project."), P[p + "out_project.bias"])
        zq = zq + q
        residual = residual - q
        out["codes"].append(idx.reshape(B, T))
        out["margin"].append((two[:, 1] - two[:, 0]).reshape(B, T))
        out["dist"].append(dist)
        out["all_q"].append(q)
    return dict(zq=zq, codes=torch.stack(out["codes"]), margin=torch.stack(out["margin"]), dist=out["dist"], all_q=torch.stack(out["all_q"]))


def vq2emb(sd, hp, codes, dtype=torch.float64, n=None, prefix="quantizers."):
    P = {k: v.to(dtype) for k, v in sd.items()}
    n = hp["N"] if n is None else n
    _, B, T = codes.shape
    out = 0.0
    for i in range(n):
        p = f"{prefix}{i}."
        q = Fn.embedding(codes[i], P[p + "codebook.weight"]).transpose(1, 2)
        if hp["D"] != hp["d"]:
            q = Fn.conv1d(q, folded(P, p + "out_project."), P[p + "out_project.bias"])
        out = out + q
    return out


def margin_rule(sd, hp, z, n=None, prefix="quantizers."):
    """The decision rule of the quantizer tests.  tau = 8 x the largest |dist32 - dist64| of the fp32 restatement walking the fp64 trajectory
    (same codes, so the two see the same residuals up to rounding); a (level, frame) is DECIDED when the fp64 margin at every level <= it
    exceeds tau.  -> (ref64, ref32, tau, decided [n, B, T] bool)"""
    r64 = rvq_forward(sd, hp, z, torch.float64, n, prefix=prefix)
    r32 = rvq_forward(sd, hp, z, torch.float32, n, codes=r64["codes"], prefix=prefix)
    tau = 8.0 * max(float((a.double() - b).abs().max()) for a, b in zip(r32["dist"], r64["dist"]))
    decided = torch.cumprod((r64["margin"] > tau).to(torch.int64), dim=0).bool()
    return r64, r32, tau, decided


# ---- the derived bounds of the f16x3 ops (tests/test_gpu_codec.py states the derivation) ---------------------------------------------
def d_snake(v, a):
    """error of the library's snake on an exact fp32 argument: (3.3e-7 + 1.2e-7 |a v|) / a + 2.4e-7 |snake(v)|"""
    return (3.3e-7 + 1.2e-7 * (a * v).abs()) / a + 2.4e-7 * snake(v, a).abs()


def sconv_bound(w, b, alpha, x, stride, padding):
    """fp64 output of [snake ->] Conv1d(k = 2 stride, stride, padding) and the derived bound of each element:
    2e-6 (|w| * |snake(x)| + |b|) + 3e-7 |ref| + |w| * d_snake(x)"""
    kw = dict(stride=stride, padding=padding)
    s1 = x if alpha is None else snake(x, alpha)
    ref = Fn.conv1d(s1, w, b, **kw)
    tol = 2e-6 * (Fn.conv1d(s1.abs(), w.abs(), **kw) + b.abs()[None, :, None]) + 3e-7 * ref.abs()
    if alpha is not None:
        tol = tol + Fn.conv1d(d_snake(x, alpha), w.abs(), **kw)
    return ref, tol


def unit_bound(sd64, x, dil, padding=None):
    """fp64 output of the residual unit and the derived bound of each element; padding: conv7's, 3 * dil (the unit's own) when None"""
    pad = 3 * dil if padding is None else padding
    a1, a2 = sd64["0.alpha"], sd64["2.alpha"]
    w1, w2 = folded(sd64, "1."), folded(sd64, "3.")
    b1, b2 = sd64["1.bias"], sd64["3.bias"]
    s1 = snake(x, a1)
    v = Fn.conv1d(s1, w1, b1, dilation=dil, padding=pad)
    tol1 = 2e-6 * (Fn.conv1d(s1.abs(), w1.abs(), dilation=dil, padding=pad) + b1.abs()[None, :, None]) + 3e-7 * v.abs() \
        + Fn.conv1d(d_snake(x, a1), w1.abs(), dilation=dil, padding=pad)
    z = snake(v, a2)
    dz = 2 * tol1 + d_snake(v, a2)
    r = Fn.conv1d(z, w2, b2)
    tol2 = Fn.conv1d(dz, w2.abs()) + 2e-6 * (Fn.conv1d(z.abs(), w2.abs()) + b2.abs()[None, :, None]) + 3e-7 * r.abs()
    y = x + r
    return y, tol2 + 1.2e-7 * (x.abs() + r.abs()) + 1.2e-7 * y.abs()


def unit_param_shapes(Cn):
    """the residual unit's own state_dict: 0.alpha, 1. (conv7), 2.alpha, 3. (conv 1 x 1)"""
    shapes = {"0.alpha": (1, Cn, 1)}
    _wn(shapes, "1.", Cn, Cn, 7)
    shapes["2.alpha"] = (1, Cn, 1)
    _wn(shapes, "3.", Cn, Cn, 1)
    return shapes
