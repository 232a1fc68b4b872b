"""fp64 / fp32 restatement of SpeechTokenizer in eval mode, written from the reference's arithmetic (models/codec/speechtokenizer/model.py,
modules/{conv,seanet,lstm}.py, modules/quantization/{core_vq,vq}.py): reflect pads with the small-input rule, ELU, convs, the LSTM stacks and the
Euclidean residual quantizer with codes, distances and margins.  Weights regenerate from seeds.  Not imported by the library."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as Fn

from codec_ref import folded


def small_hp():
    return dict(n_filters=8, dimension=32, strides=[4, 3, 2, 2], lstm_layers=2, bidirectional=True, dilation_base=2, residual_kernel_size=3,
                n_residual_layers=1, activation="ELU", sample_rate=16000, n_q=4, codebook_size=64, semantic_dimension=24)


def recipe_hp():
    return dict(n_filters=64, dimension=1024, strides=[8, 5, 4, 2], lstm_layers=2, bidirectional=True, dilation_base=2, residual_kernel_size=3,
                n_residual_layers=1, activation="ELU", sample_rate=16000, n_q=8, codebook_size=1024, semantic_dimension=768)


def hop(hp):
    return int(math.prod(hp["strides"]))


# ---- layout: the reference's modules in order, as (kind, prefix, geometry) ---------------------------------------------------------------
def encoder_layout(hp, p="encoder.model."):
    nf, out = hp["n_filters"], []
    i, mult = 0, 1
    out.append(("conv", f"{p}{i}.", dict(cin=1, cout=nf, k=7, stride=1, dil=1, elu=False)))
    i += 1
    for ratio in reversed(hp["strides"]):
        for j in range(hp["n_residual_layers"]):
            out.append(("res", f"{p}{i}.", dict(dim=mult * nf, k=hp["residual_kernel_size"], dil=hp["dilation_base"] ** j,
                                                 true_skip=bool(hp.get("true_skip")))))
            i += 1
        i += 1                                                  # the ELU module
        out.append(("conv", f"{p}{i}.", dict(cin=mult * nf, cout=2 * mult * nf, k=2 * ratio, stride=ratio, dil=1, elu=True)))
        i += 1
        mult *= 2
    if hp["lstm_layers"]:
        out.append(("lstm", f"{p}{i}.", dict(H=mult * nf, layers=hp["lstm_layers"], bidir=bool(hp["bidirectional"]))))
        i += 1
    if hp["bidirectional"]:
        mult *= 2
    i += 1
    out.append(("conv", f"{p}{i}.", dict(cin=mult * nf, cout=hp["dimension"], k=7, stride=1, dil=1, elu=True)))
    return out


def decoder_layout(hp, p="decoder.model."):
    nf, out = hp["n_filters"], []
    i, mult = 0, 2 ** len(hp["strides"])
    out.append(("conv", f"{p}{i}.", dict(cin=hp["dimension"], cout=mult * nf, k=7, stride=1, dil=1, elu=False)))
    i += 1
    if hp["lstm_layers"]:
        out.append(("lstm", f"{p}{i}.", dict(H=mult * nf, layers=hp["lstm_layers"], bidir=False)))
        i += 1
    for ratio in hp["strides"]:
        i += 1
        out.append(("tconv", f"{p}{i}.", dict(cin=mult * nf, cout=mult * nf // 2, stride=ratio)))
        i += 1
        for j in range(hp["n_residual_layers"]):
            out.append(("res", f"{p}{i}.", dict(dim=mult * nf // 2, k=hp["residual_kernel_size"], dil=hp["dilation_base"] ** j,
                                                 true_skip=bool(hp.get("true_skip")))))
            i += 1
        mult //= 2
    i += 1
    out.append(("conv", f"{p}{i}.", dict(cin=nf, cout=1, k=7, stride=1, dil=1, elu=True)))
    return out


def _wn(shapes, p, cout, cin, k, transposed=False):
    d0 = cin if transposed else cout
    shapes[p + "bias"] = (cout,)
    shapes[p + "weight_g"] = (d0, 1, 1)
    shapes[p + "weight_v"] = (cin, cout, k) if transposed else (cout, cin, k)


def _layout_shapes(shapes, layout):
    for kind, p, g in layout:
        if kind == "conv":
            _wn(shapes, p + "conv.conv.", g["cout"], g["cin"], g["k"])
        elif kind == "tconv":
            _wn(shapes, p + "convtr.convtr.", g["cout"], g["cin"], 2 * g["stride"], transposed=True)
        elif kind == "res":
            _wn(shapes, p + "block.1.conv.conv.", g["dim"] // 2, g["dim"], g["k"])
            _wn(shapes, p + "block.3.conv.conv.", g["dim"], g["dim"] // 2, 1)
            if not g["true_skip"]:
                _wn(shapes, p + "shortcut.conv.conv.", g["dim"], g["dim"], 1)
        else:
            H = g["H"]
            for layer in range(g["layers"]):
                for sfx in ("", "_reverse") if g["bidir"] else ("",):
                    cin = H if layer == 0 else H * (2 if g["bidir"] else 1)
                    shapes[f"{p}lstm.weight_ih_l{layer}{sfx}"] = (4 * H, cin)
                    shapes[f"{p}lstm.weight_hh_l{layer}{sfx}"] = (4 * H, H)
                    shapes[f"{p}lstm.bias_ih_l{layer}{sfx}"] = (4 * H,)
                    shapes[f"{p}lstm.bias_hh_l{layer}{sfx}"] = (4 * H,)


def param_shapes(hp):
    """every key of SpeechTokenizer(hp).state_dict() with its shape, in the reference's order"""
    shapes = OrderedDict()
    _layout_shapes(shapes, encoder_layout(hp))
    if hp["dimension"] != hp["semantic_dimension"]:
        shapes["transform.weight"] = (hp["semantic_dimension"], hp["dimension"])
        shapes["transform.bias"] = (hp["semantic_dimension"],)
    for i in range(hp["n_q"]):
        p = f"quantizer.vq.layers.{i}._codebook."
        shapes[p + "inited"] = (1,)
        shapes[p + "cluster_size"] = (hp["codebook_size"],)
        shapes[p + "embed"] = (hp["codebook_size"], hp["dimension"])
        shapes[p + "embed_avg"] = (hp["codebook_size"], hp["dimension"])
    _layout_shapes(shapes, decoder_layout(hp))
    return shapes


def synth_codebooks(D, K, N, seed, s=1.0):
    """randn * s * 0.6^level: each level's rows at the scale of the residual the levels before it leave"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(K, D, generator=g) * s * 0.6 ** lvl).float() for lvl in range(N)]


def stack_hp():
    """a SEANet pair that takes the routes the model configurations do not: two residual layers per ratio (dilations 1 and 2, so the reflect
    staging of a dilated conv) and true_skip (the block's input itself is the residual)"""
    return dict(n_filters=8, dimension=16, strides=[3, 2], lstm_layers=1, bidirectional=False, dilation_base=2, residual_kernel_size=3,
                n_residual_layers=2, true_skip=True)


def stack_shapes(hp, which):
    """the keys of a stand-alone SEANetEncoder / SEANetDecoder (prefix ``model.``)"""
    shapes = OrderedDict()
    _layout_shapes(shapes, (encoder_layout if which == "encoder" else decoder_layout)(hp, "model."))
    return shapes


def synth_stack_state_dict(hp, which, seed):
    return OrderedDict((k, v.float()) for k, v in _synth_params(stack_shapes(hp, which), seed).items())


def stack_forward(sd, hp, which, x, dtype=torch.float64):
    return run_layout(_P(sd, dtype), (encoder_layout if which == "encoder" else decoder_layout)(hp, "model."), x.to(dtype))


def synth_state_dict(hp, seed):
    """weight-normed convs with rows of norm about 1 (activations keep their scale), LSTM weights at U(+-1/sqrt(H)), codebooks as synth_codebooks"""
    sd = _synth_params(param_shapes(hp), seed)
    cbs = synth_codebooks(hp["dimension"], hp["codebook_size"], hp["n_q"], seed + 1, s=0.5)
    out = OrderedDict()
    for k in param_shapes(hp):
        if k.endswith("_codebook.embed") or k.endswith("_codebook.embed_avg"):
            out[k] = cbs[int(k.split(".")[3])].clone()
        else:
            out[k] = sd[k].float()
    return out


def _synth_params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for k, shape in shapes.items():
        if k.endswith("weight_v") or k == "transform.weight":
            fan = shape[1] * (shape[2] if len(shape) == 3 else 1)
            sd[k] = torch.randn(shape, generator=g) / math.sqrt(fan)
        elif k.endswith("weight_g"):
            sd[k] = 0.9 + 0.2 * torch.rand(shape, generator=g)
        elif ".lstm." in k:
            H = shape[0] // 4
            sd[k] = (2 * torch.rand(shape, generator=g) - 1) / math.sqrt(H)
        elif k.endswith("inited"):
            sd[k] = torch.ones(shape)
        elif k.endswith("cluster_size"):
            sd[k] = torch.ones(shape)
        elif k.endswith("embed") or k.endswith("embed_avg"):
            continue
        else:
            sd[k] = 0.1 * torch.randn(shape, generator=g)
    return sd


def codebooks_of(sd, hp):
    return [sd[f"quantizer.vq.layers.{i}._codebook.embed"] for i in range(hp["n_q"])]


def synth_wave(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(B, 1, T, generator=g)).float()


# ---- pads and convs ---------------------------------------------------------------------------------------------------------------------
def extra_padding(length, k, stride, padding_total):
    n_frames = (length - k + padding_total) / stride + 1
    return (math.ceil(n_frames) - 1) * stride + (k - padding_total) - length


def pad1d_reflect(x, pl, pr):
    """conv.py:97-119: zero-extend a short input on the right, reflect, crop the extension"""
    length = x.shape[-1]
    max_pad = max(pl, pr)
    extra = 0
    if length <= max_pad:
        extra = max_pad - length + 1
        x = Fn.pad(x, (0, extra))
    y = Fn.pad(x, (pl, pr), "reflect") if (pl or pr) else x
    return y[..., :y.shape[-1] - extra]


def sconv_pads(T, k, stride, dil):
    total = (k - 1) * dil - (stride - 1)
    right = total // 2
    return total - right, right + extra_padding(T, k, stride, total)


def sconv(P, p, x, k, stride=1, dil=1):
    pl, pr = sconv_pads(x.shape[-1], k, stride, dil)
    return Fn.conv1d(pad1d_reflect(x, pl, pr), folded(P, p + "conv.conv."), P[p + "conv.conv.bias"], stride=stride, dilation=dil)


def stconv(P, p, x, stride):
    v, g = P[p + "convtr.convtr.weight_v"], P[p + "convtr.convtr.weight_g"]
    w = g * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)
    y = Fn.conv_transpose1d(x, w, P[p + "convtr.convtr.bias"], stride=stride)
    right = stride // 2
    return y[..., stride - right:y.shape[-1] - right]


def resblock(P, p, x, k, dil, true_skip=False):
    h = sconv(P, p + "block.1.", Fn.elu(x), k, dil=dil)
    h = sconv(P, p + "block.3.", Fn.elu(h), 1)
    return (x if true_skip else sconv(P, p + "shortcut.", x, 1)) + h


# ---- LSTM -------------------------------------------------------------------------------------------------------------------------------
def lstm_recur(w_hh, gx, skip=None):
    """the recurrence alone: w_hh [ndir, 4H, H], gx [B, ndir * 4H, T] (W_ih x + b_ih + b_hh, gate rows i, f, g, o per direction), skip [B, H, T]
    or None -> y [B, ndir * H, T]; direction 1 walks time backwards"""
    ndir, H4, H = w_hh.shape
    B, _, T = gx.shape
    ys = []
    for d in range(ndir):
        h = torch.zeros(B, H, dtype=gx.dtype, device=gx.device)
        c = torch.zeros(B, H, dtype=gx.dtype, device=gx.device)
        y = torch.zeros(B, H, T, dtype=gx.dtype, device=gx.device)
        for s in range(T):
            t = T - 1 - s if d else s
            gates = gx[:, d * H4:(d + 1) * H4, t] + h @ w_hh[d].t()
            i, f, g, o = gates.split(H, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            y[:, :, t] = h
        ys.append(y if skip is None else y + skip)
    return torch.cat(ys, 1)


def lstm_weights(P, p, layer, bidir):
    sfx = ("", "_reverse") if bidir else ("",)
    w_ih = torch.cat([P[f"{p}weight_ih_l{layer}{s}"] for s in sfx], 0)
    w_hh = torch.stack([P[f"{p}weight_hh_l{layer}{s}"] for s in sfx], 0)
    b = torch.cat([P[f"{p}bias_ih_l{layer}{s}"] + P[f"{p}bias_hh_l{layer}{s}"] for s in sfx], 0)
    return w_ih, w_hh, b


def lstm_input_projection(w_ih, b, x):
    return torch.einsum("gi,bit->bgt", w_ih, x) + b[None, :, None]


def slstm(P, p, x, layers, bidir, skip=True):
    """SLSTM.forward in the conv layout; P[p + 'weight_ih_l0'] .. as nn.LSTM names them"""
    h = x
    for layer in range(layers):
        w_ih, w_hh, b = lstm_weights(P, p, layer, bidir)
        last = layer == layers - 1
        h = lstm_recur(w_hh, lstm_input_projection(w_ih, b, h), x if (skip and last) else None)
    return h


# ---- the stacks ---------------------------------------------------------------------------------------------------------------------------
def run_layout(P, layout, x):
    for kind, p, g in layout:
        if kind == "conv":
            x = sconv(P, p, Fn.elu(x) if g["elu"] else x, g["k"], g["stride"], g["dil"])
        elif kind == "tconv":
            x = stconv(P, p, Fn.elu(x), g["stride"])
        elif kind == "res":
            x = resblock(P, p, x, g["k"], g["dil"], g["true_skip"])
        else:
            x = slstm(P, p + "lstm.", x, g["layers"], g["bidir"])
    return x


def _P(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def encoder_forward(sd, hp, x, dtype=torch.float64):
    return run_layout(_P(sd, dtype), encoder_layout(hp), x.to(dtype))


def decoder_forward(sd, hp, z, dtype=torch.float64):
    return run_layout(_P(sd, dtype), decoder_layout(hp), z.to(dtype))


# ---- the quantizer ----------------------------------------------------------------------------------------------------------------------
def evq_distances(cb, residual):
    """core_vq.py:180-188 -> dist [B * T, K] (the larger the closer)"""
    B, D, T = residual.shape
    x = residual.transpose(1, 2).reshape(-1, D)
    embed = cb.t()
    return -(x.pow(2).sum(1, keepdim=True) - 2 * x @ embed + embed.pow(2).sum(0, keepdim=True))


def evq_forward(cbs, z, dtype=torch.float64, st=0, n_q=None, codes=None):
    """levels [st, n_q) from the WHOLE input (ResidualVectorQuantization.encode's quirk for st > 0; st = 0 is .forward).  -> dict(zq, codes
    [n, B, T], margin [n, B, T] best minus second-best distance, dist: list of [B * T, K], all_q [n, B, D, T]).  `codes` given: follow THOSE."""
    cbs = [c.to(dtype) for c in cbs]
    n_q = len(cbs) if n_q is None else n_q
    B, D, T = z.shape
    residual = z.to(dtype)
    zq = 0.0
    out = dict(codes=[], margin=[], dist=[], all_q=[])
    for i, lvl in enumerate(range(st, n_q)):
        dist = evq_distances(cbs[lvl], residual)
        idx = dist.max(dim=-1).indices if codes is None else codes[i].reshape(-1)
        two = torch.topk(dist, 2, dim=1).values if dist.shape[1] > 1 else torch.cat([dist, dist - 1], 1)
        q = Fn.embedding(idx, cbs[lvl]).reshape(B, T, D).transpose(1, 2)
        residual = residual - q
        zq = zq + q
        out["codes"].append(idx.reshape(B, T))
        out["margin"].append((two[:, 0] - two[:, 1]).reshape(B, T))
        out["dist"].append(dist)
        out["all_q"].append(q)
    return dict(zq=zq, codes=torch.stack(out["codes"]), margin=torch.stack(out["margin"]), dist=out["dist"], all_q=torch.stack(out["all_q"]))


def rvq_encode_plain(cbs, z, st=0, n_q=None):
    """ResidualVectorQuantization.encode with the reference's own ops and nothing else (core_vq.py:180-188,367-380): per level the distance,
    max(-1).indices, the embedding and the subtraction -- the yardstick tools/speechtokenizer_bench.py times"""
    n_q = len(cbs) if n_q is None else n_q
    B, D, T = z.shape
    residual = z
    out = []
    for cb in cbs[st:n_q]:
        x = residual.transpose(1, 2).reshape(-1, D)
        embed = cb.t()
        dist = -(x.pow(2).sum(1, keepdim=True) - 2 * x @ embed + embed.pow(2).sum(0, keepdim=True))
        ind = dist.max(dim=-1).indices.view(B, T)
        residual = residual - Fn.embedding(ind, cb).transpose(1, 2)
        out.append(ind)
    return torch.stack(out)


def evq_decode(cbs, codes, dtype=torch.float64, st=0):
    out = torch.tensor(0.0, dtype=dtype, device=codes.device)
    for i in range(codes.shape[0]):
        out = out + Fn.embedding(codes[i], cbs[st + i].to(dtype)).transpose(1, 2)
    return out


def margin_rule(cbs, z, st=0, n_q=None):
    """codec_ref.margin_rule's definition on the Euclidean quantizer: tau = 8 x the largest |dist32 - dist64| of the fp32 restatement walking the
    fp64 trajectory; a (level, frame) is DECIDED when the fp64 margin at every level up to it exceeds tau.  -> (ref64, ref32, tau, decided)"""
    r64 = evq_forward(cbs, z, torch.float64, st, n_q)
    r32 = evq_forward(cbs, z, torch.float32, st, n_q, codes=r64["codes"])
    tau = 8.0 * max(float((a.double() - b).abs().max()) for a, b in zip(r32["dist"], r64["dist"]))
    decided = torch.cumprod((r64["margin"] > tau).to(torch.int64), dim=0).bool()
    return r64, r32, tau, decided


def quantizer_case(D, K, N, T, s=1.0, B=2):
    """the inputs of the quantizer tests: codebooks randn * s * 0.6^level, latents randn * s"""
    seed = 7000 + 131 * D + 17 * K + T
    cbs = synth_codebooks(D, K, N, seed, s)
    g = torch.Generator().manual_seed(seed + 1)
    return cbs, (torch.randn(B, D, T, generator=g) * s).float()


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def feature(sd, q, dtype):
    if "transform.weight" not in sd:
        return q.transpose(1, 2)
    return q.transpose(1, 2) @ sd["transform.weight"].to(dtype).t() + sd["transform.bias"].to(dtype)


def model_forward(sd, hp, x, dtype=torch.float64, n_q=None, codes=None):
    """SpeechTokenizer.forward(x, n_q, layers=[0]) -> dict(e, codes, quantized, o, feature); `codes`: follow those"""
    e = encoder_forward(sd, hp, x, dtype)
    r = evq_forward(codebooks_of(sd, hp), e, dtype, 0, n_q or hp["n_q"], codes=codes)
    return dict(e=e, codes=r["codes"], quantized=r["zq"], o=decoder_forward(sd, hp, r["zq"], dtype), feature=feature(sd, r["all_q"][0], dtype),
                margin=r["margin"])


def model_decode(sd, hp, codes, dtype=torch.float64, st=0):
    return decoder_forward(sd, hp, evq_decode(codebooks_of(sd, hp), codes, dtype, st), dtype)
