"""fp64 / fp32 torch restatement of FACodec (models/codec/ns3_codec/facodec.py:121-576, quantize/{fvq,rvq}.py, transformer.py,
alias_free_torch/), computed from a state_dict under the reference's keys, with seeded synthetic state_dicts and the margin helper of the
three-group quantizer tests.  Eval mode.  The predictor heads (never run in inference) are not restated."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as Fn

import codec_ref as C

PREDICTOR_PREFIXES = ("f0_predictor.", "phone_predictor.", "res_f0_predictor.", "res_phone_predictor.", "content_f0_predictor.",
                      "prosody_phone_predictor.", "x_timbre_predictor.")


# ---- hyperparameters -------------------------------------------------------------------------------------------------------------
def recipe_encoder_hp():
    """models/codec/ns3_codec/README.md"""
    return dict(ngf=32, up_ratios=[2, 4, 5, 5], out_channels=256)


def recipe_decoder_hp():
    return dict(in_channels=256, upsample_initial_channel=1024, ngf=32, up_ratios=[5, 5, 4, 2], vq_num_q_c=2, vq_num_q_p=1, vq_num_q_r=3, vq_dim=256,
                codebook_dim=8, codebook_size_prosody=10, codebook_size_content=10, codebook_size_residual=10, use_gr_x_timbre=True,
                use_gr_residual_f0=True, use_gr_residual_phone=True)


def small_encoder_hp():
    return dict(ngf=32, up_ratios=[2, 3], out_channels=256)


def small_decoder_hp():
    return dict(in_channels=256, upsample_initial_channel=128, ngf=32, up_ratios=[3, 2], vq_num_q_c=2, vq_num_q_p=1, vq_num_q_r=3, vq_dim=256,
                codebook_dim=8, codebook_size_prosody=5, codebook_size_content=6, codebook_size_residual=5)


# latent seeds of the GPU quantizer tests, per frame count: the fp64 reference alone decides every frame for them (tests/test_oracle_facodec.py)
QUANT_SEEDS = {1: 100, 63: 101, 65: 102}

TIMBRE_HP = dict(layers=4, hidden=256, heads=4, filter=1024, kernel=5)


def group_hps(hp):
    """the three quantizer groups (prosody, content, residual) as codec_ref's fvq hyperparameters"""
    out = [dict(D=hp["vq_dim"], d=hp["codebook_dim"], K=2 ** hp["codebook_size_prosody"], N=hp["vq_num_q_p"], l2=True),
           dict(D=hp["vq_dim"], d=hp["codebook_dim"], K=2 ** hp["codebook_size_content"], N=hp["vq_num_q_c"], l2=True)]
    if hp["vq_num_q_r"] > 0:
        out.append(dict(D=hp["vq_dim"], d=hp["codebook_dim"], K=2 ** hp["codebook_size_residual"], N=hp["vq_num_q_r"], l2=True))
    return out


# ---- the anti-aliasing filter ----------------------------------------------------------------------------------------------------
def kaiser_sinc_filter12():
    """alias_free_torch/filter.py:28-59 for cutoff 0.25, half width 0.3, 12 taps (ratio 2, both ways) -> [1, 1, 12] fp32"""
    half_size = 6
    A = 2.285 * (half_size - 1) * math.pi * (4 * 0.3) + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50.0 else (0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21.0) if A >= 21.0 else 0.0)
    window = torch.kaiser_window(12, beta=beta, periodic=False)
    time = torch.arange(-half_size, half_size) + 0.5
    f = 2 * 0.25 * window * torch.sinc(2 * 0.25 * time)
    f /= f.sum()
    return f.view(1, 1, 12)


FILT = kaiser_sinc_filter12()


# ---- state_dict layouts (the reference's keys and order) ---------------------------------------------------------------------------
def _act(s, p, c):
    s[p + "act.alpha"] = (c,)
    s[p + "act.beta"] = (c,)
    s[p + "upsample.filter"] = (1, 1, 12)
    s[p + "downsample.lowpass.filter"] = (1, 1, 12)


def _unit(s, p, c):
    _act(s, p + "block.0.", c)
    C._wn(s, p + "block.1.", c, c, 7)
    _act(s, p + "block.2.", c)
    C._wn(s, p + "block.3.", c, c, 1)


def unit_param_shapes(c):
    s = {}
    _unit(s, "", c)
    return s


def encoder_param_shapes(hp):
    s = {}
    c = hp["ngf"]
    C._wn(s, "block.0.", c, 1, 7)
    for i, stride in enumerate(hp["up_ratios"]):
        for u in range(3):
            _unit(s, f"block.{1 + i}.block.{u}.", c)
        _act(s, f"block.{1 + i}.block.3.", c)
        C._wn(s, f"block.{1 + i}.block.4.", 2 * c, c, 2 * stride)
        c *= 2
    n = len(hp["up_ratios"])
    _act(s, f"block.{1 + n}.", c)
    C._wn(s, f"block.{2 + n}.", hp["out_channels"], c, 3)
    return s


def quantizer_param_shapes(hp, prefix="quantizer."):
    s = {}
    for gi, g in enumerate(group_hps(hp)):
        for i in range(g["N"]):
            p = f"{prefix}{gi}.layers.{i}."
            if g["D"] != g["d"]:
                for name, (o, n_in) in (("in_proj.", (g["d"], g["D"])), ("out_proj.", (g["D"], g["d"]))):
                    s[p + name + "bias"] = (o,)
                    s[p + name + "weight_g"] = (o, 1)
                    s[p + name + "weight_v"] = (o, n_in)
            s[p + "_codebook.weight"] = (g["K"], g["d"])
    return s


def timbre_param_shapes(prefix="timbre_encoder."):
    H, Fc, K = TIMBRE_HP["hidden"], TIMBRE_HP["filter"], TIMBRE_HP["kernel"]
    s = {prefix + "position_emb.pe": (5000, 1, H)}
    for i in range(TIMBRE_HP["layers"]):
        p = f"{prefix}layers.{i}."
        s[p + "ln_1.weight"] = (H,)
        s[p + "ln_1.bias"] = (H,)
        s[p + "ln_2.weight"] = (H,)
        s[p + "ln_2.bias"] = (H,)
        s[p + "self_attn.in_proj_weight"] = (3 * H, H)
        s[p + "self_attn.in_proj_bias"] = (3 * H,)
        s[p + "self_attn.out_proj.weight"] = (H, H)
        s[p + "self_attn.out_proj.bias"] = (H,)
        s[p + "ffn.ffn_1.weight"] = (Fc, H, K)
        s[p + "ffn.ffn_1.bias"] = (Fc,)
        s[p + "ffn.ffn_2.weight"] = (H, Fc)
        s[p + "ffn.ffn_2.bias"] = (H,)
    s[prefix + "last_ln.weight"] = (H,)
    s[prefix + "last_ln.bias"] = (H,)
    return s


def decoder_param_shapes(hp):
    """FACodecDecoder's state_dict without the predictor heads, in the reference's order"""
    s = quantizer_param_shapes(hp)
    ch = hp["upsample_initial_channel"]
    C._wn(s, "model.0.", ch, hp["in_channels"], 7)
    out = ch
    for i, stride in enumerate(hp["up_ratios"]):
        cin, out = ch // 2 ** i, ch // 2 ** (i + 1)
        p = f"model.{1 + i}."
        _act(s, p + "block.0.", cin)
        s[p + "block.1.bias"] = (out,)
        s[p + "block.1.weight_g"] = (cin, 1, 1)
        s[p + "block.1.weight_v"] = (cin, out, 2 * stride)
        for u in range(3):
            _unit(s, f"{p}block.{2 + u}.", out)
    n = len(hp["up_ratios"])
    _act(s, f"model.{1 + n}.", out)
    C._wn(s, f"model.{2 + n}.", 1, out, 7)
    s.update(timbre_param_shapes())
    s["timbre_linear.weight"] = (2 * hp["in_channels"], hp["in_channels"])
    s["timbre_linear.bias"] = (2 * hp["in_channels"],)
    return s


def positional_table(H, max_len=5000):
    """transformer.py:40-46"""
    position = torch.arange(max_len).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, H, 2) * (-math.log(10000.0) / H))
    pe = torch.zeros(max_len, 1, H)
    pe[:, 0, 0::2] = torch.sin(position * div_term)
    pe[:, 0, 1::2] = torch.cos(position * div_term)
    return pe


def _synth(shapes, seed):
    """log-scale alpha / beta uniform in [ln 0.3, ln 3]; weight_v ~ N(0, 1 / fan_in), weight_g = ||v|| (1 + N(0, 0.1)); plain weights N(0, 1 / fan_in);
    LayerNorm weights 1 + N(0, 0.1); biases N(0, 0.05); codebooks N(0, 1); the decoder's last conv x 0.1; the filters and the position table are the reference's buffers"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in shapes.items():
        if k.endswith("act.alpha") or k.endswith("act.beta"):
            sd[k] = math.log(0.3) + (math.log(3.0) - math.log(0.3)) * torch.rand(shp, generator=g, dtype=torch.float64)
        elif k.endswith(".filter"):
            sd[k] = FILT.double().clone()
        elif k.endswith("position_emb.pe"):
            sd[k] = positional_table(shp[2], shp[0]).double()
        elif k.endswith("weight_v"):
            fan = 1
            for n in shp[1:]:
                fan *= n
            if k.endswith("block.1.weight_v") and len(shp) == 3 and k.startswith("model.") and k.count("block.") == 1:
                fan = shp[0] * 2          # a ConvTranspose1d(k = 2 s, stride s): two taps of every input channel meet in one output sample
            sd[k] = torch.randn(shp, generator=g, dtype=torch.float64) / math.sqrt(fan)
        elif k.endswith("weight_g"):
            sd[k] = torch.randn(shp, generator=g, dtype=torch.float64)      # placeholder draw, fixed below
        elif k.endswith("_codebook.weight"):
            sd[k] = torch.randn(shp, generator=g, dtype=torch.float64)
        elif k.endswith("ln_1.weight") or k.endswith("ln_2.weight") or k.endswith("last_ln.weight"):
            sd[k] = 1 + 0.1 * torch.randn(shp, generator=g, dtype=torch.float64)
        elif k.endswith("weight"):
            fan = 1
            for n in shp[1:]:
                fan *= n
            sd[k] = torch.randn(shp, generator=g, dtype=torch.float64) / math.sqrt(fan)
        else:
            sd[k] = 0.05 * torch.randn(shp, generator=g, dtype=torch.float64)
    for k in list(sd):
        if k.endswith("weight_g"):
            v = sd[k[:-1] + "v"]
            sd[k] = v.flatten(1).norm(dim=1).reshape(sd[k].shape) * (1 + 0.1 * sd[k])
    for k in list(sd):
        if k.startswith("model.") and k.endswith("weight_g") and sd[k].numel() == 1:
            sd[k] = 0.1 * sd[k]                             # the decoder's last conv: keeps the tanh out of saturation
    if "timbre_linear.bias" in sd:
        n = sd["timbre_linear.bias"].numel() // 2
        sd["timbre_linear.bias"][:n] += 1.0                 # gamma around 1, as the reference initialises it
    return {k: v.float().contiguous() for k, v in sd.items()}


def synth_unit_state_dict(c, seed):
    return _synth(unit_param_shapes(c), seed)


def synth_encoder_state_dict(hp, seed):
    return _synth(encoder_param_shapes(hp), seed)


def synth_decoder_state_dict(hp, seed):
    return _synth(decoder_param_shapes(hp), seed)


def fold(sd):
    """the same state_dict with every weight-normed pair folded into `weight`"""
    out = {}
    for k, v in sd.items():
        if k.endswith("weight_g"):
            continue
        if k.endswith("weight_v"):
            g = sd[k[:-1] + "g"]
            out[k[:-8] + "weight"] = g * v / v.flatten(1).norm(dim=1).reshape(g.shape)
        else:
            out[k] = v
    return out


# ---- the activation and the unit ---------------------------------------------------------------------------------------------------
def up2(x, filt):
    """UpSample1d.forward (resample.py:36-45), ratio 2, 12 taps; filt [12] of x's dtype"""
    Cn = x.shape[1]
    y = Fn.pad(x, (5, 5), mode="replicate")
    y = 2 * Fn.conv_transpose1d(y, filt.reshape(1, 1, 12).expand(Cn, -1, -1), stride=2, groups=Cn)
    return y[..., 15:-15]


def down2(x, filt):
    """DownSample1d.forward (resample.py:62-65, filter.py:92-99)"""
    Cn = x.shape[1]
    y = Fn.pad(x, (5, 6), mode="replicate")
    return Fn.conv1d(y, filt.reshape(1, 1, 12).expand(Cn, -1, -1), stride=2, groups=Cn)


def snake_beta(u, alpha, beta, logscale=True):
    a = alpha.reshape(1, -1, 1)
    b = a if beta is None else beta.reshape(1, -1, 1)
    if logscale:
        a, b = torch.exp(a), torch.exp(b)
    return u + (1.0 / (b + 0.000000001)) * torch.sin(u * a).pow(2)


def activation1d(x, alpha, beta, logscale=True):
    f = FILT.reshape(-1).to(x)
    return down2(snake_beta(up2(x, f), alpha, beta, logscale), f)


def _act_p(P, p, x):
    return activation1d(x, P[p + "act.alpha"], P.get(p + "act.beta"))


def residual_unit(P, p, x, dilation):
    y = Fn.conv1d(_act_p(P, p + "block.0.", x), C.folded(P, p + "block.1."), P[p + "block.1.bias"], dilation=dilation, padding=3 * dilation)
    y = Fn.conv1d(_act_p(P, p + "block.2.", y), C.folded(P, p + "block.3."), P[p + "block.3.bias"])
    return x + y


def encoder_forward(sd, hp, x, dtype=torch.float64):
    P = {k: v.to(dtype) for k, v in sd.items()}
    h = Fn.conv1d(x.to(dtype), C.folded(P, "block.0."), P["block.0.bias"], padding=3)
    for i, stride in enumerate(hp["up_ratios"]):
        for u, dil in enumerate((1, 3, 9)):
            h = residual_unit(P, f"block.{1 + i}.block.{u}.", h, dil)
        h = _act_p(P, f"block.{1 + i}.block.3.", h)
        h = Fn.conv1d(h, C.folded(P, f"block.{1 + i}.block.4."), P[f"block.{1 + i}.block.4.bias"], stride=stride, padding=stride // 2 + stride % 2)
    n = len(hp["up_ratios"])
    return Fn.conv1d(_act_p(P, f"block.{1 + n}.", h), C.folded(P, f"block.{2 + n}."), P[f"block.{2 + n}.bias"], padding=1)


# ---- the three-group quantizer -----------------------------------------------------------------------------------------------------
def group_state_dict(sd, gi, prefix="quantizer."):
    """group gi's levels under codec_ref's keys (quantizers.i.{in_project,out_project,codebook}: the Linear weights as k = 1 convs)"""
    out = {}
    p = f"{prefix}{gi}.layers."
    for k, v in sd.items():
        if not k.startswith(p):
            continue
        k2 = "quantizers." + k[len(p):]
        k2 = k2.replace("in_proj.", "in_project.").replace("out_proj.", "out_project.").replace("_codebook.", "codebook.")
        if k2.endswith("weight_g") or k2.endswith("weight_v") or k2.endswith("project.weight"):
            v = v.unsqueeze(-1)
        out[k2] = v
    return out


def _levels(g, n):
    return g["N"] if n is None else min(int(n), g["N"])


def quantize(sd, hp, x, dtype=torch.float64, n=None, codes=None):
    """FACodecDecoder.quantize (facodec.py:408-445) -> dict(outs, qs [sum n, B, T], quantized_buf: list, groups: codec_ref.rvq_forward's dicts).
    `codes` [sum n, B, T] given: follow those indices"""
    groups = group_hps(hp)
    res, buf, at = [], [], 0
    x = x.to(dtype)
    outs = torch.zeros_like(x)
    for gi, g in enumerate(groups):
        ng = _levels(g, n)
        inp = x if gi < 2 else x - (buf[0] + buf[1])
        r = C.rvq_forward(group_state_dict(sd, gi), g, inp, dtype, ng, codes=None if codes is None else codes[at:at + ng])
        at += ng
        outs = outs + r["zq"]
        buf.append(r["all_q"].sum(0))
        res.append(r)
    return dict(outs=outs, qs=torch.cat([r["codes"] for r in res], 0), quantized_buf=buf, groups=res)


def margin_rule(sd, hp, x, n=None):
    """codec_ref.margin_rule over the three groups: tau = 8 x the largest |dist32 - dist64| of the fp32 restatement walking the fp64 trajectory, over
    every level of every group; a (level, frame) is decided when the fp64 margin of every level up to it in its group exceeds tau -- and, in the
    residual group, when the frame is decided at EVERY level of the prosody and content groups too (their sum is the residual group's input).
    -> (ref64, ref32, tau, decided [sum n, B, T] bool)"""
    r64 = quantize(sd, hp, x, torch.float64, n)
    r32 = quantize(sd, hp, x, torch.float32, n, codes=r64["qs"])
    tau = 8.0 * max(float((a.double() - b).abs().max()) for g32, g64 in zip(r32["groups"], r64["groups"]) for a, b in zip(g32["dist"], g64["dist"]))
    dec = [torch.cumprod((g["margin"] > tau).to(torch.int64), dim=0).bool() for g in r64["groups"]]
    if len(dec) > 2:
        dec[2] = dec[2] & (dec[0][-1] & dec[1][-1])[None]
    return r64, r32, tau, torch.cat(dec, 0)


def vq2emb(sd, hp, vq, dtype=torch.float64, use_residual_code=True):
    """FACodecDecoder.vq2emb (facodec.py:556-566)"""
    groups = group_hps(hp)
    out, at = 0.0, 0
    for gi, g in enumerate(groups):
        if gi == 2 and not use_residual_code:
            break
        out = out + C.vq2emb(group_state_dict(sd, gi), g, vq[at:at + g["N"]], dtype)
        at += g["N"]
    return out


# ---- the timbre path ---------------------------------------------------------------------------------------------------------------
def timbre_encoder(sd, x, dtype=torch.float64, prefix="timbre_encoder."):
    """TransformerEncoder.forward (transformer.py:219-234) on x [B, T, 256], use_cln=False, no padding mask, eval mode.  The position table is
    indexed with x.size(0) of a BATCH-FIRST tensor (transformer.py:50): row pe[b] is added to every frame of item b"""
    P = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    H, nh = TIMBRE_HP["hidden"], TIMBRE_HP["heads"]
    x = x.to(dtype)
    B, T, _ = x.shape
    x = x + P[prefix + "position_emb.pe"][:B]
    for i in range(TIMBRE_HP["layers"]):
        p = f"{prefix}layers.{i}."
        h = Fn.layer_norm(x, (H,), P[p + "ln_1.weight"], P[p + "ln_1.bias"], 1e-5)
        qkv = Fn.linear(h, P[p + "self_attn.in_proj_weight"], P[p + "self_attn.in_proj_bias"])
        q, k, v = (t.reshape(B, T, nh, H // nh).transpose(1, 2) for t in qkv.chunk(3, -1))
        att = torch.softmax((q / math.sqrt(H // nh)) @ k.transpose(-1, -2), dim=-1) @ v
        att = att.transpose(1, 2).reshape(B, T, H)
        x = x + Fn.linear(att, P[p + "self_attn.out_proj.weight"], P[p + "self_attn.out_proj.bias"])
        h = Fn.layer_norm(x, (H,), P[p + "ln_2.weight"], P[p + "ln_2.bias"], 1e-5)
        h = Fn.conv1d(h.transpose(1, 2), P[p + "ffn.ffn_1.weight"], P[p + "ffn.ffn_1.bias"], padding=TIMBRE_HP["kernel"] // 2).transpose(1, 2)
        x = x + Fn.linear(torch.relu(h), P[p + "ffn.ffn_2.weight"], P[p + "ffn.ffn_2.bias"])
    return Fn.layer_norm(x, (H,), P[prefix + "last_ln.weight"], P[prefix + "last_ln.bias"], 1e-5)


def speaker_embedding(sd, x, dtype=torch.float64):
    """facodec.py:467-470: x [B, 256, T] -> spk_embs [B, 256]"""
    return timbre_encoder(sd, x.transpose(1, 2), dtype).mean(dim=1)


# ---- the decoder -------------------------------------------------------------------------------------------------------------------
def decoder_inference(sd, hp, x, spk, dtype=torch.float64):
    """FACodecDecoder.inference (facodec.py:568-576): x [B, 256, T], spk [B, 256] -> wave [B, 1, T * prod(up_ratios)]"""
    P = {k: v.to(dtype) for k, v in sd.items() if not k.startswith("quantizer.") and not k.startswith("timbre_encoder.")}
    x, spk = x.to(dtype), spk.to(dtype)
    style = Fn.linear(spk, P["timbre_linear.weight"], P["timbre_linear.bias"]).unsqueeze(2)
    gamma, beta = style.chunk(2, 1)
    h = Fn.layer_norm(x.transpose(1, 2), (x.shape[1],), None, None, 1e-5).transpose(1, 2)
    h = h * gamma + beta
    h = Fn.conv1d(h, C.folded(P, "model.0."), P["model.0.bias"], padding=3)
    for i, stride in enumerate(hp["up_ratios"]):
        p = f"model.{1 + i}."
        h = _act_p(P, p + "block.0.", h)
        v, g = P[p + "block.1.weight_v"], P[p + "block.1.weight_g"]
        w = g * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)
        h = Fn.conv_transpose1d(h, w, P[p + "block.1.bias"], stride=stride, padding=stride // 2 + stride % 2, output_padding=stride % 2)
        for u, dil in enumerate((1, 3, 9)):
            h = residual_unit(P, f"{p}block.{2 + u}.", h, dil)
    n = len(hp["up_ratios"])
    h = _act_p(P, f"model.{1 + n}.", h)
    return torch.tanh(Fn.conv1d(h, C.folded(P, f"model.{2 + n}."), P[f"model.{2 + n}.bias"], padding=3))


# ---- the derived bound of the f16x3 unit (tests/test_gpu_facodec.py) ----------------------------------------------------------------
def act_with_error(x, alpha, beta, e_in):
    """fp64 Activation1d(x) and a per-element bound of the library's fp32 evaluation of it, given a bound e_in on its input's error.
    Up-sampling FIR: six fma per value, <= 4e-7 of sum |2 f_up| |x|, and e_in passes with the gain sum |2 f_up| of its phase.  Snake
    (tests/test_gpu_codec.py: d_snake, with 1 / b in place of 1 / a): (3.3e-7 + 1.2e-7 |a u|) / b + 2.4e-7 |s|, and an input error passes with
    |1 + (a / b) sin(2 a u)| <= 1 + a / b.  Down-sampling FIR: two chains of six fma and one add, <= 4.5e-7 of sum |f_dn| |s|, and the Snake error
    passes with sum |f_dn|."""
    f = FILT.reshape(-1).double()
    a = torch.exp(alpha.reshape(1, -1, 1))
    b = a if beta is None else torch.exp(beta.reshape(1, -1, 1))
    u = up2(x, f)
    e_u = 4e-7 * up2(x.abs(), f.abs()) + up2(e_in, f.abs())
    s = u + torch.sin(u * a).pow(2) / (b + 1e-9)
    e_s = (1 + a / b) * e_u + (3.3e-7 + 1.2e-7 * (a * u).abs()) / b + 2.4e-7 * s.abs()
    y = down2(s, f)
    return y, down2(e_s, f.abs()) + 4.5e-7 * down2(s.abs(), f.abs())


def unit_bound(sd64, x, dil):
    """fp64 output of the unit and the derived bound of each element: tests/test_gpu_codec.py's unit_bound with Activation1d's two FIR gains
    and Snake's Lipschitz factor in place of the element-wise Snake (a GEMM output is off by 2e-6 sum |w||v| + 3e-7 |sum| plus sum |w| times
    its operand's error; the epilogue adds the residual and stores)"""
    w1, w2 = C.folded(sd64, "block.1."), C.folded(sd64, "block.3.")
    b1, b2 = sd64["block.1.bias"], sd64["block.3.bias"]
    zero = torch.zeros_like(x)
    s1, e1 = act_with_error(x, sd64["block.0.act.alpha"], sd64.get("block.0.act.beta"), zero)
    v = Fn.conv1d(s1, w1, b1, dilation=dil, padding=3 * dil)
    tol1 = 2e-6 * (Fn.conv1d(s1.abs(), w1.abs(), dilation=dil, padding=3 * dil) + b1.abs()[None, :, None]) + 3e-7 * v.abs() \
        + Fn.conv1d(e1, w1.abs(), dilation=dil, padding=3 * dil)
    z, ez = act_with_error(v, sd64["block.2.act.alpha"], sd64.get("block.2.act.beta"), tol1)
    r = Fn.conv1d(z, w2, b2)
    tol2 = Fn.conv1d(ez, w2.abs()) + 2e-6 * (Fn.conv1d(z.abs(), w2.abs()) + b2.abs()[None, :, None]) + 3e-7 * r.abs()
    y = x + r
    return y, tol2 + 1.2e-7 * (x.abs() + r.abs()) + 1.2e-7 * y.abs()
