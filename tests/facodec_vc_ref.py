"""fp64 / fp32 torch restatement of FACodec's voice-conversion classes (models/codec/ns3_codec/facodec.py:602-1219, transformer.py:13-32,
melspec.py:39-102), computed from a state_dict under the reference's keys: the style-adaptive LayerNorm, the conditioned transformer encoder,
MelSpectrogram, FACodecDecoderV2's quantize / vq2emb / inference and FACodecRedecoder's three methods, with seeded synthetic state_dicts and the
three-group margin rule that takes the prosody latent and x separately.  Builds on tests/facodec_ref.py (not edited).  Eval mode."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as Fn

import codec_ref as C
import facodec_ref as R

MEL_HP = dict(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=200, win_size=800, fmin=0, fmax=8000)
N_PROSODY = 20          # mel bands of the prosody feature (facodec.py:822)


def small_redecoder_hp():
    return dict(in_channels=256, upsample_initial_channel=128, up_ratios=[3, 2], vq_num_q_c=2, vq_num_q_p=1, vq_num_q_r=3, vq_dim=256,
                codebook_size_prosody=5, codebook_size_content=6, codebook_size_residual=5)


def recipe_redecoder_hp():
    """the constructor's defaults (the published ns3_facodec_redecoder.bin)"""
    return dict(in_channels=256, upsample_initial_channel=1280, up_ratios=[5, 5, 4, 2], vq_num_q_c=2, vq_num_q_p=1, vq_num_q_r=3, vq_dim=256,
                codebook_size_prosody=10, codebook_size_content=10, codebook_size_residual=10)


# latent seeds of the GPU quantizer tests of FACodecDecoderV2, per frame count, as (x seed, prosody-feature seed): the fp64 reference alone
# leaves at most 2 % of the frames undecided for them (tests/test_oracle_facodec_vc.py)
QUANT_SEEDS = {1: (201, 301), 63: (202, 302), 65: (203, 303)}


# ---- state_dict layouts (the reference's keys and order) ---------------------------------------------------------------------------
def cond_encoder_param_shapes(prefix):
    """TransformerEncoder(use_cln=True): the norms hold a `style` Linear and nothing else"""
    H = R.TIMBRE_HP["hidden"]
    s = {}
    for k, v in R.timbre_param_shapes(prefix).items():
        for ln in ("ln_1.", "ln_2.", "last_ln."):
            if k.endswith(ln + "weight"):
                k, v = k[:-len("weight")] + "style.weight", (2 * H, H)
            elif k.endswith(ln + "bias"):
                k, v = k[:-len("bias")] + "style.bias", (2 * H,)
        s[k] = v
    return s


def encoder_v2_param_shapes(hp):
    s = R.encoder_param_shapes(hp)
    s["mel_transform.mel_basis"] = (MEL_HP["num_mels"], MEL_HP["n_fft"] // 2 + 1)
    s["mel_transform.hann_window"] = (MEL_HP["win_size"],)
    return s


def decoder_v2_param_shapes(hp):
    """FACodecDecoderV2's state_dict without the predictor heads, in the reference's order"""
    s = R.decoder_param_shapes(hp)
    s["melspec_linear.weight"] = (256, N_PROSODY)
    s["melspec_linear.bias"] = (256,)
    s.update(R.timbre_param_shapes("melspec_encoder."))
    return s


def redecoder_param_shapes(hp):
    s = {}
    for name, n, size in (("prosody", hp["vq_num_q_p"], hp["codebook_size_prosody"]), ("content", hp["vq_num_q_c"], hp["codebook_size_content"]),
                          ("residual", hp["vq_num_q_r"], hp["codebook_size_residual"])):
        for i in range(n):
            s[f"{name}_embs.{i}.weight"] = (2 ** size, hp["vq_dim"])
    dec = R.decoder_param_shapes(dict(hp, codebook_dim=8))
    s.update({k: v for k, v in dec.items() if k.startswith("model.")})
    s["timbre_linear.weight"] = dec["timbre_linear.weight"]
    s["timbre_linear.bias"] = dec["timbre_linear.bias"]
    s.update(cond_encoder_param_shapes("timbre_cond_prosody_enc."))
    return s


def mel_buffers():
    """MelSpectrogram's two buffers as the module builds them (melspec.py:64-71); librosa's filterbank is this project's restatement of it,
    which tests/test_oracle_golden.py pins"""
    from amphion_amd.utils.mel import librosa_mel_fn

    mel = librosa_mel_fn(sr=MEL_HP["sampling_rate"], n_fft=MEL_HP["n_fft"], n_mels=MEL_HP["num_mels"], fmin=MEL_HP["fmin"], fmax=MEL_HP["fmax"])
    return torch.from_numpy(mel).float(), torch.hann_window(MEL_HP["win_size"])


def _synth(shapes, seed):
    """facodec_ref._synth, then: the style Linears' scale half around 1 (the reference initialises it to 1), the embedding tables N(0, 1) (the
    magnitude of a latent), the mel buffers as the module builds them"""
    sd = R._synth(shapes, seed)
    g = torch.Generator().manual_seed(seed + 7919)
    for k in sd:
        if k.endswith(".style.bias"):
            sd[k][: sd[k].numel() // 2] += 1.0
        elif "_embs." in k:
            sd[k] = torch.randn(sd[k].shape, generator=g, dtype=torch.float64).float()
    if "mel_transform.mel_basis" in sd:
        sd["mel_transform.mel_basis"], sd["mel_transform.hann_window"] = mel_buffers()
    return sd


def synth_encoder_v2_state_dict(hp, seed):
    return _synth(encoder_v2_param_shapes(hp), seed)


def synth_decoder_v2_state_dict(hp, seed):
    return _synth(decoder_v2_param_shapes(hp), seed)


def synth_redecoder_state_dict(hp, seed):
    return _synth(redecoder_param_shapes(hp), seed)


def synth_codes(hp, B, T, seed):
    """[n_p + n_c + n_r, B, T] int64, every level uniform over its table; the first frame holds 0 and the last the largest index"""
    g = torch.Generator().manual_seed(seed)
    sizes = [hp["codebook_size_prosody"]] * hp["vq_num_q_p"] + [hp["codebook_size_content"]] * hp["vq_num_q_c"] \
        + [hp["codebook_size_residual"]] * hp["vq_num_q_r"]
    vq = torch.stack([torch.randint(0, 2 ** s, (B, T), generator=g) for s in sizes])
    vq[:, 0, 0] = 0
    vq[:, -1, -1] = torch.tensor([2 ** s - 1 for s in sizes])
    return vq


def synth_prosody_feature(B, T, seed):
    """[B, 20, T] in the range of a log-mel: between log(1e-5) and about 2"""
    g = torch.Generator().manual_seed(seed)
    return (-4.0 + 3.0 * torch.randn((B, N_PROSODY, T), generator=g, dtype=torch.float64)).clamp(math.log(1e-5), 3.0).float()


# ---- the style-adaptive LayerNorm and the transformer ----------------------------------------------------------------------------------
def style_layer_norm(x, cond_mean, weight, bias, eps=1e-5):
    """StyleAdaptiveLayerNorm.forward (transformer.py:22-32): x [B, T, d], cond_mean [B, 1, d] = the condition's mean over time"""
    style = Fn.linear(cond_mean, weight, bias)
    gamma, beta = style.chunk(2, -1)
    return gamma * Fn.layer_norm(x, (x.shape[-1],), None, None, eps) + beta


def transformer_encoder(sd, x, dtype=torch.float64, prefix="timbre_encoder.", condition=None):
    """TransformerEncoder.forward (transformer.py:219-234) on x [B, T, 256], no padding mask, eval mode; ``condition`` [B, T, 256]: use_cln=True.
    facodec_ref.timbre_encoder with the norm chosen by the keys (the batch-indexed position table included)"""
    P = {k: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    H, nh = R.TIMBRE_HP["hidden"], R.TIMBRE_HP["heads"]
    x = x.to(dtype)
    B, T, _ = x.shape
    cm = None if condition is None else condition.to(dtype).mean(dim=1, keepdim=True)

    def norm(p, h):
        if cm is None:
            return Fn.layer_norm(h, (H,), P[p + "weight"], P[p + "bias"], 1e-5)
        return style_layer_norm(h, cm, P[p + "style.weight"], P[p + "style.bias"])

    x = x + P[prefix + "position_emb.pe"][:B]
    for i in range(R.TIMBRE_HP["layers"]):
        p = f"{prefix}layers.{i}."
        h = norm(p + "ln_1.", x)
        qkv = Fn.linear(h, P[p + "self_attn.in_proj_weight"], P[p + "self_attn.in_proj_bias"])
        q, k, v = (t.reshape(B, T, nh, H // nh).transpose(1, 2) for t in qkv.chunk(3, -1))
        att = torch.softmax((q / math.sqrt(H // nh)) @ k.transpose(-1, -2), dim=-1) @ v
        att = att.transpose(1, 2).reshape(B, T, H)
        x = x + Fn.linear(att, P[p + "self_attn.out_proj.weight"], P[p + "self_attn.out_proj.bias"])
        h = norm(p + "ln_2.", x)
        h = Fn.conv1d(h.transpose(1, 2), P[p + "ffn.ffn_1.weight"], P[p + "ffn.ffn_1.bias"], padding=R.TIMBRE_HP["kernel"] // 2).transpose(1, 2)
        x = x + Fn.linear(torch.relu(h), P[p + "ffn.ffn_2.weight"], P[p + "ffn.ffn_2.bias"])
    return norm(prefix + "last_ln.", x)


def cond_encoder(sd, x, spk, dtype=torch.float64, prefix="timbre_cond_prosody_enc."):
    """the redecoder's call (facodec.py:703-706): x [B, T, 256], the speaker embedding [B, 256] expanded over time as the condition"""
    return transformer_encoder(sd, x, dtype, prefix, condition=spk.unsqueeze(1).expand(-1, x.shape[1], -1))


# ---- MelSpectrogram ---------------------------------------------------------------------------------------------------------------------
def mel_spectrogram(y, dtype=torch.float64, mel_basis=None, hann_window=None):
    """MelSpectrogram.forward (melspec.py:73-102) for MEL_HP: y [B, L] -> [B, 80, 1 + (L - 200) // 200]"""
    if mel_basis is None:
        mel_basis, hann_window = mel_buffers()
    pad = int((MEL_HP["n_fft"] - MEL_HP["hop_size"]) / 2)
    y = Fn.pad(y.to(dtype).unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, MEL_HP["n_fft"], hop_length=MEL_HP["hop_size"], win_length=MEL_HP["win_size"], window=hann_window.to(dtype), center=False,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    spec = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + 1e-9)
    return torch.log(torch.clamp(torch.matmul(mel_basis.to(dtype), spec), min=1e-5))


def prosody_feature(x, dtype=torch.float64):
    """FACodecEncoderV2.get_prosody_feature (facodec.py:821-822): x [B, 1, L] -> [B, 20, F]"""
    return mel_spectrogram(x.squeeze(1), dtype)[:, :N_PROSODY, :]


# ---- FACodecDecoderV2 -------------------------------------------------------------------------------------------------------------------
def prosody_latent(sd, pf, dtype=torch.float64):
    """facodec.py:1031-1034: pf [B, 20, T] -> melspec_encoder(melspec_linear(pf^T))^T [B, 256, T]"""
    h = Fn.linear(pf.to(dtype).transpose(1, 2), sd["melspec_linear.weight"].to(dtype), sd["melspec_linear.bias"].to(dtype))
    return transformer_encoder(sd, h, dtype, "melspec_encoder.").transpose(1, 2)


def quantize3(sd, hp, xp, x, dtype=torch.float64, n=None, codes=None):
    """FACodecDecoderV2.quantize (facodec.py:1027-1067) past the prosody encoder: the prosody group quantizes xp, the content group x, the
    residual group x - (q_p + q_c).  The result has facodec_ref.quantize's layout"""
    groups = R.group_hps(hp)
    res, buf, at = [], [], 0
    x, xp = x.to(dtype), xp.to(dtype)
    outs = torch.zeros_like(x)
    for gi, g in enumerate(groups):
        ng = R._levels(g, n)
        inp = xp if gi == 0 else x if gi == 1 else x - (buf[0] + buf[1])
        r = C.rvq_forward(R.group_state_dict(sd, gi), g, inp, dtype, ng, codes=None if codes is None else codes[at:at + ng])
        at += ng
        outs = outs + r["zq"]
        buf.append(r["all_q"].sum(0))
        res.append(r)
    return dict(outs=outs, qs=torch.cat([r["codes"] for r in res], 0), quantized_buf=buf, groups=res)


def margin_rule3(sd, hp, xp, x, n=None):
    """facodec_ref.margin_rule for quantize3: the prosody latent xp and x are given separately (the GPU tests pass the HIP prosody latent, so
    that the codes are judged from the very tensor the kernel quantized) -> (ref64, ref32, tau, decided [sum n, B, T] bool)"""
    r64 = quantize3(sd, hp, xp, x, torch.float64, n)
    r32 = quantize3(sd, hp, xp, x, torch.float32, n, codes=r64["qs"])
    tau = 8.0 * max(float((a.double() - b).abs().max()) for g32, g64 in zip(r32["groups"], r64["groups"]) for a, b in zip(g32["dist"], g64["dist"]))
    dec = [torch.cumprod((g["margin"] > tau).to(torch.int64), dim=0).bool() for g in r64["groups"]]
    if len(dec) > 2:
        dec[2] = dec[2] & (dec[0][-1] & dec[1][-1])[None]
    return r64, r32, tau, torch.cat(dec, 0)


def vq2emb_v2(sd, hp, vq, dtype=torch.float64, use_residual=True):
    """FACodecDecoderV2.vq2emb (facodec.py:1179-1189): FACodecDecoder's under the other argument name"""
    return R.vq2emb(sd, hp, vq, dtype, use_residual_code=use_residual)


def styled_inference(sd, hp, x, spk, dtype=torch.float64):
    """FACodecDecoderV2.inference / FACodecRedecoder.inference (facodec.py:1191-1199,761-769): the expression of FACodecDecoder.inference on
    this state_dict's `model` and `timbre_linear`"""
    return R.decoder_inference({k: v for k, v in sd.items() if k.startswith(("model.", "timbre_linear."))}, hp, x, spk, dtype)


# ---- FACodecRedecoder -------------------------------------------------------------------------------------------------------------------
def _emb(sd, name, i, codes, dtype):
    return Fn.embedding(codes, sd[f"{name}_embs.{i}.weight"].to(dtype))            # [B, T, d]


def redecoder_latent(sd, hp, vq, spk, dtype=torch.float64, use_residual_code=False):
    """FACodecRedecoder.forward up to the timbre norm (facodec.py:698-722): x_p + (c_0 + c_1) [+ (r_0 + r_1 + r_2)] -> [B, 256, T]"""
    p, c, r = hp["vq_num_q_p"], hp["vq_num_q_c"], hp["vq_num_q_r"]
    x_p = 0
    for i in range(p):
        x_p = x_p + _emb(sd, "prosody", i, vq[i], dtype)
    x = 0 + cond_encoder(sd, x_p, spk.to(dtype), dtype)
    x_c = 0
    for i in range(c):
        x_c = x_c + _emb(sd, "content", i, vq[p + i], dtype)
    x = x + x_c
    if use_residual_code:
        x_r = 0
        for i in range(r):
            x_r = x_r + _emb(sd, "residual", i, vq[p + c + i], dtype)
        x = x + x_r
    return x.transpose(1, 2)


def redecoder_forward(sd, hp, vq, spk, dtype=torch.float64, use_residual_code=False):
    return styled_inference(sd, hp, redecoder_latent(sd, hp, vq, spk, dtype, use_residual_code), spk, dtype)


def redecoder_vq2emb(sd, hp, vq, spk, dtype=torch.float64, use_residual=True):
    """FACodecRedecoder.vq2emb (facodec.py:734-759): the transformer INSIDE the prosody loop, then one table after another"""
    p, c, r = hp["vq_num_q_p"], hp["vq_num_q_c"], hp["vq_num_q_r"]
    x_t = 0
    for i in range(p):
        x_t = x_t + _emb(sd, "prosody", i, vq[i], dtype)
        x_t = cond_encoder(sd, x_t, spk.to(dtype), dtype)
    out = 0 + x_t
    for i in range(c):
        out = out + _emb(sd, "content", i, vq[p + i], dtype)
    if use_residual:
        for i in range(r):
            out = out + _emb(sd, "residual", i, vq[p + c + i], dtype)
    return out.transpose(1, 2)
