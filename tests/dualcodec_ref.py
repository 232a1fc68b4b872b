"""fp64 / fp32 torch restatement of DualCodec in eval mode (models/codec/dualcodec/dualcodec/model_codec/dualcodec_model.py:30-160,
dac_model.py:172-323, dac_quantize.py:23-262, cnn.py:12-102; the feature preparation of infer/dualcodec/inference_with_semantic.py:155-164,232),
computed from a state_dict, with key / shape lists and seeded synthetic state_dicts.  The quantizer, the decoder stack and the encoder stack are
those of tests/codec_ref.py and tests/dac_ref.py under the DualCodec key names.

The DAC latent is 1024 wide in every net here, the small ones included: ``convnext_decoder`` ends in WNConv1d(convnext_dim, 1024) and its output is
subtracted from the encoder's latent, so the reference itself runs with no other latent_dim (decode_semantic_for_codec=False asserts
convnext_dim == 1024 for the same reason)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as Fn

import codec_ref as C
import dac_ref as D
import vocos_ref as V

SEMANTIC_DIM, INTERMEDIATE = 1024, 2048


# ---- hyperparameters -------------------------------------------------------------------------------------------------------------
def small_hp(is_causal=True):
    """the golden nets (tests/golden/make_golden_dualcodec.py): DualCodec's keyword arguments"""
    return dict(encoder_dim=8, encoder_rates=[2, 3], latent_dim=SEMANTIC_DIM, decoder_dim=64, decoder_rates=[3, 2], n_codebooks=3, codebook_size=64,
                semantic_codebook_size=256, codebook_dim=8, semantic_codebook_dim=8, sample_rate=24000, convnext_dim=64, convnext_layers=2,
                decode_semantic_for_codec=True, is_causal=is_causal, semantic_downsample_factor=2)


def recipe_hp(name):
    """conf/model/dualcodec_12hz_16384_4096_8vq.yaml and dualcodec_25hz_16384_1024_12vq.yaml"""
    common = dict(latent_dim=SEMANTIC_DIM, decoder_dim=1536, semantic_codebook_size=16384, codebook_dim=8, semantic_codebook_dim=8,
                  sample_rate=24000, convnext_dim=768, convnext_layers=4, decode_semantic_for_codec=True, is_causal=True)
    if name == "12hz":
        return dict(common, encoder_dim=32, encoder_rates=[4, 5, 6, 8, 2], decoder_rates=[2, 8, 6, 5, 4], n_codebooks=7, codebook_size=4096,
                    semantic_downsample_factor=4)
    if name == "25hz":
        return dict(common, encoder_dim=64, encoder_rates=[4, 5, 6, 8], decoder_rates=[8, 6, 5, 4], n_codebooks=11, codebook_size=1024,
                    semantic_downsample_factor=2)
    raise KeyError(name)


def hop(hp):
    return int(math.prod(hp["encoder_rates"]))


def encoder_hp(hp):
    return dict(d_model=hp["encoder_dim"], up_ratios=list(hp["encoder_rates"]), out_channels=hp["latent_dim"])


def decoder_hp(hp):
    return dict(input_channel=hp["latent_dim"], channels=hp["decoder_dim"], rates=list(hp["decoder_rates"]), d_out=1)


def acoustic_q_hp(hp):
    return dict(D=hp["latent_dim"], d=hp["codebook_dim"], K=hp["codebook_size"], N=hp["n_codebooks"], l2=True)


def semantic_q_hp(hp):
    return dict(D=hp["convnext_dim"], d=hp["semantic_codebook_dim"], K=hp["semantic_codebook_size"], N=1, l2=True)


# ---- state_dict layouts -----------------------------------------------------------------------------------------------------------
def rvq_param_shapes(qhp, prefix="quantizers."):
    """ResidualVectorQuantize: quantizers.i.{in_proj,out_proj}.{bias,weight_g,weight_v}, quantizers.i.codebook.weight"""
    s = {}
    for i in range(qhp["N"]):
        p = f"{prefix}{i}."
        C._wn(s, p + "in_proj.", qhp["d"], qhp["D"], 1)
        C._wn(s, p + "out_proj.", qhp["D"], qhp["d"], 1)
        s[p + "codebook.weight"] = (qhp["K"], qhp["d"])
    return s


def convnext_block_shapes(dim, prefix, gamma=False):
    s = {}
    if gamma:
        s[prefix + "gamma"] = (dim,)
    s[prefix + "dwconv.weight"] = (dim, 1, 7)
    s[prefix + "dwconv.bias"] = (dim,)
    s[prefix + "norm.weight"] = (dim,)
    s[prefix + "norm.bias"] = (dim,)
    s[prefix + "pwconv1.weight"] = (INTERMEDIATE, dim)
    s[prefix + "pwconv1.bias"] = (INTERMEDIATE,)
    s[prefix + "pwconv2.weight"] = (dim, INTERMEDIATE)
    s[prefix + "pwconv2.bias"] = (dim,)
    return s


def dualcodec_param_shapes(hp):
    """state_dict key -> shape of DualCodec(**hp), in the reference's order (weight-normed form)"""
    s = {}
    s.update({"dac.encoder." + k: v for k, v in C.encoder_param_shapes(encoder_hp(hp)).items()})
    s.update(rvq_param_shapes(acoustic_q_hp(hp), "dac.quantizer.quantizers."))
    s.update({"dac.decoder." + k: v for k, v in D.decoder_param_shapes(decoder_hp(hp)).items()})
    dim, L = hp["convnext_dim"], hp["convnext_layers"]
    C._wn(s, "convnext_encoder.0.", dim, SEMANTIC_DIM, 1)
    for i in range(L):
        s.update(convnext_block_shapes(dim, f"convnext_encoder.{1 + i}."))
    s.update(rvq_param_shapes(semantic_q_hp(hp), "semantic_vq.quantizers."))
    for i in range(L):
        s.update(convnext_block_shapes(dim, f"convnext_decoder.{i}."))
    C._wn(s, f"convnext_decoder.{L}.", SEMANTIC_DIM, dim, 1)
    return s


def synth_convnext_block(dim, prefix, seed, gamma=False):
    """LayerNorm weights 1 + N(0, 0.1), fan-in scaled depthwise / Linear weights, the second Linear at half gain (the block has no layer scale:
    the residual stream would otherwise double per block), biases N(0, 0.05), gamma (when present) 0.5 (1 + N(0, 0.2))"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in convnext_block_shapes(dim, prefix, gamma).items():
        n = torch.randn(shp, generator=g, dtype=torch.float64)
        if k.endswith("gamma"):
            sd[k] = 0.5 * (1 + 0.2 * n)
        elif k.endswith("norm.weight"):
            sd[k] = 1 + 0.1 * n
        elif k.endswith("dwconv.weight"):
            sd[k] = n / math.sqrt(7)
        elif k.endswith("pwconv1.weight"):
            sd[k] = n / math.sqrt(shp[1])
        elif k.endswith("pwconv2.weight"):
            sd[k] = 0.5 * n / math.sqrt(shp[1])
        else:
            sd[k] = 0.05 * n
    return {k: v.float().contiguous() for k, v in sd.items()}


def _wn_conv(prefix, cout, cin, seed):
    s = {}
    C._wn(s, prefix, cout, cin, 1)
    return C._synth(s, seed)


def synth_rvq_state_dict(qhp, seed, prefix="quantizers."):
    return C._synth(rvq_param_shapes(qhp, prefix), seed)


def synth_dualcodec_state_dict(hp, seed):
    """every part from its own seed (seed, seed + 1, ..): encoder, acoustic quantizer, decoder (the calm draw of dac_ref), the two ConvNeXt
    stacks, the semantic quantizer -- assembled in the reference's key order"""
    parts = {}
    parts.update({"dac.encoder." + k: v for k, v in C.synth_encoder_state_dict(encoder_hp(hp), seed).items()})
    parts.update(synth_rvq_state_dict(acoustic_q_hp(hp), seed + 1, "dac.quantizer.quantizers."))
    parts.update({"dac.decoder." + k: v for k, v in D.synth_decoder_state_dict(decoder_hp(hp), seed + 2).items()})
    dim, L = hp["convnext_dim"], hp["convnext_layers"]
    parts.update(_wn_conv("convnext_encoder.0.", dim, SEMANTIC_DIM, seed + 3))
    for i in range(L):
        parts.update(synth_convnext_block(dim, f"convnext_encoder.{1 + i}.", seed + 10 + i))
    parts.update(synth_rvq_state_dict(semantic_q_hp(hp), seed + 4, "semantic_vq.quantizers."))
    for i in range(L):
        parts.update(synth_convnext_block(dim, f"convnext_decoder.{i}.", seed + 30 + i))
    parts.update(_wn_conv(f"convnext_decoder.{L}.", SEMANTIC_DIM, dim, seed + 5))
    return {k: parts[k] for k in dualcodec_param_shapes(hp)}


def synth_inputs(hp, B, T, seed, extra_frames=0):
    """-> (wave [B, 1, (T + extra_frames) * hop], semantic features [B, 1024, T])"""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, SEMANTIC_DIM, T, generator=g).float()
    return C.synth_wave(B, (T + extra_frames) * hop(hp), seed + 1), feats


def synth_hidden(B, T, Cn, seed):
    """w2v-BERT-like hidden states [B, T, C] with per-channel offsets and scales, and their statistics (mean [C], std [C])"""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(Cn, generator=g)
    std = 0.5 + torch.rand(Cn, generator=g)
    return (mean + std * torch.randn(B, T, Cn, generator=g)).float(), mean.float(), std.float()


# ---- the forward passes -----------------------------------------------------------------------------------------------------------
def prepare_semantic_features(hidden, mean, std, factor, dtype=torch.float64):
    x = hidden.to(dtype)
    if mean is not None:
        x = x - mean.to(dtype)
    if std is not None:
        x = x / std.to(dtype)
    return Fn.avg_pool1d(x.transpose(1, 2), factor, factor)


def _linear(P, p, x):
    return torch.einsum("oc,bct->bot", P[p + "weight"], x) + P[p + "bias"][None, :, None]


def convnext_block(P, p, x, causal):
    """cnn.py:84-102 on [B, C, T]"""
    y = Fn.pad(x, (6, 0)) if causal else x
    y = Fn.conv1d(y, P[p + "dwconv.weight"], P[p + "dwconv.bias"], padding=0 if causal else 3, groups=x.shape[1])
    y = V._ln_c(y, P[p + "norm.weight"], P[p + "norm.bias"])
    y = _linear(P, p + "pwconv2.", Fn.gelu(_linear(P, p + "pwconv1.", y)))
    if p + "gamma" in P:
        y = P[p + "gamma"][None, :, None] * y
    return x + y


def dwconv_layer_norm(w, b, lw, lb, x, causal):
    """the front of the block alone (fp64 reference of the fused launch)"""
    y = Fn.pad(x, (6, 0)) if causal else x
    return V._ln_c(Fn.conv1d(y, w, b, padding=0 if causal else 3, groups=x.shape[1]), lw, lb)


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def convnext_encoder(sd, hp, x, dtype=torch.float64):
    P = _cast(sd, dtype)
    h = Fn.conv1d(x.to(dtype), C.folded(P, "convnext_encoder.0."), P["convnext_encoder.0.bias"])
    for i in range(hp["convnext_layers"]):
        h = convnext_block(P, f"convnext_encoder.{1 + i}.", h, hp["is_causal"])
    return h


def convnext_decoder(sd, hp, x, dtype=torch.float64):
    P = _cast(sd, dtype)
    h = x.to(dtype)
    L = hp["convnext_layers"]
    for i in range(L):
        h = convnext_block(P, f"convnext_decoder.{i}.", h, hp["is_causal"])
    return Fn.conv1d(h, C.folded(P, f"convnext_decoder.{L}."), P[f"convnext_decoder.{L}.bias"])


def quantizer_sd(sd, prefix):
    """the keys under `prefix` (".. .quantizers." included) as codec_ref's quantizer functions name them: quantizers.i.in_project / out_project"""
    return {"quantizers." + k[len(prefix):].replace("in_proj.", "in_project.").replace("out_proj.", "out_project."): v
            for k, v in sd.items() if k.startswith(prefix)}


def rvq_forward(qsd, qhp, z, dtype=torch.float64, n=None, codes=None):
    """ResidualVectorQuantize.forward in eval mode on a ``quantizer_sd``: codec_ref.rvq_forward plus latents [B, n * d, T] and z_q_1"""
    r = C.rvq_forward(qsd, qhp, z, dtype, n, codes)
    P = _cast(qsd, dtype)
    residual = z.to(dtype)
    lat = []
    for i in range(r["codes"].shape[0]):
        lat.append(Fn.conv1d(residual, C.folded(P, f"quantizers.{i}.in_project."), P[f"quantizers.{i}.in_project.bias"]))
        residual = residual - r["all_q"][i]
    r["latents"] = torch.cat(lat, 1)
    r["z_q_1"] = r["all_q"][0]
    return r


def rvq_losses(qsd, r):
    """(commitment_loss, codebook_loss): one forward value, sum over levels of mean_b mean_{d,t} (z_e - codebook[code])^2"""
    d = r["latents"].shape[1] // r["codes"].shape[0]
    total = 0.0
    for i in range(r["codes"].shape[0]):
        q = Fn.embedding(r["codes"][i], qsd[f"quantizers.{i}.codebook.weight"].to(r["latents"].dtype)).transpose(1, 2)
        total = total + (r["latents"][:, i * d:(i + 1) * d] - q).pow(2).mean([1, 2]).mean()
    return total


def semantic_quantize(sd, hp, feats, dtype=torch.float64):
    """-> dict(h = convnext_encoder output, r = the one-level rvq_forward result, codes [B, T])"""
    h = convnext_encoder(sd, hp, feats, dtype)
    r = rvq_forward(quantizer_sd(sd, "semantic_vq.quantizers."), semantic_q_hp(hp), h, dtype)
    return dict(h=h, r=r, codes=r["codes"][0])


def semantic_latent(sd, hp, zq, dtype=torch.float64):
    return convnext_decoder(sd, hp, zq, dtype) if hp["decode_semantic_for_codec"] else zq.to(dtype)


def preprocess(hp, audio):
    length = audio.shape[-1]
    return Fn.pad(audio, (0, math.ceil(length / hop(hp)) * hop(hp) - length))


def dac_latent(sd, hp, audio, dtype=torch.float64):
    esd = {k[len("dac.encoder."):]: v for k, v in sd.items() if k.startswith("dac.encoder.")}
    return C.encoder_forward(esd, encoder_hp(hp), preprocess(hp, audio), dtype)


def encode(sd, hp, audio, feats, dtype=torch.float64, num_quantizers=None):
    """DualCodec.encode -> dict(semantic_codes [B, 1, T], acoustic_codes [B, n - 1, T] or None, semantic = the subtracted latent, z_enc = the
    DAC encoder's latent, z = z_q + semantic, r = the acoustic rvq_forward result)"""
    s = semantic_quantize(sd, hp, feats, dtype)
    semantic = semantic_latent(sd, hp, s["r"]["zq"], dtype)
    out = dict(semantic_codes=s["codes"][:, None, :], semantic=semantic, acoustic_codes=None)
    if num_quantizers == 1:
        return out
    n = None if num_quantizers is None else num_quantizers - 1
    z_enc = dac_latent(sd, hp, audio, dtype)
    assert 0 <= z_enc.shape[-1] - semantic.shape[-1] <= 2
    r = rvq_forward(quantizer_sd(sd, "dac.quantizer.quantizers."), acoustic_q_hp(hp), z_enc[..., : semantic.shape[-1]] - semantic, dtype, n)
    out.update(z_enc=z_enc, r=r, z=r["zq"] + semantic, acoustic_codes=r["codes"].transpose(0, 1))
    return out


def decode_from_codes(sd, hp, semantic_codes, acoustic_codes, dtype=torch.float64, pre_tanh=False):
    """DualCodec.decode_from_codes: codes [B, 1, T] / [B, n, T] or None -> wave"""
    semantic = C.vq2emb(quantizer_sd(sd, "semantic_vq.quantizers."), semantic_q_hp(hp), semantic_codes.transpose(0, 1), dtype)
    semantic = semantic_latent(sd, hp, semantic, dtype)
    z = semantic
    if acoustic_codes is not None:
        z = C.vq2emb(quantizer_sd(sd, "dac.quantizer.quantizers."), acoustic_q_hp(hp), acoustic_codes.transpose(0, 1), dtype,
                     n=acoustic_codes.shape[1]) + semantic
    dsd = {k[len("dac.decoder."):]: v for k, v in sd.items() if k.startswith("dac.decoder.")}
    return D.decoder_forward(dsd, decoder_hp(hp), z, dtype, pre_tanh=pre_tanh)


# ---- the quantizer cases of tests/test_gpu_dualcodec.py (tests/test_oracle_dualcodec.py checks the margin rule's cap on each, on the CPU) ------
FVQ_OP_CASES = {"small": (dict(D=64, d=8, K=64, N=3, l2=True), 811), "semantic": (dict(D=768, d=8, K=256, N=1, l2=True), 812)}
FVQ_OP_LENGTHS = (9, 33)
MODEL_SEED, MODEL_LENGTHS = 700, (9, 33)


def fvq_op_inputs(name, T, B=2):
    """-> (quantizer hp, state_dict under "quantizers.", z [B, D, T + 2] of which the first T columns count, sub [B, D, T])"""
    qhp, seed = FVQ_OP_CASES[name]
    return qhp, synth_rvq_state_dict(qhp, seed), C.synth_latent(B, qhp["D"], T + 2, seed + T), 0.5 * C.synth_latent(B, qhp["D"], T, seed + 100 + T)


def model_inputs(hp, T, B=2, extra_frames=0):
    return synth_inputs(hp, B, T, MODEL_SEED + 10 + T, extra_frames)
