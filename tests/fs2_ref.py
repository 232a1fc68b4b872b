"""FastSpeech2 (models/tts/fastspeech2/fs2.py) and the FFT block (modules/transformer/{Models,Layers,SubLayers,Modules}.py) restated as
plain functions of a state dict, in whatever dtype the state dict and the inputs have: the fp64 evaluation is the reference of the GPU
tests, the fp32 evaluation gives the error scale (tau) of their bounds.  Batch-first [B, T, C] like the reference; eval mode (no dropout,
BatchNorm on its running statistics).  Also: the seeded weights of the small test models and the decision margins of a run (the
distance of every rounded duration from its half-integer and of every scaled prediction from its nearest bin boundary)."""
import math

import numpy as np
import torch
import torch.nn.functional as F


# ---- hyper-parameters and weights -----------------------------------------------------------------------------------------------------
def small_hp(**over):
    """hidden 256 in 2 heads (dk 128), 2 + 2 layers, filter 512, k = (9, 1); predictors 256 x k 3; 256 bins; 20 mel bands; vocabulary 152"""
    hp = dict(hidden=256, heads=2, enc_layers=2, dec_layers=2, d_inner=512, kernel=(9, 1), vp_filter=256, vp_kernel=3, n_bins=256, n_mel=20,
              n_vocab=152, max_seq_len=1000, postnet_dim=512, postnet_k=5, postnet_n=5, n_speaker=0, pitch_level="phoneme_level",
              energy_level="phoneme_level", pitch_quant="linear", energy_quant="linear",
              stats=dict(pitch_min=-2.5, pitch_max=6.0, energy_min=-1.5, energy_max=5.0))
    hp.update(over)
    return hp


def sinusoid_table(n_position, d_hid):
    """get_sinusoid_encoding_table (Models.py:24-44): float64 on the host, then rounded to fp32"""
    pos = np.arange(n_position, dtype=np.float64)[:, None]
    j = np.arange(d_hid)[None, :]
    t = pos / np.power(10000.0, 2 * (j // 2) / d_hid)
    t[:, 0::2] = np.sin(t[:, 0::2])
    t[:, 1::2] = np.cos(t[:, 1::2])
    return torch.from_numpy(t).float()


def bins_of(hp, which):
    lo, hi = hp["stats"][which + "_min"], hp["stats"][which + "_max"]
    if hp[which + "_quant"] == "log":
        return torch.exp(torch.linspace(np.log(lo), np.log(hi), hp["n_bins"] - 1))
    return torch.linspace(lo, hi, hp["n_bins"] - 1)


def param_shapes(hp):
    """name -> shape, the reference's FastSpeech2.state_dict() in its order of registration"""
    C, H, Fi, (k1, k2) = hp["hidden"], hp["heads"], hp["d_inner"], hp["kernel"]
    out = {}

    def fft(pfx):
        for n in ("w_qs", "w_ks", "w_vs"):
            out[f"{pfx}.slf_attn.{n}.weight"], out[f"{pfx}.slf_attn.{n}.bias"] = (C, C), (C,)
        out[f"{pfx}.slf_attn.layer_norm.weight"], out[f"{pfx}.slf_attn.layer_norm.bias"] = (C,), (C,)
        out[f"{pfx}.slf_attn.fc.weight"], out[f"{pfx}.slf_attn.fc.bias"] = (C, C), (C,)
        out[f"{pfx}.pos_ffn.w_1.weight"], out[f"{pfx}.pos_ffn.w_1.bias"] = (Fi, C, k1), (Fi,)
        out[f"{pfx}.pos_ffn.w_2.weight"], out[f"{pfx}.pos_ffn.w_2.bias"] = (C, Fi, k2), (C,)
        out[f"{pfx}.pos_ffn.layer_norm.weight"], out[f"{pfx}.pos_ffn.layer_norm.bias"] = (C,), (C,)

    out["encoder.position_enc"] = (1, hp["max_seq_len"] + 1, C)
    out["encoder.src_word_emb.weight"] = (hp["n_vocab"], C)
    for i in range(hp["enc_layers"]):
        fft(f"encoder.layer_stack.{i}")
    out["variance_adaptor.pitch_bins"], out["variance_adaptor.energy_bins"] = (hp["n_bins"] - 1,), (hp["n_bins"] - 1,)
    Fv, kv = hp["vp_filter"], hp["vp_kernel"]
    for p in ("duration_predictor", "pitch_predictor", "energy_predictor"):
        q = f"variance_adaptor.{p}"
        out[f"{q}.conv_layer.conv1d_1.conv.weight"], out[f"{q}.conv_layer.conv1d_1.conv.bias"] = (Fv, C, kv), (Fv,)
        out[f"{q}.conv_layer.layer_norm_1.weight"], out[f"{q}.conv_layer.layer_norm_1.bias"] = (Fv,), (Fv,)
        out[f"{q}.conv_layer.conv1d_2.conv.weight"], out[f"{q}.conv_layer.conv1d_2.conv.bias"] = (Fv, Fv, kv), (Fv,)
        out[f"{q}.conv_layer.layer_norm_2.weight"], out[f"{q}.conv_layer.layer_norm_2.bias"] = (Fv,), (Fv,)
        out[f"{q}.linear_layer.weight"], out[f"{q}.linear_layer.bias"] = (1, Fv), (1,)
    out["variance_adaptor.pitch_embedding.weight"] = (hp["n_bins"], C)
    out["variance_adaptor.energy_embedding.weight"] = (hp["n_bins"], C)
    out["decoder.position_enc"] = (1, hp["max_seq_len"] + 1, C)
    for i in range(hp["dec_layers"]):
        fft(f"decoder.layer_stack.{i}")
    out["mel_linear.weight"], out["mel_linear.bias"] = (hp["n_mel"], C), (hp["n_mel"],)
    P, kp, n = hp["postnet_dim"], hp["postnet_k"], hp["postnet_n"]
    for i in range(n):
        ci, co = (hp["n_mel"] if i == 0 else P), (hp["n_mel"] if i == n - 1 else P)
        q = f"postnet.convolutions.{i}"
        out[f"{q}.0.conv.weight"], out[f"{q}.0.conv.bias"] = (co, ci, kp), (co,)
        for nm in ("weight", "bias", "running_mean", "running_var"):
            out[f"{q}.1.{nm}"] = (co,)
        out[f"{q}.1.num_batches_tracked"] = ()
    if hp["n_speaker"]:
        out["speaker_emb.weight"] = (hp["n_speaker"], C)
    return out


def synth_state_dict(hp, seed, d_gain=1.3, d_bias=1.2):
    """Seeded weights at 1 / sqrt(fan_in): every LayerNorm / BatchNorm affine and running statistic non-trivial, embedding row 0 non-zero, the
    duration head's gain and bias chosen so that durations spread over roughly 0 .. 8 (a random head gives almost all zeros)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, shape in param_shapes(hp).items():
        leaf = name.rsplit(".", 1)[-1]
        if name.endswith("position_enc"):
            sd[name] = sinusoid_table(shape[1], shape[2])[None]
        elif name.endswith("pitch_bins"):
            sd[name] = bins_of(hp, "pitch")
        elif name.endswith("energy_bins"):
            sd[name] = bins_of(hp, "energy")
        elif leaf == "num_batches_tracked":
            sd[name] = torch.tensor(100, dtype=torch.int64)
        elif leaf == "running_var":
            sd[name] = 0.5 + torch.rand(shape, generator=g)
        elif leaf == "running_mean":
            sd[name] = 0.2 * torch.randn(shape, generator=g)
        elif "layer_norm" in name or name.startswith("postnet") and ".1." in name:      # LayerNorm / BatchNorm affine
            sd[name] = (1.0 + 0.2 * torch.randn(shape, generator=g)) if leaf == "weight" else 0.1 * torch.randn(shape, generator=g)
        elif "embedding" in name or "emb" in name:
            sd[name] = 0.5 * torch.randn(shape, generator=g)
        elif leaf == "bias":
            sd[name] = 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = int(np.prod(shape[1:]))
            sd[name] = torch.randn(shape, generator=g) / math.sqrt(fan_in)
    sd["variance_adaptor.duration_predictor.linear_layer.weight"] *= d_gain
    sd["variance_adaptor.duration_predictor.linear_layer.bias"] += d_bias
    for p in ("pitch_predictor", "energy_predictor"):             # predictions that spread over the bins
        sd[f"variance_adaptor.{p}.linear_layer.weight"] *= 2.0
        sd[f"variance_adaptor.{p}.linear_layer.bias"] += 1.0
    return sd


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


# ---- the functions ----------------------------------------------------------------------------------------------------------------------
def mh_attention_cf(q, k, v, H, mask=None, scale=None):
    """the op under test, channel-first [B, H dk, T]: mask [B, T] True = VALID key"""
    B, C, T = q.shape
    dk = C // H
    qh, kh, vh = (t.reshape(B, H, dk, T).transpose(2, 3) for t in (q, k, v))
    s = qh @ kh.transpose(2, 3) * (1.0 / math.sqrt(dk) if scale is None else scale)
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    o = torch.softmax(s, -1) @ vh
    return o.transpose(2, 3).reshape(B, C, T)


def multi_head_attention(sd, pfx, x, pad, H):
    """MultiHeadAttention.forward (SubLayers.py:34-61) on q = k = v = x [B, T, C]; pad [B, T] True = padded"""
    B, T, C = x.shape
    dk = C // H
    lin = lambda n, t: F.linear(t, sd[f"{pfx}.{n}.weight"], sd[f"{pfx}.{n}.bias"])
    q, k, v = (lin(n, x).view(B, T, H, dk).permute(0, 2, 1, 3) for n in ("w_qs", "w_ks", "w_vs"))
    attn = q @ k.transpose(2, 3) / np.power(dk, 0.5)
    attn = attn.masked_fill(pad[:, None, None, :], float("-inf"))
    o = (torch.softmax(attn, -1) @ v).permute(0, 2, 1, 3).reshape(B, T, C)
    return F.layer_norm(lin("fc", o) + x, (C,), sd[f"{pfx}.layer_norm.weight"], sd[f"{pfx}.layer_norm.bias"])


def fft_block(sd, pfx, x, pad, H):
    """FFTBlock.forward (Layers.py:22-31)"""
    C = x.shape[2]
    x = multi_head_attention(sd, pfx + ".slf_attn", x, pad, H).masked_fill(pad[:, :, None], 0)
    p = pfx + ".pos_ffn"
    k1, k2 = sd[p + ".w_1.weight"].shape[2], sd[p + ".w_2.weight"].shape[2]
    h = F.relu(F.conv1d(x.transpose(1, 2), sd[p + ".w_1.weight"], sd[p + ".w_1.bias"], padding=(k1 - 1) // 2))
    h = F.conv1d(h, sd[p + ".w_2.weight"], sd[p + ".w_2.bias"], padding=(k2 - 1) // 2).transpose(1, 2)
    x = F.layer_norm(h + x, (C,), sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"])
    return x.masked_fill(pad[:, :, None], 0)


def variance_predictor(sd, pfx, x, pad):
    """VariancePredictor.forward (fs2.py:315-323): no mask between the convs"""
    c = pfx + ".conv_layer"
    k = sd[c + ".conv1d_1.conv.weight"].shape[2]
    Fv = sd[c + ".conv1d_1.conv.weight"].shape[0]
    h = F.relu(F.conv1d(x.transpose(1, 2), sd[c + ".conv1d_1.conv.weight"], sd[c + ".conv1d_1.conv.bias"], padding=(k - 1) // 2)).transpose(1, 2)
    h = F.layer_norm(h, (Fv,), sd[c + ".layer_norm_1.weight"], sd[c + ".layer_norm_1.bias"])
    h = F.relu(F.conv1d(h.transpose(1, 2), sd[c + ".conv1d_2.conv.weight"], sd[c + ".conv1d_2.conv.bias"], padding=1)).transpose(1, 2)
    h = F.layer_norm(h, (Fv,), sd[c + ".layer_norm_2.weight"], sd[c + ".layer_norm_2.bias"])
    out = F.linear(h, sd[pfx + ".linear_layer.weight"], sd[pfx + ".linear_layer.bias"]).squeeze(-1)
    return out.masked_fill(pad, 0.0) if pad is not None else out


def pad_mask(lens, max_len=None):
    max_len = int(lens.max()) if max_len is None else int(max_len)
    return torch.arange(max_len, device=lens.device)[None, :] >= lens[:, None]


def _pos(sd, pfx, T, C, max_seq_len, dtype):
    if T > max_seq_len:
        return sinusoid_table(T, C).to(sd[pfx + ".position_enc"])
    return sd[pfx + ".position_enc"][0, :T]


def length_regulate(x, d):
    """LengthRegulator (fs2.py:239-263): d [B, T] float, each truncated by int()"""
    outs = [x[b].repeat_interleave(d[b].clamp(min=0).long(), 0) for b in range(x.shape[0])]
    lens = torch.tensor([o.shape[0] for o in outs], dtype=torch.long, device=x.device)
    L = int(lens.max())
    return torch.stack([F.pad(o, (0, 0, 0, L - o.shape[0])) for o in outs]), lens


def postnet(sd, x, n):
    h = x.transpose(1, 2)
    for i in range(n):
        q = f"postnet.convolutions.{i}"
        k = sd[q + ".0.conv.weight"].shape[2]
        h = F.conv1d(h, sd[q + ".0.conv.weight"], sd[q + ".0.conv.bias"], padding=(k - 1) // 2)
        h = F.batch_norm(h, sd[q + ".1.running_mean"], sd[q + ".1.running_var"], sd[q + ".1.weight"], sd[q + ".1.bias"], False, 0.1, 1e-5)
        if i < n - 1:
            h = torch.tanh(h)
    return h.transpose(1, 2)


def fs2_forward(sd, hp, texts, src_lens, spk=None, p_control=1.0, e_control=1.0, d_control=1.0, durations=None):
    """FastSpeech2.forward (fs2.py:399-460) for inference inputs, in the dtype of ``sd``.  ``durations``: teacher-forced d_rounded.  Returns
    the reference's dict plus ``p_index`` / ``e_index`` (the bin of every scaled prediction) for the margin rule."""
    dtype = sd["mel_linear.weight"].dtype
    C, H = hp["hidden"], hp["heads"]
    Tx = int(max(src_lens))
    src_pad = pad_mask(src_lens, Tx)
    x = sd["encoder.src_word_emb.weight"][texts] + _pos(sd, "encoder", Tx, C, hp["max_seq_len"], dtype)[None]
    for i in range(hp["enc_layers"]):
        x = fft_block(sd, f"encoder.layer_stack.{i}", x, src_pad, H)
    if hp["n_speaker"]:
        x = x + sd["speaker_emb.weight"][spk][:, None, :]
    va = "variance_adaptor"
    out = {}
    log_d = variance_predictor(sd, va + ".duration_predictor", x, src_pad)

    def embed(which, x, pad, control):
        pred = variance_predictor(sd, f"{va}.{which}_predictor", x, pad) * control
        idx = torch.bucketize(pred, sd[f"{va}.{which}_bins"])
        out[which[0] + "_index"] = idx
        return pred, x + sd[f"{va}.{which}_embedding.weight"][idx]

    if hp["pitch_level"] == "phoneme_level":
        p_pred, x = embed("pitch", x, src_pad, p_control)
    if hp["energy_level"] == "phoneme_level":
        e_pred, x = embed("energy", x, src_pad, e_control)
    d_rounded = torch.clamp(torch.round(torch.exp(log_d) - 1) * d_control, min=0) if durations is None else durations.to(dtype)
    x, mel_lens = length_regulate(x, d_rounded)
    mel_pad = pad_mask(mel_lens)
    if hp["pitch_level"] == "frame_level":
        p_pred, x = embed("pitch", x, mel_pad, p_control)
    if hp["energy_level"] == "frame_level":
        e_pred, x = embed("energy", x, mel_pad, e_control)
    Ty = x.shape[1]
    if Ty > hp["max_seq_len"]:
        x = x + _pos(sd, "decoder", Ty, C, hp["max_seq_len"], dtype)[None]
    else:
        x = x + sd["decoder.position_enc"][0, :Ty][None]
    for i in range(hp["dec_layers"]):
        x = fft_block(sd, f"decoder.layer_stack.{i}", x, mel_pad, H)
    mel = F.linear(x, sd["mel_linear.weight"], sd["mel_linear.bias"])
    out.update(output=mel, postnet_output=postnet(sd, mel, hp["postnet_n"]) + mel, p_predictions=p_pred, e_predictions=e_pred,
               log_d_predictions=log_d, d_rounded=d_rounded, src_masks=src_pad, mel_masks=mel_pad, src_lens=src_lens, mel_lens=mel_lens)
    return out


def margins(out64, hp, sd64, src_lens):
    """the smallest distance of a decision of the fp64 run from its boundary: (duration gap, bin gap).  Durations: |exp(log_d) - 1 - (n + 1/2)|
    over the valid phones (a padded phone's log_d is the masked 0: exp(0) - 1 = 0, half a unit from the boundary).  Bins: the distance of
    every scaled prediction -- padded columns included, they are embedded too -- from the nearest boundary."""
    x = torch.exp(out64["log_d_predictions"]) - 1
    d_gap = float(((x - torch.floor(x)) - 0.5).abs().min())
    b_gap = float("inf")
    for which, key in (("pitch", "p_predictions"), ("energy", "e_predictions")):
        bins = sd64[f"variance_adaptor.{which}_bins"]
        b_gap = min(b_gap, float((out64[key][..., None] - bins).abs().min()))
    return d_gap, b_gap


# ---- the config object both the reference's classes and the package's take ---------------------------------------------------------------
class Cfg(dict):
    """answers both ``cfg.a.b`` and ``cfg["a"]`` (Models.py subscripts ``cfg.model``)"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def make_cfg(hp, processed_dir="", dataset="ds"):
    tr = Cfg(encoder_hidden=hp["hidden"], decoder_hidden=hp["hidden"], encoder_layer=hp["enc_layers"], decoder_layer=hp["dec_layers"],
             encoder_head=hp["heads"], decoder_head=hp["heads"], conv_filter_size=hp["d_inner"], conv_kernel_size=list(hp["kernel"]),
             encoder_dropout=0.2, decoder_dropout=0.2)
    model = Cfg(transformer=tr, max_seq_len=hp["max_seq_len"],
                variance_predictor=Cfg(filter_size=hp["vp_filter"], kernel_size=hp["vp_kernel"], dropout=0.5),
                variance_embedding=Cfg(pitch_quantization=hp["pitch_quant"], energy_quantization=hp["energy_quant"], n_bins=hp["n_bins"]))
    pre = Cfg(n_mel=hp["n_mel"], use_frame_pitch=hp["pitch_level"] == "frame_level", use_frame_energy=hp["energy_level"] == "frame_level",
              processed_dir=processed_dir, pitch_dir="pitches", phone_pitch_dir="phone_pitches", energy_dir="energys",
              phone_energy_dir="phone_energys")
    return Cfg(model=model, preprocess=pre, dataset=[dataset], train=Cfg(multi_speaker_training=bool(hp["n_speaker"]), segment_size=32))


def stats_of(hp):
    s = hp["stats"]
    return {"pitch": (s["pitch_min"], s["pitch_max"]), "energy": (s["energy_min"], s["energy_max"])}


def make_inputs(text_len, n_vocab, seed, n_speaker=0):
    g = torch.Generator().manual_seed(int(seed) + 77)
    lens = torch.tensor(text_len, dtype=torch.long)
    texts = torch.randint(1, n_vocab, (len(text_len), int(lens.max())), generator=g)
    texts[pad_mask(lens)] = 0
    spk = torch.randint(0, max(1, n_speaker), (len(text_len),), generator=g)
    return texts, lens, spk


def decided(hp, sd, texts, lens, spk, controls):
    """the margin rule for one run: tau = the fp32 restatement's distance from fp64 on the quantities the decisions read; every duration and
    bin decision of the fp64 run at least 4 tau from its boundary, and the fp32 run takes the same decisions.  -> (ok, tau, d_gap, b_gap, o64, o32)"""
    sd64, sd32 = cast(sd, torch.float64), cast(sd, torch.float32)
    o64 = fs2_forward(sd64, hp, texts, lens, spk, *controls)
    o32 = fs2_forward(sd32, hp, texts, lens, spk, *controls)
    same = (torch.equal(o64["d_rounded"].float(), o32["d_rounded"]) and torch.equal(o64["mel_lens"], o32["mel_lens"])
            and torch.equal(o64["p_index"], o32["p_index"]) and torch.equal(o64["e_index"], o32["e_index"]))
    if not same:
        return False, float("nan"), 0.0, 0.0, o64, o32
    tau_d = float(((torch.exp(o32["log_d_predictions"]) - 1).double() - (torch.exp(o64["log_d_predictions"]) - 1)).abs().max())
    tau_b = max(float((o32[k].double() - o64[k]).abs().max()) for k in ("p_predictions", "e_predictions"))
    d_gap, b_gap = margins(o64, hp, sd64, lens)
    return d_gap >= 4 * tau_d and b_gap >= 4 * tau_b, max(tau_d, tau_b), d_gap / max(tau_d, 1e-300), b_gap / max(tau_b, 1e-300), o64, o32


# ---- JETS inference (models/tts/jets/jets.py:573-621) -------------------------------------------------------------------------------------
JETS_ADIM = 256
JETS_HIFIGAN = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
                    resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]])      # egs/vocoder/gan/hifigan/exp_config.json


def jets_state_dict(hp, seed):
    """FastSpeech2's weights (the parts JETS shares), the alignment module and the two k = 9 embedding convs at 1 / sqrt(fan_in), and the
    generator's seeded weights of oracle/synth.py under ``generator.``"""
    from oracle import synth

    sd = synth_state_dict(hp, seed)
    g = torch.Generator().manual_seed(int(seed) + 4242)
    A = JETS_ADIM
    extra = {"alignment_module.t_conv1": (A, A, 3), "alignment_module.t_conv2": (A, A, 1), "alignment_module.f_conv1": (A, hp["n_mel"], 3),
             "alignment_module.f_conv2": (A, A, 3), "alignment_module.f_conv3": (A, A, 1), "pitch_embed.0": (A, 1, 9), "energy_embed.0": (A, 1, 9)}
    for name, shape in extra.items():
        sd[name + ".weight"] = torch.randn(shape, generator=g) / math.sqrt(shape[1] * shape[2])
        sd[name + ".bias"] = 0.1 * torch.randn(shape[0], generator=g)
    for k, v in synth.synth_state_dict(synth.hifigan_param_shapes(A, JETS_HIFIGAN), int(seed) + 1).items():
        sd["generator." + k] = v
    return sd


def jets_inference(sd, hp, texts, src_lens):
    """Jets.inference in the dtype of ``sd`` -> dict(wav, d_predictions, log_d, mel_lens)"""
    from oracle import vocoder_oracle as vo

    dtype = sd["mel_linear.weight"].dtype
    C, H = hp["hidden"], hp["heads"]
    Tx = int(max(src_lens))
    src_pad = pad_mask(src_lens, Tx)
    hs = sd["encoder.src_word_emb.weight"][texts] + _pos(sd, "encoder", Tx, C, hp["max_seq_len"], dtype)[None]
    for i in range(hp["enc_layers"]):
        hs = fft_block(sd, f"encoder.layer_stack.{i}", hs, src_pad, H)
    va = "variance_adaptor"
    p = variance_predictor(sd, va + ".pitch_predictor", hs, src_pad)
    e = variance_predictor(sd, va + ".energy_predictor", hs, src_pad)
    log_d = variance_predictor(sd, va + ".duration_predictor", hs, src_pad)
    emb = lambda n, t: F.conv1d(t[:, None, :], sd[n + ".0.weight"], sd[n + ".0.bias"], padding=4).transpose(1, 2)
    hs = hs + emb("energy_embed", e) + emb("pitch_embed", p)
    d = torch.clamp(torch.round(log_d.exp() - 1.0), min=0).long()
    hs, mel_lens = length_regulate(hs, d)
    mel_pad = pad_mask(mel_lens)
    Ty = hs.shape[1]
    hs = hs + _pos(sd, "decoder", Ty, C, hp["max_seq_len"], dtype)[None]
    for i in range(hp["dec_layers"]):
        hs = fft_block(sd, f"decoder.layer_stack.{i}", hs, mel_pad, H)
    gen = {k[len("generator."):]: v for k, v in sd.items() if k.startswith("generator.")}
    wav = vo.hifigan_forward(gen, JETS_HIFIGAN, hs.transpose(1, 2), dtype=dtype)
    return dict(wav=wav, d_predictions=d, log_d=log_d, mel_lens=mel_lens)


def jets_decided(hp, sd, texts, lens):
    """the margin rule for the durations of a JETS run -> (ok, tau, gap in tau, o64, o32)"""
    o64, o32 = jets_inference(cast(sd, torch.float64), hp, texts, lens), jets_inference(cast(sd, torch.float32), hp, texts, lens)
    if not torch.equal(o64["d_predictions"], o32["d_predictions"]):
        return False, float("nan"), 0.0, o64, o32
    tau = float(((torch.exp(o32["log_d"]) - 1).double() - (torch.exp(o64["log_d"]) - 1)).abs().max())
    x = torch.exp(o64["log_d"]) - 1
    gap = float(((x - torch.floor(x)) - 0.5).abs().min())
    return gap >= 4 * tau, tau, gap / max(tau, 1e-300), o64, o32
