"""NaturalSpeech2 inference restated in plain torch, dtype-generic (fp64 is the reference, fp32 on the CPU sets the bounds): the three new
ops (cross-attention with separate query / key lengths, the WaveNet residual layer, the ODE step's element-wise tail) written from the
formulas of include/amphion_hip.h.  Everything is channel-first [B, C, T] like the kernels."""
import math

import torch
import torch.nn.functional as F


# ---- the ops ----------------------------------------------------------------------------------------------------------------------------
def cross_attention_cf(q, k, v, H, mask=None, scale=None):
    """q [B, H dk, Tq], k / v [B, H dk, Tk]; mask [B, Tk] True = VALID key -> [B, H dk, Tq]"""
    B, C, Tq = q.shape
    Tk = k.shape[2]
    dk = C // H
    qh = q.reshape(B, H, dk, Tq).transpose(2, 3)
    kh, vh = (t.reshape(B, H, dk, Tk).transpose(2, 3) for t in (k, v))
    s = qh @ kh.transpose(2, 3) * (1.0 / math.sqrt(dk) if scale is None else scale)
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    o = torch.softmax(s, -1) @ vh
    return o.transpose(2, 3).reshape(B, C, Tq)


def layer_conv(x, dconst, conv_w, conv_b, d, pad_x=False):
    """dilated_conv(x + dconst) with bias: dconst [1 | B, H].  The conv pads y = x + dconst with zeros; ``pad_x`` is the WRONG form that pads
    x and adds dconst to the padding too (what a kernel that stages x and adds the constant afterwards would compute)."""
    if pad_x:
        return F.conv1d(F.pad(x, (d, d)) + dconst[:, :, None], conv_w, conv_b, dilation=d)
    return F.conv1d(x + dconst[:, :, None], conv_w, conv_b, padding=d, dilation=d)


def layer_tail(x, a, cterm, out_w, out_b, film=None, skip=None):
    """everything behind the conv: + cterm, FiLM (film [B, 4H, T] = gain | bias), gate, out_proj, residual | skip -> (x_out, skip_out)"""
    H = x.shape[1]
    a = a + cterm
    if film is not None:
        a = a * film[:, : 2 * H] + film[:, 2 * H:]
    z = torch.sigmoid(a[:, :H]) * torch.tanh(a[:, H:])
    r = F.conv1d(z, out_w.reshape(2 * H, H, 1), out_b)
    x_out = (x + r[:, :H]) / math.sqrt(2.0)
    return x_out, (r[:, H:] if skip is None else skip + r[:, H:])


def ode_step(x_eval, x0_pred, x_base, mean_scale, variance, h_beta, inv_sigma2, mid=False):
    """cal_dxt's tail and the update; the four scalars are Python floats (exact in either dtype)"""
    mean = x0_pred * mean_scale
    logp = -(x_eval - mean) / (variance + 1e-8)
    dxt = (-0.5 * h_beta) * (logp + x_eval * inv_sigma2)
    out = x_base - dxt
    return 0.5 * (out + x_base) if mid else out


# ---- hyper-parameters, the config object, weights -----------------------------------------------------------------------------------------
def small_hp(**over):
    """hidden 128 in 2 heads (dk 64); 2 + 2 encoder layers, filter 256, k 9; predictors of 6 layers (k 3 and k 5), cross-attention every 3rd;
    WaveNet of 6 layers, cross-attention every 3rd, dilation cycle 2; latent 32, 8 query tokens, 64 pitch bins, vocabulary 100, 4 codebooks of
    64 x 32"""
    hp = dict(hidden=128, heads=2, enc_layers=2, d_inner=256, kernel=9, pred_layers=6, dur_kernel=3, pitch_kernel=5, pred_cattn=3,
              wn_layers=6, wn_cattn=3, wn_cycle=2, latent=32, n_query=8, n_bins=64, n_vocab=100, pitch_min=50, pitch_max=1100,
              n_q=4, codebook_size=64, beta_min=0.05, beta_max=20, sigma=1.0, solver="euler", diffusion_type="diffusion")
    hp.update(over)
    return hp


class Cfg(dict):
    """answers ``cfg.a.b`` like the reference's JsonHParams"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def make_cfg(hp):
    """cfg.model of config/ns2.json at the sizes of ``hp`` (+ ``codec``, which only this package reads: the stand-in quantizer's size)"""
    C = hp["hidden"]
    enc = lambda cln: Cfg(encoder_layer=hp["enc_layers"], encoder_hidden=C, encoder_head=hp["heads"], conv_filter_size=hp["d_inner"],
                          conv_kernel_size=hp["kernel"], encoder_dropout=0.2, use_cln=cln)
    pred = lambda k: Cfg(input_size=C, filter_size=C, kernel_size=k, conv_layers=hp["pred_layers"], cross_attn_per_layer=hp["pred_cattn"],
                         attn_head=hp["heads"], drop_out=0.5)
    wn = Cfg(input_size=hp["latent"], hidden_size=C, out_size=hp["latent"], num_layers=hp["wn_layers"], cross_attn_per_layer=hp["wn_cattn"],
             dilation_cycle=hp["wn_cycle"], attn_head=hp["heads"], drop_out=0.2)
    return Cfg(latent_dim=hp["latent"],
               prior_encoder=Cfg(vocab_size=hp["n_vocab"], pitch_min=hp["pitch_min"], pitch_max=hp["pitch_max"], pitch_bins_num=hp["n_bins"],
                                 encoder=enc(True), duration_predictor=pred(hp["dur_kernel"]), pitch_predictor=pred(hp["pitch_kernel"])),
               diffusion=Cfg(wavenet=wn, beta_min=hp["beta_min"], beta_max=hp["beta_max"], sigma=hp["sigma"], noise_factor=1.0,
                             ode_solver=hp["solver"], diffusion_type=hp["diffusion_type"]),
               prompt_encoder=enc(False), query_emb=Cfg(query_token_num=hp["n_query"], hidden_size=C, head_num=hp["heads"]),
               codec=Cfg(n_q=hp["n_q"], codebook_size=hp["codebook_size"], dim=hp["latent"]))


def pe_table(d_model, max_len=5000):
    """PositionalEncoding's buffer [max_len, 1, d]: sin at even, cos at odd channels of position * 10000^(-2i / d)"""
    pos = torch.arange(max_len).unsqueeze(1)
    div = torch.exp(torch.arange(0, d_model, 2) * (-math.log(10000.0) / d_model))
    pe = torch.zeros(max_len, 1, d_model)
    pe[:, 0, 0::2] = torch.sin(pos * div)
    pe[:, 0, 1::2] = torch.cos(pos * div)
    return pe


def pitch_bins(hp):
    import numpy as np

    return torch.exp(torch.linspace(np.log(hp["pitch_min"]), np.log(hp["pitch_max"]), hp["n_bins"] - 1))


def param_shapes(hp):
    """name -> shape of NaturalSpeech2.state_dict()"""
    C, Fi, k, L = hp["hidden"], hp["d_inner"], hp["kernel"], hp["latent"]
    out = {}

    def mha(p):
        out[p + ".in_proj_weight"], out[p + ".in_proj_bias"] = (3 * C, C), (3 * C,)
        out[p + ".out_proj.weight"], out[p + ".out_proj.bias"] = (C, C), (C,)

    def ln(p, cln):
        if cln:
            out[p + ".style.weight"], out[p + ".style.bias"] = (2 * C, C), (2 * C,)
        else:
            out[p + ".weight"], out[p + ".bias"] = (C,), (C,)

    def encoder(p, cln):
        out[p + ".position_emb.pe"] = (5000, 1, C)
        for i in range(hp["enc_layers"]):
            q = f"{p}.layers.{i}"
            ln(q + ".ln_1", cln)
            ln(q + ".ln_2", cln)
            mha(q + ".self_attn")
            out[q + ".ffn.ffn_1.weight"], out[q + ".ffn.ffn_1.bias"] = (Fi, C, k), (Fi,)
            out[q + ".ffn.ffn_2.weight"], out[q + ".ffn.ffn_2.bias"] = (C, Fi), (C,)
        ln(p + ".last_ln", cln)

    def predictor(p, kk):
        for i in range(hp["pred_layers"]):
            out[f"{p}.conv.{i}.0.weight"], out[f"{p}.conv.{i}.0.bias"] = (C, C, kk), (C,)
            out[f"{p}.conv.{i}.2.weight"], out[f"{p}.conv.{i}.2.bias"] = (C,), (C,)
            if i % hp["pred_cattn"] == 0:
                j = i // hp["pred_cattn"]
                mha(f"{p}.cattn.{j}.0")
                out[f"{p}.cattn.{j}.1.weight"], out[f"{p}.cattn.{j}.1.bias"] = (C,), (C,)
        out[p + ".linear.weight"], out[p + ".linear.bias"] = (1, C), (1,)

    out["prior_encoder.enc_emb_tokens.weight"] = (hp["n_vocab"], C)
    out["prior_encoder.encoder.enc_emb_tokens.weight"] = (hp["n_vocab"], C)
    encoder("prior_encoder.encoder", True)
    predictor("prior_encoder.duration_predictor", hp["dur_kernel"])
    predictor("prior_encoder.pitch_predictor", hp["pitch_kernel"])
    out["prior_encoder.pitch_bins"] = (hp["n_bins"] - 1,)
    out["prior_encoder.pitch_embedding.weight"] = (hp["n_bins"], C)
    w = "diffusion.diff_estimator"
    out[w + ".in_proj.weight"], out[w + ".in_proj.bias"] = (C, L, 1), (C,)
    out[w + ".mlp.0.weight"], out[w + ".mlp.0.bias"] = (4 * C, C), (4 * C,)
    out[w + ".mlp.2.weight"], out[w + ".mlp.2.bias"] = (C, 4 * C), (C,)
    out[w + ".cond_ln.weight"], out[w + ".cond_ln.bias"] = (C,), (C,)
    for i in range(hp["wn_layers"]):
        q = f"{w}.layers.{i}"
        out[q + ".dilated_conv.weight"], out[q + ".dilated_conv.bias"] = (2 * C, C, 3), (2 * C,)
        out[q + ".diffusion_proj.weight"], out[q + ".diffusion_proj.bias"] = (C, C), (C,)
        out[q + ".cond_proj.weight"], out[q + ".cond_proj.bias"] = (2 * C, C, 1), (2 * C,)
        out[q + ".out_proj.weight"], out[q + ".out_proj.bias"] = (2 * C, C, 1), (2 * C,)
        if i % hp["wn_cattn"] == 0:
            mha(q + ".attn")
            out[q + ".film.gain.weight"], out[q + ".film.gain.bias"] = (2 * C, C), (2 * C,)
            out[q + ".film.bias.weight"], out[q + ".film.bias.bias"] = (2 * C, C), (2 * C,)
            out[q + ".ln.weight"], out[q + ".ln.bias"] = (C,), (C,)
    out[w + ".skip_proj.weight"], out[w + ".skip_proj.bias"] = (C, C, 1), (C,)
    out[w + ".out_proj.weight"], out[w + ".out_proj.bias"] = (L, C, 1), (L,)
    encoder("prompt_encoder", False)
    out["prompt_lin.weight"], out["prompt_lin.bias"] = (C, L), (C,)
    out["query_emb.weight"] = (hp["n_query"], C)
    mha("query_attn")
    for i in range(hp["n_q"]):
        q = f"quantizer.vq.layers.{i}._codebook"
        out[q + ".inited"], out[q + ".cluster_size"] = (1,), (hp["codebook_size"],)
        out[q + ".embed"], out[q + ".embed_avg"] = (hp["codebook_size"], L), (hp["codebook_size"], L)
    return out


def synth_state_dict(hp, seed, d_gain=0.4, d_bias=1.2, p_gain=0.25):
    """Seeded weights at 1 / sqrt(fan_in) with every norm affine non-trivial; the duration head scaled so that durations spread over 0 .. 10
    (a random head gives almost all zeros) and the pitch head centred on log 250 Hz so that the tokens spread over the bins; the WaveNet's
    out_proj is NOT zero (the reference's initialisation would make every x0 the bias)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, shape in param_shapes(hp).items():
        leaf = name.rsplit(".", 1)[-1]
        if name.endswith(".pe"):
            sd[name] = pe_table(shape[2], shape[0])
        elif name.endswith("pitch_bins"):
            sd[name] = pitch_bins(hp)
        elif name == "prior_encoder.encoder.enc_emb_tokens.weight":
            sd[name] = sd["prior_encoder.enc_emb_tokens.weight"]
        elif leaf == "inited":
            sd[name] = torch.ones(1)
        elif leaf == "cluster_size":
            sd[name] = torch.ones(shape)
        elif leaf == "embed_avg":
            sd[name] = sd[name[: -len("_avg")]].clone()
        elif leaf == "embed":
            sd[name] = torch.randn(shape, generator=g)
        elif leaf == "in_proj_bias" or leaf == "bias" and len(shape) == 1 and not _is_norm(name):
            sd[name] = 0.1 * torch.randn(shape, generator=g)
        elif _is_norm(name):
            sd[name] = (1.0 + 0.2 * torch.randn(shape, generator=g)) if leaf == "weight" else 0.1 * torch.randn(shape, generator=g)
        elif "emb" in name:
            sd[name] = 0.5 * torch.randn(shape, generator=g)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            sd[name] = torch.randn(shape, generator=g) / math.sqrt(fan_in)
    for p in ("prior_encoder.encoder", "prompt_encoder"):       # a style Linear's bias is gamma | beta around 1 | 0
        for k in [k for k in sd if k.startswith(p) and k.endswith(".style.bias")]:
            sd[k][: hp["hidden"]] += 1.0
    for k in [k for k in sd if k.endswith("film.gain.bias")]:
        sd[k] += 1.0
    sd["prior_encoder.duration_predictor.linear.weight"] *= d_gain
    sd["prior_encoder.duration_predictor.linear.bias"] += d_bias
    sd["prior_encoder.pitch_predictor.linear.weight"] *= p_gain
    sd["prior_encoder.pitch_predictor.linear.bias"] += math.log(250.0)
    return sd


def _is_norm(name):
    leafless = name.rsplit(".", 1)[0]
    return (leafless.endswith((".ln_1", ".ln_2", ".last_ln", ".cond_ln", ".ln")) or leafless.rsplit(".", 1)[-1] in ("1", "2") and
            (".cattn." in name or ".conv." in name))


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def make_inputs(hp, seed, n_phones, ref_lens):
    """phone ids [B, N] (equal counts: inference has no phone mask), a prompt latent [B, latent, T'] with NON-zero padded columns and its
    mask [B, T'] (1 = valid), prompt codes [n_q, B, T']"""
    g = torch.Generator().manual_seed(1000 + int(seed))
    B, Tr = len(ref_lens), max(ref_lens)
    phone = torch.randint(1, hp["n_vocab"], (B, n_phones), generator=g)
    codes = torch.randint(0, hp["codebook_size"], (hp["n_q"], B, Tr), generator=g)
    mask = (torch.arange(Tr)[None, :] < torch.tensor(ref_lens)[:, None]).float()
    return phone, codes, mask


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def _ln(x, w=None, b=None, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def mha(sd, p, q, kv, H, valid=None):
    """nn.MultiheadAttention(batch_first) in eval mode: q [B, Tq, C], kv [B, Tk, C] (key = value), valid [B, Tk] True = attend"""
    W, b = sd[p + ".in_proj_weight"], sd[p + ".in_proj_bias"]
    B, Tq, C = q.shape
    Tk, dk = kv.shape[1], C // H
    qq = F.linear(q, W[:C], b[:C]).reshape(B, Tq, H, dk).transpose(1, 2)
    kk = F.linear(kv, W[C:2 * C], b[C:2 * C]).reshape(B, Tk, H, dk).transpose(1, 2)
    vv = F.linear(kv, W[2 * C:], b[2 * C:]).reshape(B, Tk, H, dk).transpose(1, 2)
    s = qq @ kk.transpose(2, 3) / math.sqrt(dk)
    if valid is not None:
        s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, -1) @ vv).transpose(1, 2).reshape(B, Tq, C)
    return F.linear(o, sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"])


def encoder_layer(sd, p, x, H, valid, style_of):
    """one TransformerEncoderLayer: style_of(name) -> (gamma, beta) rows [B, 1, C] for the style-adaptive norm, or None for a plain LayerNorm"""
    def norm(name, t):
        st = style_of(f"{p}.{name}")
        if st is None:
            return _ln(t, sd[f"{p}.{name}.weight"], sd[f"{p}.{name}.bias"])
        return st[0] * _ln(t) + st[1]

    h = norm("ln_1", x)
    x = x + mha(sd, p + ".self_attn", h, h, H, valid)
    h = norm("ln_2", x)
    k = sd[p + ".ffn.ffn_1.weight"].shape[2]
    h = F.relu(F.conv1d(h.transpose(1, 2), sd[p + ".ffn.ffn_1.weight"], sd[p + ".ffn.ffn_1.bias"], padding=k // 2)).transpose(1, 2)
    return x + F.linear(h, sd[p + ".ffn.ffn_2.weight"], sd[p + ".ffn.ffn_2.bias"])


def encoder(sd, p, hp, x, valid, cond=None, cond_valid=None, fix_pe=False, fix_style=False):
    """TransformerEncoder on x [B, T, C].  The reference adds row b of the position table to EVERY frame of item b (``fix_pe``: the table's
    row t to frame t, what the class name promises) and takes the style from the mean of the condition over its whole PADDED length
    (``fix_style``: over the valid frames).  The two "fixed" forms exist to show that the goldens tell them apart."""
    B, T, C = x.shape
    pe = sd[p + ".position_emb.pe"]
    x = x + (pe[:T, 0][None] if fix_pe else pe[:B])
    if cond is None:
        style_of = lambda name: None
    else:
        if fix_style and cond_valid is not None:
            m = cond_valid.to(cond.dtype)[:, :, None]
            mean = (cond * m).sum(1, keepdim=True) / m.sum(1, keepdim=True)
        else:
            mean = cond.mean(1, keepdim=True)

        def style_of(name):
            st = F.linear(mean, sd[name + ".style.weight"], sd[name + ".style.bias"])
            return st[..., :C], st[..., C:]
    for i in range(hp["enc_layers"]):
        x = encoder_layer(sd, f"{p}.layers.{i}", x, hp["heads"], valid, style_of)
    st = style_of(p + ".last_ln")
    return _ln(x, sd[p + ".last_ln.weight"], sd[p + ".last_ln.bias"]) if st is None else st[0] * _ln(x) + st[1]


def predictor(sd, p, hp, x, ref, ref_valid):
    """DurationPredictor / PitchPredictor without a mask: x [B, N, C], ref [B, T', C] -> [B, N]"""
    for i in range(hp["pred_layers"]):
        res = x
        if i % hp["pred_cattn"] == 0:
            q = f"{p}.cattn.{i // hp['pred_cattn']}"
            y = _ln(x, sd[q + ".1.weight"], sd[q + ".1.bias"])
            x = (mha(sd, q + ".0", y, ref, hp["heads"], ref_valid) + x) / math.sqrt(2.0)
        w = sd[f"{p}.conv.{i}.0.weight"]
        x = F.relu(F.conv1d(x.transpose(1, 2), w, sd[f"{p}.conv.{i}.0.bias"], padding=w.shape[2] // 2)).transpose(1, 2)
        x = _ln(x, sd[f"{p}.conv.{i}.2.weight"], sd[f"{p}.conv.{i}.2.bias"])
        if i:
            x = x + res
    return F.linear(x, sd[p + ".linear.weight"], sd[p + ".linear.bias"])[..., 0]


def expand(x, dur):
    """LengthRegulator: x [B, N, C], integer durations [B, N] -> ([B, max, C] zero padded, lengths [B])"""
    rows = [torch.repeat_interleave(x[b], dur[b].clamp(min=0), 0) for b in range(x.shape[0])]
    T = max(r.shape[0] for r in rows)
    return torch.stack([F.pad(r, (0, 0, 0, T - r.shape[0])) for r in rows]), torch.tensor([r.shape[0] for r in rows], device=x.device)


def prior(sd, hp, phone, ref, ref_valid, **fix):
    """PriorEncoder at inference: ref [B, T', C] is the prompt encoder's output (padded frames as they come) -> the dict of the reference"""
    p = "prior_encoder"
    x = F.embedding(phone, sd[p + ".enc_emb_tokens.weight"])
    x = encoder(sd, p + ".encoder", hp, x, None, ref, ref_valid, **fix)
    log_d = predictor(sd, p + ".duration_predictor", hp, x, ref, ref_valid)
    d_round = torch.clamp(torch.round(log_d.exp() - 1), min=0).long()
    x, mel_len = expand(x, d_round)
    pitch_log = predictor(sd, p + ".pitch_predictor", hp, x, ref, ref_valid)
    tok = torch.bucketize(pitch_log.exp(), sd[p + ".pitch_bins"])
    x = x + F.embedding(tok, sd[p + ".pitch_embedding.weight"])
    return dict(dur_pred_round=d_round, dur_pred_log=log_d, dur_pred=log_d.exp() - 1, pitch_pred_log=pitch_log, pitch_token=tok, mel_len=mel_len,
                prior_out=x)


def step_embedding(sd, w, t, dim):
    """SinusoidalPosEmb + mlp (Linear, Mish, Linear): t [n] -> [n, C]"""
    half = dim // 2
    f = torch.exp(torch.arange(half, device=t.device) * -(math.log(10000) / (half - 1))).to(t.dtype)
    e = t[:, None] * f[None, :]
    e = torch.cat((e.sin(), e.cos()), -1)
    h = F.linear(e, sd[w + ".mlp.0.weight"], sd[w + ".mlp.0.bias"])
    h = h * torch.tanh(F.softplus(h))
    return F.linear(h, sd[w + ".mlp.2.weight"], sd[w + ".mlp.2.bias"])


def wavenet(sd, hp, x, cond, t, spk, w="diffusion.diff_estimator"):
    """WaveNet.forward with x_mask = None: x [B, latent, T], cond [B, T, C], t [B], spk [B, Q, C] -> [B, latent, T]"""
    C = hp["hidden"]
    c = _ln(cond, sd[w + ".cond_ln.weight"], sd[w + ".cond_ln.bias"]).transpose(1, 2)
    h = F.relu(F.conv1d(x, sd[w + ".in_proj.weight"], sd[w + ".in_proj.bias"]))
    e = step_embedding(sd, w, t, C)
    skip = None
    for i in range(hp["wn_layers"]):
        q = f"{w}.layers.{i}"
        d = 2 ** (i % hp["wn_cycle"])
        dconst = F.linear(e, sd[q + ".diffusion_proj.weight"], sd[q + ".diffusion_proj.bias"])
        cterm = F.conv1d(c, sd[q + ".cond_proj.weight"], sd[q + ".cond_proj.bias"])
        film = None
        if i % hp["wn_cattn"] == 0:
            y = _ln((h + dconst[:, :, None]).transpose(1, 2), sd[q + ".ln.weight"], sd[q + ".ln.bias"])
            a = mha(sd, q + ".attn", y, spk, hp["heads"])
            film = torch.cat((F.linear(a, sd[q + ".film.gain.weight"], sd[q + ".film.gain.bias"]),
                              F.linear(a, sd[q + ".film.bias.weight"], sd[q + ".film.bias.bias"])), -1).transpose(1, 2)
        a = layer_conv(h, dconst, sd[q + ".dilated_conv.weight"], sd[q + ".dilated_conv.bias"], d)
        h, skip = layer_tail(h, a, cterm, sd[q + ".out_proj.weight"], sd[q + ".out_proj.bias"], film, skip)
    h = skip / math.sqrt(hp["wn_layers"])
    h = F.relu(F.conv1d(h, sd[w + ".skip_proj.weight"], sd[w + ".skip_proj.bias"]))
    return F.conv1d(h, sd[w + ".out_proj.weight"], sd[w + ".out_proj.bias"])


def ode_scalars(hp, t, h):
    """the step's scalars as the reference forms them: fp32 torch on a one-element tensor -> Python floats holding fp32 values"""
    ts = torch.tensor([t], dtype=torch.float32)
    s2 = hp["sigma"] ** 2
    cum_beta = hp["beta_min"] * ts + 0.5 * (hp["beta_max"] - hp["beta_min"]) * (ts ** 2)
    beta_t = hp["beta_min"] + (hp["beta_max"] - hp["beta_min"]) * ts
    return (float(torch.exp(-0.5 * cum_beta / s2)), float(s2 * (1.0 - torch.exp(-cum_beta / s2))), float(h * beta_t),
            float(torch.tensor(1.0 / s2, dtype=torch.float32)))


def step_times(hp, n_steps):
    """the fp32 step times of reverse_diffusion, in the order the WaveNet sees them (midpoint: t, then t + h / 2)"""
    h = 1.0 / max(n_steps, 1)
    one = torch.ones(1, dtype=torch.float32)
    out = []
    for i in range(n_steps):
        t = (1.0 - (i + 0.5) * h) * one
        out.append(float(t))
        if hp["diffusion_type"] == "diffusion" and hp["solver"] == "midpoint":
            out.append(float(t + 0.5 * h))
    return out, h


def reverse_diffusion(sd, hp, z, cond, n_steps, spk):
    times, h = step_times(hp, n_steps)
    xt = z
    B = z.shape[0]
    tt = lambda t: torch.full((B,), t, dtype=z.dtype, device=z.device)
    if hp["diffusion_type"] == "flow":
        for t in times:
            xt = xt - h * wavenet(sd, hp, xt, cond, tt(t), spk)
        return xt
    mid = hp["solver"] == "midpoint"
    for i in range(n_steps):
        t = times[2 * i] if mid else times[i]
        x0 = wavenet(sd, hp, xt, cond, tt(t), spk)
        if not mid:
            xt = ode_step(xt, x0, xt, *ode_scalars(hp, t, h))
            continue
        x_mid = ode_step(xt, x0, xt, *ode_scalars(hp, t, h), mid=True)
        t2 = times[2 * i + 1]
        xt = ode_step(x_mid, wavenet(sd, hp, x_mid, cond, tt(t2), spk), xt, *ode_scalars(hp, t2, h))
    return xt


def code_to_latent(sd, hp, codes):
    """the quantizer's decode: the sum of the look-ups, [n_q, B, T] -> [B, latent, T]"""
    out = 0
    for i in range(codes.shape[0]):
        out = out + F.embedding(codes[i], sd[f"quantizer.vq.layers.{i}._codebook.embed"])
    return out.transpose(1, 2)


def inference(sd, hp, codes, phone, ref_mask, z, n_steps, **fix):
    """NaturalSpeech2.inference with its noise draw given: z is ``torch.randn(B, latent, T)`` BEFORE the division by 1.2 -> (x0, prior_out)"""
    valid = ref_mask.bool()
    ref = F.linear(code_to_latent(sd, hp, codes).transpose(1, 2), sd["prompt_lin.weight"], sd["prompt_lin.bias"])
    ref = encoder(sd, "prompt_encoder", hp, ref, valid, fix_pe=fix.get("fix_pe", False))
    B = ref.shape[0]
    spk = mha(sd, "query_attn", sd["query_emb.weight"][None].expand(B, -1, -1), ref, hp["heads"], valid)
    po = prior(sd, hp, phone, ref, valid, **fix)
    po["spk_query_emb"], po["ref_emb"] = spk, ref
    if z is None:                      # the prior alone (what the decisions read)
        return None, po
    x0 = reverse_diffusion(sd, hp, z / 1.20, po["prior_out"], n_steps, spk)
    return x0, po


def margins(po64, sd64):
    """the smallest distance of a decision of the fp64 run from its boundary: (duration gap, pitch gap).  Durations: |exp(log_d) - 1 -
    (n + 1/2)|; pitch: the distance of exp(pitch_pred_log) from the nearest bin boundary, at every frame (padded frames are embedded too)."""
    x = po64["dur_pred"]
    d_gap = float(((x - torch.floor(x)) - 0.5).abs().min())
    p_gap = float((po64["pitch_pred_log"].exp()[..., None] - sd64["prior_encoder.pitch_bins"]).abs().min())
    return d_gap, p_gap


def decided(sd, hp, codes, phone, ref_mask, z_of, n_steps):
    """Runs the fp64 and the fp32 restatement (z_of(T) -> the noise for T frames) -> (ok, tau, duration gap / tau, pitch gap / tau, out64, out32):
    ok when every decision of the fp64 run is at least 4 tau from its boundary and the fp32 run takes the same decisions.  tau is the fp32
    run's distance from fp64 on the quantity each decision reads (exp(log_d) - 1, exp(pitch_pred_log)), the larger of the two."""
    sd64 = cast(sd, torch.float64)
    x64, p64 = inference(sd64, hp, codes, phone, ref_mask, None, 0)          # zero steps: the prior alone decides
    x32, p32 = inference(sd, hp, codes, phone, ref_mask, None, 0)
    same = all(torch.equal(p64[k], p32[k]) for k in ("dur_pred_round", "mel_len"))
    tau_d = float((p32["dur_pred"].double() - p64["dur_pred"]).abs().max())
    tau_p = float((p32["pitch_pred_log"].double().exp() - p64["pitch_pred_log"].exp()).abs().max()) if same else float("inf")
    same = same and torch.equal(p64["pitch_token"], p32["pitch_token"])
    d_gap, p_gap = margins(p64, sd64)
    ok = same and d_gap >= 4 * tau_d and p_gap >= 4 * tau_p
    return ok, (tau_d, tau_p), d_gap / max(tau_d, 1e-300), p_gap / max(tau_p, 1e-300), p64, p32
