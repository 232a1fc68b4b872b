"""Torch restatement of MaskGCT's decoding-step sampler (models/tts/maskgct/maskgct_t2s.py:14-32 ``top_k`` / ``log`` / ``gumbel_noise`` /
``gumbel_sample``, :319-337), parametrised by dtype through its inputs: what ``amp_mask_sample`` is tested against.  Plain torch on whatever
device and dtype the inputs have; nothing here imports amphion_amd."""
import math

import torch


def top_k_count(V, filter_thres):
    """how many logits stay: the reference's own expression"""
    return math.ceil((1 - filter_thres) * V)


def top_k_filter(logits, k):
    """logits [B, T, V] -> the same with everything but each row's k largest at -inf (``top_k``)"""
    kept = logits.topk(k, dim=-1)
    return torch.full_like(logits, float("-inf")).scatter(2, kept.indices, kept.values)


def gumbel(u, eps=1e-10):
    """``-log(-log(noise))`` with the reference's ``log(t) = torch.log(t + eps)``"""
    return -torch.log(-torch.log(u + eps) + eps)


def noisy(filtered, u, temperature):
    return filtered / max(temperature, 1e-10) + gumbel(u)


def mask_sample(logits, k, u=None, temperature=1.0, score_temperature=None):
    """logits [B, T, V]; u [B, T, V] uniform noise or None (greedy) -> (ids [B, T], score [B, T], filtered, noisy values or None).
    ``score_temperature``: None is the reference (the softmax of the filtered logits as they are); a number is the WRONG variant that takes
    the softmax at that temperature."""
    f = top_k_filter(logits, k)
    y = None if u is None else noisy(f, u, temperature)
    ids = f.argmax(-1) if u is None else y.argmax(-1)
    sm = (f if score_temperature is None else f / score_temperature).softmax(-1)
    return ids, sm.gather(2, ids[..., None])[..., 0], f, y


# ---- the models (models/tts/maskgct/{llama_nar,maskgct_s2a,maskgct_t2s}.py), functional over a state_dict under the reference's keys --------
import numpy as np  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fmt_ref as R  # noqa: E402


def small_hp_s2a():
    """two heads of 64"""
    return dict(num_quantizer=3, hidden_size=128, num_layers=2, num_heads=2, codebook_size=64, cond_codebook_size=97)


def small_hp_t2s():
    """two heads of 96"""
    return dict(hidden_size=192, num_layers=2, num_heads=2, cond_codebook_size=128)


# ---- the shapes and recipes of the goldens (tests/golden/make_golden_maskgct.py) and the inputs, which regenerate from their seeds
GOLDEN_SEED = 71
TP, TT, NPH = 11, 26, 9
S2A_STEPS, S2A_THRES, S2A_TEMP = [4, 2, 1], 0.9, 1.5
T2S_STEPS, T2S_THRES, T2S_TEMP = 5, 0.9, 0.9
RESCALE = 0.75
RUNS = {"s2a_cfg0": ("s2a", 0.0, False), "s2a_cfg25": ("s2a", 2.5, False), "s2a_gt": ("s2a", 2.5, True), "t2s_cfg0": ("t2s", 0.0, False),
        "t2s_cfg25": ("t2s", 2.5, False)}


def diffllama_inputs(hp, T, valid):
    """(x [2, T, C], t [2], cond [2, T, C], x_mask [2, T]: item 1 masked beyond frame ``valid``)"""
    g = torch.Generator().manual_seed(100 + T)
    C = hp["hidden_size"]
    x, t, cond = torch.randn(2, T, C, generator=g), torch.rand(2, generator=g), torch.randn(2, T, C, generator=g)
    mask = torch.ones(2, T)
    mask[1, valid:] = 0
    return x, t, cond, mask


def prefix_inputs(hp, valid):
    """(x [2, 37, C], t [2], phone embedding [2, 9, C], x_mask, phone_mask: item 1 has 7 phones)"""
    g = torch.Generator().manual_seed(200)
    C = hp["hidden_size"]
    x, t, ph = torch.randn(2, 37, C, generator=g), torch.rand(2, generator=g), torch.randn(2, NPH, C, generator=g)
    mask, pmask = torch.ones(2, 37), torch.ones(2, NPH)
    mask[1, valid:] = 0
    pmask[1, 7:] = 0
    return x, t, ph, mask, pmask


def sampler_inputs(kind, hp, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "s2a":
        return dict(codes=torch.randint(0, hp["cond_codebook_size"], (2, TP + TT), generator=g),
                    prompt=torch.randint(0, hp["codebook_size"], (2, TP, hp["num_quantizer"]), generator=g),
                    gt=torch.randint(0, hp["codebook_size"], (2, TT, 1), generator=g))
    return dict(prompt=torch.randint(0, hp["cond_codebook_size"], (2, TP), generator=g), phones=torch.randint(0, 1023, (2, NPH), generator=g))


def golden_run(kind, sd, hp, inp, cfg, gt, noise, dtype=torch.float32, **kw):
    """a golden's recipe through the restatement, in ``dtype``"""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    if kind == "s2a":
        return s2a_reverse_diffusion(sd, hp, sd["cond_emb.weight"][inp["codes"]], inp["prompt"], noise, temp=S2A_TEMP, filter_thres=S2A_THRES,
                                     gt_code=inp["gt"] if gt else None, n_timesteps=S2A_STEPS, cfg=cfg, rescale_cfg=RESCALE, **kw)
    return t2s_reverse_diffusion(sd, hp, inp["prompt"], TT, inp["phones"], noise, temp=T2S_TEMP, filter_thres=T2S_THRES, n_timesteps=T2S_STEPS,
                                 cfg=cfg, rescale_cfg=RESCALE, **kw)


DROPPED = ("rotary_emb.inv_freq", "diff_estimator.embed_tokens.weight")      # keys of the reference that carry nothing of the computation


def _estimator_shapes(hp, cond_mlp=True):
    C, p, out = hp["hidden_size"], "diff_estimator.", {}
    for i in range(hp["num_layers"]):
        q = f"{p}layers.{i}."
        for n in "qkvo":
            out[q + f"self_attn.{n}_proj.weight"] = (C, C)
        out[q + "mlp.gate_proj.weight"] = out[q + "mlp.up_proj.weight"] = (4 * C, C)
        out[q + "mlp.down_proj.weight"] = (C, 4 * C)
        for n in ("input_layernorm", "post_attention_layernorm"):
            out[q + n + ".to_weight.weight"], out[q + n + ".to_weight.bias"] = (C, C), (C,)
    out[p + "norm.to_weight.weight"], out[p + "norm.to_weight.bias"] = (C, C), (C,)
    for m in ("diff_step_mlp",) + (("cond_mlp",) if cond_mlp else ()):
        out[f"{p}{m}.0.weight"], out[f"{p}{m}.0.bias"] = (4 * C, C), (4 * C,)
        out[f"{p}{m}.2.weight"], out[f"{p}{m}.2.bias"] = (C, 4 * C), (C,)
    return out


def state_dict_shapes(kind, hp):
    """key -> shape of what the computation reads, in this package's ``state_dict`` order (tests/golden/keys_maskgct.json pins the keys to the
    real classes)"""
    C = hp["hidden_size"]
    if kind == "s2a":
        Q, V = hp["num_quantizer"], hp["codebook_size"]
        out = {"layer_emb.weight": (Q, C), "mask_emb.weight": (1, C)}
        out.update({f"token_emb.{i}.weight": (V, C) for i in range(Q)})
        for i in range(Q):
            out[f"to_logits.{i}.weight"], out[f"to_logits.{i}.bias"] = (V, C), (V,)
        out["cond_emb.weight"] = (hp["cond_codebook_size"], C)
    else:
        V = hp["cond_codebook_size"]
        out = {"mask_emb.weight": (1, C), "to_logit.weight": (V, C), "to_logit.bias": (V,), "cond_emb.weight": (V, C), "phone_emb.weight": (1024, C)}
    out.update(_estimator_shapes(hp))
    return out


def synth_state_dict(kind, hp, seed):
    """Weights for the tests, in the keys' sorted order from one generator: embeddings at std 0.5, Linear weights at 0.05 (``to_logit(s)`` at 0.1:
    logits of about one unit, so that the top-k filter and the noise both matter), biases at 0.02, ``to_weight`` bias 1 + 0.1 randn"""
    g = torch.Generator().manual_seed(seed)
    shapes = state_dict_shapes(kind, hp)
    sd = {}
    for key in sorted(shapes):
        r = torch.randn(shapes[key], generator=g)
        if "_emb" in key:
            sd[key] = 0.5 * r
        elif "to_weight.bias" in key:
            sd[key] = 1.0 + 0.1 * r
        elif key.endswith("bias"):
            sd[key] = 0.02 * r
        elif key.startswith("to_logit"):
            sd[key] = 0.1 * r
        else:
            sd[key] = 0.05 * r
    return {k: sd[k] for k in shapes}


def _walk(sd, hp, h, t, key_mask, p="diff_estimator."):
    """the layers and the final adaptive norm on h [B, T, C]"""
    H = hp["num_heads"]
    B, T, C = h.shape
    step = R.mlp2(sd, p + "diff_step_mlp", R.sinusoidal_pos_emb(t, C).to(h.dtype))
    cos, sin = R.rope_cos_sin(T, C // H, h.device, h.dtype)
    nw = lambda q: F.linear(step, sd[q + ".to_weight.weight"], sd[q + ".to_weight.bias"])
    heads = lambda y: y.reshape(B, T, H, C // H).transpose(1, 2)
    for i in range(hp["num_layers"]):
        q = f"{p}layers.{i}."
        y = R.adaptive_rms_norm(h, nw(q + "input_layernorm"))
        a = R.rope_attention(heads(F.linear(y, sd[q + "self_attn.q_proj.weight"])), heads(F.linear(y, sd[q + "self_attn.k_proj.weight"])),
                             heads(F.linear(y, sd[q + "self_attn.v_proj.weight"])), cos, sin, key_mask)
        h = h + F.linear(a.transpose(1, 2).reshape(B, T, C), sd[q + "self_attn.o_proj.weight"])
        h = h + R.swiglu_mlp(sd, q + "mlp.", R.adaptive_rms_norm(h, nw(q + "post_attention_layernorm")))
    return R.adaptive_rms_norm(h, nw(p + "norm"))


def diffllama_forward(sd, hp, x, t, cond, x_mask=None):
    """MaskGCT's DiffLlama.forward (llama_nar.py:295-424): x [B, T, C] -> [B, T, C]"""
    return _walk(sd, hp, x + R.mlp2(sd, "diff_estimator.cond_mlp", cond), t, x_mask)


def prefix_forward(sd, hp, x, t, x_mask=None, phone_embedding=None, phone_mask=None):
    """DiffLlamaPrefix.forward (llama_nar.py:522-659)"""
    P = 0
    if phone_embedding is not None:
        pe = R.mlp2(sd, "diff_estimator.cond_mlp", phone_embedding)
        P = pe.shape[1]
        x = torch.cat([pe, x], dim=1)
        if x_mask is not None or phone_mask is not None:
            ones = lambda n: torch.ones(x.shape[0], n, dtype=x.dtype, device=x.device)
            x_mask = torch.cat([ones(P) if phone_mask is None else phone_mask.to(x.dtype), ones(x.shape[1] - P) if x_mask is None else x_mask.to(x.dtype)], 1)
    return _walk(sd, hp, x, t, x_mask)[:, P:]


def next_mask_count(next_t, seq_len):
    """the reference's expression in torch CPU fp32, whatever dtype the restatement runs in"""
    return int((torch.sin(torch.tensor([next_t], dtype=torch.float32) * np.pi / 2) * seq_len).long()[0].item())


def _decode(B, T, steps, V, dtype, build_input, forwards, to_logit, temp, filter_thres, noise, record, k_of, score_temperature, trace, teacher=None):
    """one layer's loop (maskgct_s2a.py:396-464 = maskgct_t2s.py:280-358); ``trace`` receives per step what the decidedness check needs;
    ``teacher``: another run's trace whose ids and masks this run takes over step by step (it then walks that run's trajectory)"""
    k = k_of(V, filter_thres)
    mask = torch.ones(B, T, dtype=torch.bool)
    seq = torch.zeros(B, T, dtype=torch.int64)
    h = 1.0 / steps
    t_list = [1.0 - i * h for i in range(steps)] + [0.0]
    for i in range(steps):
        t = (t_list[i] * torch.ones(B)).to(dtype)
        embeds = forwards(build_input(mask, seq), t)
        if record is not None:
            record.append(embeds.clone())
        logits = to_logit(embeds)
        choice_temp, step_temp = 1.0 * t_list[i], temp * t_list[i]
        u = None
        if not (i == steps - 1 and steps > 1):
            if steps == 1:
                step_temp = 0.2
            u = noise((B, T, V)).to(dtype)
        ids, scores, f, y = mask_sample(logits, k, u, max(step_temp, 1e-3), score_temperature if u is not None else None)
        lead = None if teacher is None else teacher[len(trace)]
        if lead is not None:
            ids = lead["ids"]
        seq = torch.where(mask, ids, seq)
        scores = 1 - (choice_temp * gumbel(noise((B, T)).to(dtype)) + scores)
        n = next_mask_count(t_list[i + 1], T)
        st = dict(logits=logits, k=k, y=y, mask=mask.clone(), n=n, scores=None, ids=ids, mask_next=None, greedy=u is None)
        if trace is not None:
            trace.append(st)
        if n == 0:
            break
        scores = scores.masked_fill(~mask, -torch.finfo(scores.dtype).max)
        st["scores"] = scores
        mask = torch.zeros_like(scores, dtype=torch.bool).scatter(1, scores.topk(n, dim=-1).indices, True)
        if lead is not None:
            mask = lead["mask_next"]
        st["mask_next"] = mask.clone()
        seq = seq.masked_fill(mask, 0)
    return seq


def _guide(embeds, mask_embeds, cfg, rescale_cfg):
    pos_emb_std = embeds.std()
    embeds = embeds + cfg * (embeds - mask_embeds)
    return rescale_cfg * (embeds * pos_emb_std / embeds.std()) + (1 - rescale_cfg) * embeds


def s2a_reverse_diffusion(sd, hp, cond, prompt, noise, x_mask=None, prompt_mask=None, temp=1.5, filter_thres=0.98, max_layer=None, gt_code=None,
                          n_timesteps=(4, 2, 1), cfg=1.0, rescale_cfg=1.0, record=None, k_of=top_k_count, score_temperature=None, trace=None,
                          teacher=None):
    """MaskGCT_S2A.reverse_diffusion (maskgct_s2a.py:317-469); sd and cond in the working dtype; ``noise(shape)`` -> uniform draws"""
    Q, C, V = hp["num_quantizer"], hp["hidden_size"], hp["codebook_size"]
    B, Tp = prompt.shape[:2]
    T = cond.shape[1] - Tp
    dtype = cond.dtype
    one = lambda n: torch.ones(B, n, dtype=dtype)
    x_mask = one(T) if x_mask is None else x_mask.to(dtype)
    prompt_mask = one(Tp) if prompt_mask is None else prompt_mask.to(dtype)
    max_layer = Q if max_layer is None else max_layer
    cum = torch.zeros(B, T, C, dtype=dtype)
    xt = torch.zeros(B, T, max_layer, dtype=torch.int64)
    gt_layer = 0
    if gt_code is not None:
        gt_layer = gt_code.shape[-1]
        xt[:, :, :gt_layer] = gt_code
        for i in range(gt_layer):
            cum = cum + sd[f"token_emb.{i}.weight"][xt[:, :, i]]
    for layer in range(gt_layer, max_layer):
        temp_cond = cond + sd["layer_emb.weight"][layer][None, None, :]
        mask_token = sd["mask_emb.weight"][0][None]
        emb = sd[f"token_emb.{layer}.weight"]
        cur_prompt = 0
        for idx in range(Q):
            cur_prompt = cur_prompt + sd[f"token_emb.{idx}.weight"][prompt[:, :, idx]]
        layer_t = torch.tensor(layer).long().unsqueeze(0)

        def build_input(mask, seq, cum=cum):
            m = mask[..., None]
            cur = cum + m * mask_token[:, None, :] + (~m) * emb[seq]
            return cur + mask_token[:, None, :] * (max_layer - 1 - layer_t)

        def forwards(cur, t):
            embeds = diffllama_forward(sd, hp, torch.cat([cur_prompt, cur], 1), t, temp_cond, torch.cat([prompt_mask, x_mask], 1))[:, Tp:]
            if cfg > 0:
                embeds = _guide(embeds, diffllama_forward(sd, hp, cur, t, temp_cond[:, Tp:], x_mask), cfg, rescale_cfg)
            return embeds

        to_logit = lambda e: F.linear(e, sd[f"to_logits.{layer}.weight"], sd[f"to_logits.{layer}.bias"])
        seq = _decode(B, T, n_timesteps[layer], V, dtype, build_input, forwards, to_logit, temp, filter_thres, noise, record, k_of, score_temperature,
                      trace, teacher)
        cum = cum + emb[seq]
        xt[..., layer] = seq
    return xt


def t2s_reverse_diffusion(sd, hp, prompt, target_len, phone_id, noise, prompt_mask=None, temp=0.9, filter_thres=0.98, n_timesteps=40, cfg=1.0,
                          rescale_cfg=1.0, record=None, k_of=top_k_count, score_temperature=None, trace=None, teacher=None):
    """MaskGCT_T2S.reverse_diffusion (maskgct_t2s.py:225-363)"""
    C, V = hp["hidden_size"], hp["cond_codebook_size"]
    dtype = sd["mask_emb.weight"].dtype
    B, Tp = prompt.shape
    T = target_len
    phone_embedding = sd["phone_emb.weight"][phone_id]
    x_mask = torch.ones(B, T, dtype=dtype)
    phone_mask = torch.ones_like(phone_id)
    prompt_mask = torch.ones(B, Tp, dtype=dtype) if prompt_mask is None else prompt_mask.to(dtype)
    cum = torch.zeros(B, T, C, dtype=dtype)
    mask_token = sd["mask_emb.weight"][0][None]
    cur_prompt = 0 + sd["cond_emb.weight"][prompt]

    def build_input(mask, seq):
        m = mask[..., None]
        return cum + m * mask_token[:, None, :] + (~m) * sd["cond_emb.weight"][seq]

    def forwards(cur, t):
        embeds = prefix_forward(sd, hp, torch.cat([cur_prompt, cur], 1), t, torch.cat([prompt_mask, x_mask], 1), phone_embedding, phone_mask)[:, Tp:]
        if cfg > 0:
            pm = phone_mask[:, Tp:]
            if pm.shape[1]:
                raise ValueError("P > prompt_len: the reference's unconditional branch fails with a shape error")
            embeds = _guide(embeds, prefix_forward(sd, hp, cur, t, x_mask, None, None), cfg, rescale_cfg)
        return embeds

    to_logit = lambda e: F.linear(e, sd["to_logit.weight"], sd["to_logit.bias"])
    return _decode(B, T, n_timesteps, V, dtype, build_input, forwards, to_logit, temp, filter_thres, noise, record, k_of, score_temperature, trace,
                   teacher)


class Replay:
    """``noise(shape)`` that hands back stored draws in order and checks their shapes"""

    def __init__(self, draws):
        self.draws, self.i = list(draws), 0

    def __call__(self, shape):
        u = torch.as_tensor(self.draws[self.i])
        assert tuple(u.shape) == tuple(shape), (self.i, tuple(u.shape), tuple(shape))
        self.i += 1
        return u


def decidedness(run):
    """The decision rule of the sampler tests (tests/codec_ref.py: margin_rule's factor and construction).  ``run(dtype, trace, teacher)``
    executes a restatement on stored noise.  The fp32 restatement walks the fp64 trajectory (same ids and masks); for each of the three
    compared quantities tau = 8 x the largest |fp32 - fp64| along it, and a run is DECIDED when at every step, on every masked frame, the
    fp64 gap between the k-th and (k + 1)-th logit, between the best and second-best sampled value (the noisy value; the logit on a greedy
    step) and -- per item -- at the ``next_mask_num`` boundary of the re-masking scores all exceed their tau.
    -> dict(tau=(logit, noisy, score), worst=(smallest gap / tau of each), undecided=count)"""
    t64, t32 = [], []
    out64 = run(torch.float64, t64, None)
    run(torch.float32, t32, t64)
    fin = lambda a, b: float((a.double() - b)[torch.isfinite(b)].abs().max()) if bool(torch.isfinite(b).any()) else 0.0
    tau_l = 8.0 * max(fin(a["logits"], b["logits"]) for a, b in zip(t32, t64))
    tau_y = 8.0 * max([fin(a["y"], b["y"]) for a, b in zip(t32, t64) if b["y"] is not None] or [0.0])
    tau_s = 8.0 * max([fin(a["scores"][b["mask"]], b["scores"][b["mask"]]) for a, b in zip(t32, t64) if b["scores"] is not None] or [0.0])
    worst, undecided = [float("inf")] * 3, 0
    for b in t64:
        m, k, lg = b["mask"], b["k"], b["logits"]
        srt = lg.sort(-1, descending=True).values
        gaps = []
        if k < lg.shape[-1]:
            gaps.append((0, (srt[..., k - 1] - srt[..., k])[m], tau_l))
        if b["greedy"]:
            gaps.append((1, (srt[..., 0] - srt[..., 1])[m], tau_l))
        elif k > 1:
            top2 = b["y"].topk(2, -1).values
            gaps.append((1, (top2[..., 0] - top2[..., 1])[m], tau_y))
        if b["scores"] is not None:
            cnt = int(m[0].sum())
            assert bool((m.sum(1) == cnt).all())
            if b["n"] < cnt:
                s = b["scores"].sort(-1, descending=True).values
                gaps.append((2, s[:, b["n"] - 1] - s[:, b["n"]], tau_s))
        for which, g, tau in gaps:
            if g.numel():
                worst[which] = min(worst[which], float(g.min()) / max(tau, 1e-300))
                undecided += int((g <= tau).sum())
    return dict(tau=(tau_l, tau_y, tau_s), worst=tuple(worst), undecided=undecided, out=out64)
