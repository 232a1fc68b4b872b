"""A plain-torch restatement of VALL-E's ``inference`` / ``continual`` (models/tts/valle/valle.py with modules/transformer/transformer.py,
modules/norms/norm.py, modules/transformer/position_embedding.py) over a ``state_dict``, parametrised by dtype through its weights.  The AR
stage has two paths: ``recompute`` runs the whole decoder over [text | audio] for every new token as the reference does, ``cache`` runs one
prefill and then one column per token against per-layer k / v caches.  Seeded weights and inputs, the exponential-race draw, and the
decidedness measure the goldens are selected by.  Plain torch on whatever device the weights are on; nothing of this package is imported.
tests/golden/make_golden_valle.py pins it to the real class."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5        # layer_norm_eps' default, which VALLE never overrides

# ---- what the goldens were made with (tests/golden/make_golden_valle.py) ----
SD_SEED, IN_SEED = 41, 51
BASE = dict(text_token_num=32, audio_token_num=64, decoder_dim=128, nhead=2, num_decoder_layers=2, norm_first=True, add_prenet=False,
            prefix_mode=0, share_embedding=True, nar_scale_factor=1.0, prepend_bos=False, num_quantizers=4)
# name -> (hp overrides, text length, inference keywords, how the run must end: "eos" (after 10 - 40 new tokens) or "cap")
RUNS = {
    "eos": (dict(), 7, dict(top_k=-100, temperature=1.0), "eos"),
    "cap": (dict(), 2, dict(top_k=10, temperature=0.7), "cap"),
    "topk": (dict(), 8, dict(top_k=10, temperature=0.7), "eos"),
    "pm1": (dict(prefix_mode=1), 6, dict(top_k=-100, temperature=1.0), "eos"),
    "bos": (dict(prepend_bos=True), 7, dict(top_k=10, temperature=0.7), "eos"),
}
PROMPT_FRAMES = 5
EOS_GAIN = 1.5
CONTINUAL_HP = dict(num_quantizers=8)
CONTINUAL_TEXT, CONTINUAL_FRAMES = 6, 12


def make_hp(**over):
    hp = dict(BASE)
    hp.update(over)
    return hp


def state_dict_spec(hp):
    """[(key, shape)] in the order of ``VALLE.state_dict()`` (tests/golden/keys_valle.json pins the keys to the real class)"""
    D, H, V, Tx, nq = hp["decoder_dim"], hp["nhead"], hp["audio_token_num"], hp["text_token_num"], hp["num_quantizers"]
    Dn = int(D * hp["nar_scale_factor"])
    spec = [("ar_text_embedding.word_embeddings.weight", (Tx, D)), ("nar_text_embedding.word_embeddings.weight", (Tx, Dn)),
            ("ar_audio_embedding.word_embeddings.weight", (V + 1 + int(hp["prepend_bos"]), D)), ("ar_text_position.alpha", (1,)),
            ("ar_audio_position.alpha", (1,))]

    def layers(pre, d, n, adaptive):
        out = []
        for i in range(n):
            p = f"{pre}.layers.{i}."
            out += [(p + "self_attn.in_proj_weight", (3 * d, d)), (p + "self_attn.in_proj_bias", (3 * d,)), (p + "self_attn.out_proj.weight", (d, d)),
                    (p + "self_attn.out_proj.bias", (d,)), (p + "linear1.weight", (4 * d, d)), (p + "linear1.bias", (4 * d,)),
                    (p + "linear2.weight", (d, 4 * d)), (p + "linear2.bias", (d,))]
            for nm in ("norm1", "norm2"):
                if adaptive:
                    out += [(p + nm + ".project_layer.weight", (2 * d, d)), (p + nm + ".project_layer.bias", (2 * d,)), (p + nm + ".norm.weight", (d,)),
                            (p + nm + ".norm.bias", (d,))]
                else:
                    out += [(p + nm + ".weight", (d,)), (p + nm + ".bias", (d,))]
        if adaptive:
            out += [(pre + ".norm.project_layer.weight", (2 * d, d)), (pre + ".norm.project_layer.bias", (2 * d,)), (pre + ".norm.norm.weight", (d,)),
                    (pre + ".norm.norm.bias", (d,))]
        else:
            out += [(pre + ".norm.weight", (d,)), (pre + ".norm.bias", (d,))]
        return out

    spec += layers("ar_decoder", D, hp["num_decoder_layers"], False) + [("ar_predict_layer.weight", (V + 1, D))]
    if nq > 1:
        spec += [(f"nar_audio_embeddings.{j}.word_embeddings.weight", (V + 1 if j == 0 else V, Dn)) for j in range(nq)]
        spec += [("nar_text_position.alpha", (1,)), ("nar_audio_position.alpha", (1,))]
        spec += layers("nar_decoder", Dn, int(hp["num_decoder_layers"] * hp["nar_scale_factor"]), True)
        spec += [(f"nar_predict_layers.{j}.weight", (V, Dn)) for j in range(nq - 1)]
        spec += [(f"nar_stage_embeddings.{j}.word_embeddings.weight", (1, Dn)) for j in range(nq - 1)]
    return spec


def state_dict_keys(hp):
    return [k for k, _ in state_dict_spec(hp)]


def synth_state_dict(hp, seed):
    """Weights in the keys' sorted order from one generator: matrices at 1.5 / sqrt(fan_in), embeddings at std 1, the predict layers at
    4 / sqrt(d) (logits a few units apart: a sampler with something to choose from, runs of 10 - 40 tokens), norm weights 1 + 0.1 randn,
    biases 0.1 randn, the AR alphas near 1 and apart, the NAR alphas 1 (they do not train).  The EOS row of the AR predict layer is larger by
    EOS_GAIN, so that EOS wins the arg-max or the draw after some tens of tokens instead of some hundreds.  With ``share_embedding`` the tied pair
    nar_predict_layers[j] / nar_audio_embeddings[j + 2] is ONE tensor under both names."""
    g = torch.Generator().manual_seed(seed)
    spec = dict(state_dict_spec(hp))
    sd = {}
    for key in sorted(spec):
        shape = spec[key]
        r = torch.randn(shape, generator=g)
        if key.endswith(".alpha"):
            sd[key] = 1.0 + 0.25 * r if key.startswith("ar_") else torch.ones(1)
        elif "embedding" in key:
            sd[key] = r
        elif "predict_layer" in key:
            sd[key] = 4.0 / math.sqrt(shape[1]) * r
        elif len(shape) == 1:
            sd[key] = 1.0 + 0.1 * r if key.endswith("weight") else 0.1 * r
        else:
            sd[key] = 1.5 / math.sqrt(shape[1]) * r
    sd["ar_predict_layer.weight"][hp["audio_token_num"]] *= EOS_GAIN
    if hp["share_embedding"]:
        for j in range(hp["num_quantizers"] - 2):
            sd[f"nar_predict_layers.{j}.weight"] = sd[f"nar_audio_embeddings.{j + 2}.word_embeddings.weight"]
    return {k: sd[k] for k in state_dict_keys(hp)}


def cast(sd, dtype, device=None):
    return {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}


def synth_inputs(hp, seed, text_len, frames=PROMPT_FRAMES):
    """(x [1, S], x_lens [1], y [1, frames, nq], enroll_x_lens [1]), int64"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, hp["text_token_num"], (1, text_len), generator=g)
    y = torch.randint(0, hp["audio_token_num"], (1, frames, hp["num_quantizers"]), generator=g)
    return x, torch.tensor([text_len]), y, torch.tensor([min(3, text_len)])


# ---- the modules ------------------------------------------------------------------------------------------------------------------------------
_pe_tables = {}


def sine_pe(rows, d, dtype, device):
    """position_embedding.py:43-48: the table is built in fp32 whatever the model's dtype, then cast.  A row depends on its own position
    alone, so one table of 4000 rows (the reference's initial size) or more is kept per (d, dtype, device) and sliced."""
    key = (d, dtype, str(device))
    t = _pe_tables.get(key)
    if t is None or t.shape[0] < rows:
        n = max(4000, rows)
        pe = torch.zeros(n, d)
        position = torch.arange(0, n, dtype=torch.float32).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        t = _pe_tables[key] = pe.to(device=device, dtype=dtype)
    return t[:rows]


def positioned(sd, emb_key, pos_key, tokens, pos0=0):
    """position(embedding(tokens)) [1, T, d], the positions counted from ``pos0``"""
    e = sd[emb_key + ".word_embeddings.weight"][tokens]
    pe = sine_pe(pos0 + tokens.shape[1], e.shape[-1], e.dtype, e.device)[pos0:]
    return e * 1.0 + sd[pos_key + ".alpha"] * pe[None]


def add_position(sd, pos_key, y_emb):
    pe = sine_pe(y_emb.shape[1], y_emb.shape[-1], y_emb.dtype, y_emb.device)
    return y_emb * 1.0 + sd[pos_key + ".alpha"] * pe[None]


def adaptive_affine(sd, p, stage):
    """weight | bias = project_layer(stage embedding) [1, 2d]"""
    wb = F.linear(stage, sd[p + ".project_layer.weight"], sd[p + ".project_layer.bias"])
    d = wb.shape[-1] // 2
    return wb[..., :d], wb[..., d:]


def fold_affine(sd, p, stage):
    """the host fold of the port (fp64): gamma' = weight * norm.weight, beta' = weight * norm.bias + bias, rounded to the weights' dtype"""
    dt = sd[p + ".norm.weight"].dtype
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith(p)}
    w, b = adaptive_affine(sd64, p, stage.double())
    return (w * sd64[p + ".norm.weight"]).to(dt)[0], (w * sd64[p + ".norm.bias"] + b).to(dt)[0]


def norm(sd, p, x, stage=None, folded=False):
    d = x.shape[-1]
    if stage is None:
        return F.layer_norm(x, (d,), sd[p + ".weight"], sd[p + ".bias"], EPS)
    if folded:
        g, b = fold_affine(sd, p, stage)
        return F.layer_norm(x, (d,), g, b, EPS)
    w, b = adaptive_affine(sd, p, stage)
    return w * F.layer_norm(x, (d,), sd[p + ".norm.weight"], sd[p + ".norm.bias"], EPS) + b


def prefix_lm_hidden(S, T, device):
    """[T, T] bool, True = hidden: text rows (< S) see text only, audio rows see text and the audio up to themselves"""
    j = torch.arange(T, device=device)
    return ~((j[None, :] < S) | ((j[None, :] <= j[:, None]) & (j[:, None] >= S)))


def decoder(sd, pre, x, n_layers, H, hidden=None, cache=None, stage=None, folded=False, final_norm=True):
    """x [1, T, d] -> [1, T, d].  ``hidden`` [T, L] bool.  ``cache``: a list (one dict per layer) holding k, v [1, H, L0, dk] of the columns
    before these, extended by them."""
    B, T, d = x.shape
    dk = d // H
    for i in range(n_layers):
        p = f"{pre}.layers.{i}."
        h = norm(sd, p + "norm1", x, stage, folded)
        qkv = F.linear(h, sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"])
        q, k, v = (t.reshape(B, T, H, dk).transpose(1, 2) for t in qkv.split(d, dim=-1))
        if cache is not None:
            c = cache[i]
            if "k" in c:
                k, v = torch.cat((c["k"], k), 2), torch.cat((c["v"], v), 2)
            c["k"], c["v"] = k, v
        s = torch.matmul(q, k.transpose(2, 3)) / math.sqrt(dk)
        if hidden is not None:
            s = s.masked_fill(hidden[None, None], float("-inf"))
        o = torch.matmul(torch.softmax(s, dim=-1), v).transpose(1, 2).reshape(B, T, d)
        x = x + F.linear(o, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
        h = norm(sd, p + "norm2", x, stage, folded)
        x = x + F.linear(F.relu(F.linear(h, sd[p + "linear1.weight"], sd[p + "linear1.bias"])), sd[p + "linear2.weight"], sd[p + "linear2.bias"])
    return norm(sd, pre + ".norm", x, stage, folded) if final_norm else x


# ---- the sampler (utils/topk_sampling.py with top_p = 1) on ONE row ---------------------------------------------------------------------------
def process(logits, top_k, temperature, gaps=None):
    """logits [V] -> the temperature-scaled, top-k filtered logits.  ``gaps["topk"]``: half the distance of the k-th largest from the next one
    below (an error d in every logit moves a difference by at most 2 d)"""
    l = logits / temperature if temperature != 1.0 else logits.clone()
    if top_k > 0:
        k = min(max(top_k, 1), l.shape[-1])
        kth = torch.topk(l, k)[0][-1]
        if gaps is not None:
            below = l[l < kth]
            if below.numel():
                gaps["topk"] = float(kth - below.max()) / 2
        l = l.masked_fill(l < kth, float("-inf"))
    return l


def race(l, q, gaps=None):
    """the draw torch.multinomial makes, with its noise given: argmax softmax(l) / q, q ~ Exp(1).  ``gaps["race"]``: half the log-ratio of the
    winner to the runner-up"""
    r = torch.softmax(l, -1) / q.to(l.dtype)
    if gaps is not None:
        t = torch.topk(r, 2)[0]
        gaps["race"] = float("inf") if float(t[1]) == 0.0 else float(torch.log(t[0] / t[1])) / 2
    return int(torch.argmax(r))


def argmax_gap(l):
    """half the distance of the largest from the second largest along the last axis, the smallest over the rows"""
    t = torch.topk(l, 2, dim=-1)[0]
    return float((t[..., 0] - t[..., 1]).min()) / 2


# ---- inference / continual --------------------------------------------------------------------------------------------------------------------
def nar_levels(sd, hp, text, text_len, y0, prompts, prefix_len, codes, teacher=None, record=None, folded=False):
    """valle.py:556-605 / 650-701 -- levels 1 .. nq - 1 appended to ``codes``.  ``teacher``: the levels to carry forward instead of the own
    arg-max ([1, n, nq]); ``record``: receives {"nar_logits" [n, V], "gaps"} per level"""
    nq, H = hp["num_quantizers"], int(hp["nhead"] * hp["nar_scale_factor"])
    nl = int(hp["num_decoder_layers"] * hp["nar_scale_factor"])
    emb = lambda j, t: sd[f"nar_audio_embeddings.{j}.word_embeddings.weight"][t]
    x = positioned(sd, "nar_text_embedding", "nar_text_position", text)
    y_emb = emb(0, y0).clone()
    if hp["prefix_mode"] != 0:
        for j in range(1, nq):
            y_emb[:, :prefix_len] += emb(j, prompts[..., j])
    for i in range(nq - 1):
        stage = sd[f"nar_stage_embeddings.{i}.word_embeddings.weight"]
        xy = torch.cat([x, add_position(sd, "nar_audio_position", y_emb)], dim=1)
        xy = decoder(sd, "nar_decoder", xy, nl, H, stage=stage, folded=folded)
        logits = F.linear(xy[:, text_len + prefix_len:], sd[f"nar_predict_layers.{i}.weight"])
        samples = torch.argmax(logits, dim=-1)
        if record is not None:
            record.append({"nar_logits": logits[0], "gaps": {"nar": argmax_gap(logits[0])}})
        codes.append(samples)
        carried = samples if teacher is None else teacher[..., i + 1].to(samples.device)
        if i < nq - 2:
            if hp["prefix_mode"] == 0:
                y_emb[:, :prefix_len] += emb(i + 1, prompts[..., i + 1])
            y_emb[:, prefix_len:] += emb(i + 1, carried)


def inference(sd, hp, x, x_lens, y, enroll_x_lens, draws, top_k=-100, temperature=1.0, path="cache", teacher=None, record=None, folded=False):
    """valle.py:445-608, one sample.  ``draws(step, V)`` -> the step's Exp(1) row.  ``path``: "recompute" (the reference's algorithm) or
    "cache".  ``teacher`` [1, n, nq]: the codes to force (level 0 in the AR stage: it then runs n + 1 steps; the other levels as what the NAR
    stage carries forward).  ``record``: receives {"logits" [V], "gaps", "token"} per AR step, then the NAR levels' entries.
    -> (codes [1, n, nq], how the AR stage ended: "eos", "cap" or "teacher")"""
    H, nl, EOS = hp["nhead"], hp["num_decoder_layers"], hp["audio_token_num"]
    bos = int(hp["prepend_bos"])
    dev = sd["ar_predict_layer.weight"].device
    x, y = x.to(dev), y.to(dev)
    text, text_len = x, int(x_lens.max())
    xe = positioned(sd, "ar_text_embedding", "ar_text_position", text)
    prompts, prefix_len = y, y.shape[1]
    y = prompts[..., 0]
    if bos:
        y = F.pad(y, (1, 0), value=EOS + 1)
    S = text_len
    cache = [dict() for _ in range(nl)] if path == "cache" else None
    step, ended = 0, None
    while True:
        if path == "recompute" or step == 0:
            xy = torch.cat([xe, positioned(sd, "ar_audio_embedding", "ar_audio_position", y)], dim=1)
            h = decoder(sd, "ar_decoder", xy, nl, H, hidden=prefix_lm_hidden(S, xy.shape[1], dev), cache=cache)
        else:
            col = positioned(sd, "ar_audio_embedding", "ar_audio_position", y[:, -1:], pos0=y.shape[1] - 1)
            h = decoder(sd, "ar_decoder", col, nl, H, cache=cache)
        logits = F.linear(h[:, -1], sd["ar_predict_layer.weight"])[0]
        gaps = {"stop": argmax_gap(logits)}
        tok = race(process(logits, top_k, temperature, gaps), draws(step, logits.shape[0]).to(dev), gaps)
        n_new = y.shape[1] - prompts.shape[1]
        if teacher is not None:
            if step >= teacher.shape[1]:
                ended = "teacher"
            else:
                tok = int(teacher[0, step, 0])
        elif int(torch.argmax(logits)) == EOS or tok == EOS:
            ended = "eos"
        elif n_new > S * 16:
            ended = "cap"
        if record is not None:
            record.append({"logits": logits, "gaps": gaps, "token": tok})
        if ended:
            if teacher is None and prompts.shape[1] == y.shape[1]:
                raise SyntaxError("well trained model shouldn't reach here.")
            break
        y = torch.cat([y, torch.tensor([[tok]], dtype=y.dtype, device=dev)], dim=1)
        step += 1
    codes = [y[:, prefix_len + bos:]]
    if hp["num_quantizers"] == 1:
        return torch.stack(codes, dim=-1), ended
    if hp["prefix_mode"] in (2, 4):
        enrolled_len = int(enroll_x_lens.max())
        text = torch.cat([text[:, :1], text[:, enrolled_len - 1:]], dim=1)
        text_len = text_len - (enrolled_len - 2)
    nar_levels(sd, hp, text, text_len, y[:, bos:], prompts, prefix_len, codes, teacher, record, folded)
    return torch.stack(codes, dim=-1), ended


def continual(sd, hp, x, x_lens, y, teacher=None, record=None, folded=False):
    """valle.py:610-704 -> [1, T - prefix_len, 8]"""
    assert hp["num_quantizers"] == 8
    dev = sd["ar_predict_layer.weight"].device
    x, y = x.to(dev), y.to(dev)
    prefix_len = min(int(y.shape[1] * 0.5), 3 * 75)
    prompts = y[:, :prefix_len]
    codes = [y[:, prefix_len:, 0]]
    nar_levels(sd, hp, x, int(x_lens.max()), y[..., 0], prompts, prefix_len, codes, teacher, record, folded)
    return torch.stack(codes, dim=-1)


class Replay:
    """``noise=`` / ``draws=`` from a stored [steps, V] array"""

    def __init__(self, q):
        self.q, self.step = torch.as_tensor(q), 0

    def __call__(self, *a):
        if len(a) == 2:                                   # draws(step, V)
            return self.q[a[0]]
        row = self.q[self.step]                           # noise(shape)
        self.step += 1
        return row.reshape(a[0])


def _tau_gap(r32, r64, temperature):
    n = min(len(r32), len(r64))
    tau, gap = 0.0, float("inf")
    for a, b in zip(r32[:n], r64[:n]):
        key = "logits" if "logits" in a else "nar_logits"
        t = float((a[key].double() - b[key]).abs().max())
        tau = max(tau, t * (max(1.0, 1.0 / temperature) if key == "logits" else 1.0))    # in the units of the processed logits
        gap = min(gap, min(b["gaps"].values()))
    return tau, gap


def decidedness(sd32, sd64, hp, x, x_lens, y, enroll_x_lens, draws, top_k=-100, temperature=1.0, path="cache"):
    """Runs ``inference`` in fp32 and, teacher-forced on the fp32 codes, in fp64 and returns (codes32, ended, tau, gap): tau = the largest
    distance of an fp32 logit (AR steps and NAR levels) from its fp64 value, gap = the smallest distance of any discrete decision of the fp64
    run -- top-k membership, the race's winner, the stop test's arg-max, every NAR arg-max of every level and frame -- from its boundary, in
    the logits' units at that point.  A run is DECIDED when gap >= 4 tau: no evaluation within tau of fp64 takes another branch."""
    r32, r64 = [], []
    codes, ended = inference(sd32, hp, x, x_lens, y, enroll_x_lens, draws, top_k, temperature, path, record=r32)
    inference(sd64, hp, x, x_lens, y, enroll_x_lens, draws, top_k, temperature, path, teacher=codes, record=r64)
    tau, gap = _tau_gap(r32, r64, temperature)
    return codes, ended, tau, gap


def continual_decidedness(sd32, sd64, hp, x, x_lens, y):
    r32, r64 = [], []
    codes = continual(sd32, hp, x, x_lens, y, record=r32)
    continual(sd64, hp, x, x_lens, y, teacher=codes, record=r64)
    tau, gap = _tau_gap(r32, r64, 1.0)
    return codes, tau, gap
