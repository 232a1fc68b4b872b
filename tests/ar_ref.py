"""A plain-torch restatement of Vevo's autoregressive transformer (models/vc/autoregressive_transformer/ar_model.py: ``AutoregressiveTransformer``
around HF's ``LlamaForCausalLM``) and of the sampling chain ``generate(do_sample=True)`` runs, parametrised by dtype through its inputs:
the model forward, the cached decode, HF's processors and warpers in their order, the exponential-race draw, ``generate`` with its two
stopping rules, seeded weights and inputs, and the decidedness measure the goldens and the sampler tests are selected by.  Plain torch on
whatever device the inputs are on; nothing of ``transformers`` or of this package is imported.  tests/golden/make_golden_ar.py pins it to
the real class."""
import math

import torch
import torch.nn.functional as F

import fmt_ref as R

EPS = 1e-6        # LlamaConfig.rms_norm_eps' default

# ---- what the goldens were made with (tests/golden/make_golden_ar.py) ----
SD_SEED, FWD_SEED, GEN_SEED = 11, 21, 31
MAX_LENGTH, MIN_NEW = 80, 10
# name -> (dk, generate keywords, how the run must end)
RUNS = {
    "eos96": (96, dict(temperature=0.8, top_k=50, top_p=0.9, repeat_penalty=1.1), "eos"),
    "max96": (96, dict(temperature=0.8, top_k=50, top_p=0.9, repeat_penalty=1.0), "max"),
    "topp1_96": (96, dict(temperature=1.0, top_k=20, top_p=1.0, repeat_penalty=1.0), None),
    "pen64": (64, dict(temperature=0.8, top_k=50, top_p=0.9, repeat_penalty=1.1), None),
}


def small_hp(dk=96):
    """the goldens' models: two heads of ``dk``, two layers"""
    return dict(input_vocab_size=40, output_vocab_size=90, hidden_size=2 * dk, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2)


def special(hp):
    pad = hp["input_vocab_size"] + hp["output_vocab_size"]
    return dict(pad=pad, input_bos=pad + 1, input_eos=pad + 2, output_bos=pad + 3, output_eos=pad + 4, vocab=pad + 20)


def state_dict_keys(hp):
    """``AutoregressiveTransformer.state_dict()`` in the reference's order (tests/golden/keys_ar.json pins it to the real class)"""
    keys = ["model.model.embed_tokens.weight"]
    for i in range(hp["num_hidden_layers"]):
        p = f"model.model.layers.{i}."
        keys += [p + f"self_attn.{n}_proj.weight" for n in "qkvo"]
        keys += [p + f"mlp.{n}_proj.weight" for n in ("gate", "up", "down")]
        keys += [p + "input_layernorm.weight", p + "post_attention_layernorm.weight"]
    return keys + ["model.model.norm.weight", "model.lm_head.weight"]


def _shape(hp, key):
    C, I, V = hp["hidden_size"], hp["intermediate_size"], special(hp)["vocab"]
    if key.endswith("embed_tokens.weight") or key.endswith("lm_head.weight"):
        return (V, C)
    if "layernorm" in key or key.endswith("norm.weight"):
        return (C,)
    if "gate_proj" in key or "up_proj" in key:
        return (I, C)
    if "down_proj" in key:
        return (C, I)
    return (C, C)


def synth_state_dict(hp, seed):
    """Weights in the keys' sorted order from one generator: Linear weights at 1.5 / sqrt(fan_in), the embedding at std 1, the lm_head at
    4 / sqrt(C) (logits a few units apart: a sampler with something to choose from), norm weights 1 + 0.1 randn"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key in sorted(state_dict_keys(hp)):
        shape = _shape(hp, key)
        r = torch.randn(shape, generator=g)
        if len(shape) == 1:
            sd[key] = 1.0 + 0.1 * r
        elif key.endswith("embed_tokens.weight"):
            sd[key] = r
        elif key.endswith("lm_head.weight"):
            sd[key] = 4.0 / math.sqrt(shape[1]) * r
        else:
            sd[key] = 1.5 / math.sqrt(shape[1]) * r
    return {k: sd[k] for k in state_dict_keys(hp)}


def cast(sd, dtype, device=None):
    return {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}


def synth_forward_inputs(hp, seed, T1=9, T2=12):
    """B = 2 with ragged masks, item 1 shorter on both sides: (input_ids, input_mask, output_ids, output_mask), int64"""
    g = torch.Generator().manual_seed(seed)
    ii = torch.randint(0, hp["input_vocab_size"], (2, T1), generator=g)
    oi = torch.randint(0, hp["output_vocab_size"], (2, T2), generator=g)
    im, om = torch.ones(2, T1, dtype=torch.int64), torch.ones(2, T2, dtype=torch.int64)
    im[1, T1 - 3:] = 0
    om[1, T2 - 5:] = 0
    return ii, im, oi, om


def synth_generate_inputs(hp, seed, T1=9, T2=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, hp["input_vocab_size"], (1, T1), generator=g), torch.randint(0, hp["output_vocab_size"], (1, T2), generator=g)


# ---- the reference's padding (ar_model.py:174-235), integer torch ops ---------------------------------------------------------------------
def padding_for_input(hp, input_ids, input_mask):
    sp = special(hp)
    ids = (input_ids + hp["output_vocab_size"]) * input_mask
    ids = F.pad(ids, (0, 1), value=0) + sp["input_eos"] * F.pad(1 - input_mask, (0, 1), value=1)
    mask = F.pad(input_mask, (1, 0), value=1)
    ids = ids * mask + sp["pad"] * (1 - mask)
    ids = F.pad(ids, (1, 0), value=sp["input_bos"])
    mask = F.pad(mask, (1, 0), value=1)
    return ids.long(), mask.long(), (-100 * torch.ones_like(ids)).long()


def padding_for_output(hp, output_ids, output_mask):
    sp = special(hp)
    ids = output_ids * output_mask
    ids = F.pad(ids, (0, 1), value=0) + sp["output_eos"] * F.pad(1 - output_mask, (0, 1), value=1)
    mask = F.pad(output_mask, (1, 0), value=1)
    ids = ids * mask + sp["pad"] * (1 - mask)
    ids = F.pad(ids, (1, 0), value=sp["output_bos"])
    mask = F.pad(mask, (1, 0), value=1)
    return ids.long(), mask.long(), (ids * mask + -100 * (1 - mask)).long()


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def rms_norm(x, w):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS))


def causal_attention(q, k, v, key_mask=None, scale=None, offset=0):
    """q [B, H, Tq, dk] at positions offset .. offset + Tq - 1, k, v [B, H, L, dk], all already rotated; key j is visible to query i iff
    j <= offset + i and the key mask [B, L] admits it"""
    Tq, L = q.shape[2], k.shape[2]
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    s = torch.matmul(q, k.transpose(2, 3)) * scale
    hidden = torch.arange(L, device=q.device)[None, :] > (offset + torch.arange(Tq, device=q.device))[:, None]
    hidden = hidden[None, None]
    if key_mask is not None:
        hidden = hidden | (key_mask == 0)[:, None, None, :]
    return torch.matmul(torch.softmax(s.masked_fill(hidden, float("-inf")), dim=-1), v)


def causal_attention_cf(q, k, v, n_heads, cos, sin, key_mask=None):
    """the channel-first form of the kernel: un-rotated q, k, v [B, H*dk, T] -> [B, H*dk, T]"""
    B, C, T = q.shape
    sp = lambda t: t.reshape(B, n_heads, C // n_heads, T).transpose(2, 3)
    o = causal_attention(R.apply_rope(sp(q), cos, sin), R.apply_rope(sp(k), cos, sin), sp(v), key_mask)
    return o.transpose(2, 3).reshape(B, C, T)


def llama(sd, hp, ids, key_mask=None, cache=None, hidden_only=False):
    """ids [B, T] int64 -> logits [B, T, V].  ``cache``: a list (one dict per layer, or empty dicts) that holds rotated k and v of the
    positions before these and is extended by them; the ids then sit at positions L .. L + T - 1."""
    H, C = hp["num_attention_heads"], hp["hidden_size"]
    dk = C // H
    B, T = ids.shape
    dtype = sd["model.model.norm.weight"].dtype
    L0 = 0 if not cache or "k" not in cache[0] else cache[0]["k"].shape[2]
    cos, sin = R.rope_cos_sin(L0 + T, dk, device=ids.device)
    cos, sin = cos[L0:].to(dtype), sin[L0:].to(dtype)
    x = sd["model.model.embed_tokens.weight"][ids]
    for i in range(hp["num_hidden_layers"]):
        p = f"model.model.layers.{i}."
        h = rms_norm(x, sd[p + "input_layernorm.weight"])
        sp = lambda t: t.reshape(B, T, H, dk).transpose(1, 2)
        q = R.apply_rope(sp(F.linear(h, sd[p + "self_attn.q_proj.weight"])), cos, sin)
        k = R.apply_rope(sp(F.linear(h, sd[p + "self_attn.k_proj.weight"])), cos, sin)
        v = sp(F.linear(h, sd[p + "self_attn.v_proj.weight"]))
        if cache is not None:
            c = cache[i]
            if "k" in c:
                k, v = torch.cat((c["k"], k), 2), torch.cat((c["v"], v), 2)
            c["k"], c["v"] = k, v
        o = causal_attention(q, k, v, key_mask, offset=L0).transpose(1, 2).reshape(B, T, C)
        x = x + F.linear(o, sd[p + "self_attn.o_proj.weight"])
        x = x + R.swiglu_mlp(sd, p + "mlp.", rms_norm(x, sd[p + "post_attention_layernorm.weight"]))
    x = rms_norm(x, sd["model.model.norm.weight"])
    return x if hidden_only else F.linear(x, sd["model.lm_head.weight"])


def forward(sd, hp, input_ids, input_mask, output_ids, output_mask):
    """ar_model.py:81-172 without the global style encoder -> (logits [B, T1 + T2 + 4, V], loss): HF's shifted cross-entropy"""
    ii, im, il = padding_for_input(hp, input_ids, input_mask)
    oi, om, ol = padding_for_output(hp, output_ids, output_mask)
    ids, mask, labels = torch.cat((ii, oi), -1), torch.cat((im, om), -1), torch.cat((il, ol), -1)
    logits = llama(sd, hp, ids, mask)
    return logits, shifted_loss(logits, labels)


def shifted_loss(logits, labels):
    V = logits.shape[-1]
    return F.cross_entropy(logits[:, :-1].reshape(-1, V).float() if logits.dtype != torch.float64 else logits[:, :-1].reshape(-1, V),
                           labels[:, 1:].reshape(-1), ignore_index=-100)


# ---- HF's chain (transformers/generation/logits_process.py) on ONE row ----------------------------------------------------------------------
def process(logits, history, repetition_penalty=1.0, eos=None, suppress_eos=False, temperature=1.0, top_k=50, top_p=1.0, gaps=None):
    """logits [V], history: the ids so far [n] -> the filtered, temperature-scaled logits (-inf = removed).  ``gaps``: a dict that receives
    the distance of every discrete decision from its boundary, in the units of the logits at that point: ``sign`` (the penalised logits
    from 0), ``topk`` (the k-th largest from the next one below), ``topp`` (the cumulative probability nearest to 1 - top_p, halved: a
    logit error d moves a cumulative probability by at most 2 d)."""
    l = logits.clone()
    V = l.shape[0]
    if repetition_penalty != 1.0:
        idx = torch.unique(history)
        s = l[idx]
        if gaps is not None:
            gaps["sign"] = float(s.abs().min())
        l[idx] = torch.where(s < 0, s * repetition_penalty, s / repetition_penalty)
    if suppress_eos:
        l[eos] = float("-inf")
    l = l / temperature
    k = min(int(top_k), V)
    top = torch.topk(l, k)[0]
    if gaps is not None and k < V:
        below = l[l < top[-1]]
        if below.numel() and bool(torch.isfinite(below.max())):
            gaps["topk"] = float(top[-1] - below.max())
    l = l.masked_fill(l < top[-1], float("-inf"))
    if top_p < 1.0:
        sl, si = torch.sort(l, descending=False)
        cum = sl.softmax(-1).cumsum(-1)
        remove = cum <= (1 - top_p)
        remove[-1:] = False
        if gaps is not None:
            live = torch.isfinite(sl)
            live[-1] = False                              # the last one stays whatever its cumulative probability
            if bool(live.any()):
                gaps["topp"] = float((cum[live] - (1 - top_p)).abs().min()) / 2
        l = l.masked_fill(torch.zeros_like(remove).scatter(0, si, remove), float("-inf"))
    return l


def race(l, q, gaps=None):
    """the draw torch.multinomial makes, with its noise given: argmax softmax(l) / q, q ~ Exp(1).  ``gaps["race"]``: half the log-ratio of
    the winner to the runner-up (a logit error d moves log(p / q) by at most 2 d)."""
    r = torch.softmax(l, -1) / q.to(l.dtype)
    if gaps is not None:
        t = torch.topk(r, 2)[0]
        gaps["race"] = float("inf") if float(t[1]) == 0.0 else float(torch.log(t[0] / t[1])) / 2
    return int(torch.argmax(r))


def generate(sd, hp, input_ids, prompt_output_ids, draws, max_length=2000, temperature=0.8, top_k=50, top_p=0.9, repeat_penalty=1.0,
             min_new_tokens=50, teacher=None, record=None):
    """ar_model.py:237-344 around HF's sampling loop, one sample, with a KV cache.  ``draws(step, V)`` -> the step's Exp(1) row.  ``teacher``:
    the tokens to force (every step's logits stay comparable with the run that produced them).  ``record``: a list that receives per step
    {"logits", "gaps", "token"}.  -> the new tokens [1, n] after the reference's BOS / EOS stripping."""
    sp = special(hp)
    ii, _, _ = padding_for_input(hp, input_ids, torch.ones_like(input_ids))
    po, _, _ = padding_for_output(hp, prompt_output_ids, torch.ones_like(prompt_output_ids))
    ids = torch.cat((ii, po[:, :-1]), -1)
    n0 = ids.shape[1]
    cache = [dict() for _ in range(hp["num_hidden_layers"])]
    logits = llama(sd, hp, ids, cache=cache)[0, -1]
    step = 0
    while True:
        gaps = {}
        n_new = ids.shape[1] - n0
        l = process(logits, ids[0], repeat_penalty, sp["output_eos"], n_new < min_new_tokens, temperature, top_k, top_p, gaps)
        tok = race(l, draws(step, l.shape[0]), gaps)
        if teacher is not None:
            tok = int(teacher[step])
        if record is not None:
            record.append({"logits": logits, "gaps": gaps, "token": tok})
        ids = torch.cat((ids, torch.tensor([[tok]], dtype=ids.dtype, device=ids.device)), -1)
        step += 1
        if tok == sp["output_eos"] or ids.shape[1] >= max_length:
            break
        logits = llama(sd, hp, ids[:, -1:], cache=cache)[0, -1]
    gen = ids[:, n0:]
    if gen[0, 0] == sp["output_bos"]:
        gen = gen[:, 1:]
    if gen[0, -1] == sp["output_eos"]:
        gen = gen[:, :-1]
    return gen, ids[0, n0:]


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


def decidedness(sd32, sd64, hp, input_ids, prompt_output_ids, draws, teacher=None, **kw):
    """Runs ``generate`` in fp32 and (teacher-forced on the fp32 tokens, or on ``teacher``) in fp64 and returns (tokens32, tau, gap): tau =
    the largest distance of an fp32 logit from its fp64 value over the run, gap = the smallest distance of any discrete decision of the
    fp64 run -- the penalty's sign test, the top-k boundary, the top-p cut, the race -- from its boundary, in the logits' units at that
    point (``process`` / ``race``).  A run is DECIDED when gap >= 4 tau: no evaluation within tau of fp64 takes another branch."""
    r32, r64 = [], []
    _, raw32 = generate(sd32, hp, input_ids, prompt_output_ids, draws, teacher=teacher, record=r32, **kw)
    generate(sd64, hp, input_ids, prompt_output_ids, draws, teacher=raw32.tolist() if teacher is None else teacher, record=r64, **kw)
    n = min(len(r32), len(r64))
    tau = max(float((a["logits"].double() - b["logits"]).abs().max()) for a, b in zip(r32[:n], r64[:n]))
    pen = kw.get("repeat_penalty", 1.0)
    tau *= max(1.0, 1.0 / kw.get("temperature", 0.8)) * max(pen, 1.0 / pen)      # in the units of the processed logits
    gap = min(min(b["gaps"].values()) for b in r64[:n])
    return raw32, tau, gap
