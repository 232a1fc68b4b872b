"""Torch restatement of Vevo's flow-matching transformer (models/vc/flow_matching_transformer/{llama_nar,fmt_model}.py), runnable in fp32 and
fp64 on the CPU (or on a device): the reference of the GPU tests and, in fp32 on the device, the torch-ops baseline of tools/bench_fmt.py.

    rope_attention       LlamaAttention as DiffLlama calls it: q / k rotated by HF's rotate-half RoPE (modeling_llama.py: rotate_half,
                         apply_rotary_pos_emb), the non-causal additive KEY mask of llama_nar.py:197-234 (finfo.min on padded keys, every query
                         row computed), softmax, @ v
    adaptive_rms_norm    LlamaAdaptiveRMSNorm.forward, llama_nar.py:41-50
    swiglu_mlp           LlamaMLP: down(silu(gate(x)) * up(x))
    diffllama_forward    DiffLlama.forward, llama_nar.py:236-397
    reverse_diffusion    FlowMatchingTransformer.reverse_diffusion, fmt_model.py:228-283, with the noise given

Everything is functional over a ``state_dict`` under the reference's keys.  The ``rope`` / ``mask_on`` / ``unbiased`` arguments select DELIBERATELY
WRONG variants (interleaved-pair RoPE, the mask on queries, another std): tests/test_oracle_fmt.py shows that each misses the golden outputs, i.e.
that the goldens can tell them apart."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-6        # LlamaAdaptiveRMSNorm's default, which DiffLlama never overrides (llama_nar.py:33,156,184-189)
THETA = 10000.0   # LlamaConfig.rope_theta's default


def small_hp():
    """the configuration of the goldens and the GPU model tests: two heads of 64"""
    return dict(mel_dim=20, hidden_size=128, num_layers=2, num_heads=2, cond_codebook_size=32)


def state_dict_keys(hp, use_cond_code=True):
    """the keys of FlowMatchingTransformer.state_dict() in the reference's order (tests/golden/keys_fmt.json pins them to the real class)"""
    keys = ["cond_emb.weight"] + ([] if use_cond_code else ["cond_emb.bias"])
    p = "diff_estimator."
    for i in range(hp["num_layers"]):
        q = f"{p}layers.{i}."
        keys += [q + f"self_attn.{n}_proj.weight" for n in "qkvo"]
        keys += [q + f"mlp.{n}_proj.weight" for n in ("gate", "up", "down")]
        keys += [q + f"{n}.to_weight.{w}" for n in ("input_layernorm", "post_attention_layernorm") for w in ("weight", "bias")]
    keys += [p + "norm.to_weight.weight", p + "norm.to_weight.bias"]
    for m in ("diff_step_mlp", "cond_mlp", "mel_mlp", "mel_out_mlp"):
        keys += [f"{p}{m}.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")]
    return keys


def _shape(hp, key):
    C, M = hp["hidden_size"], hp["mel_dim"]
    if key == "cond_emb.weight":
        return (hp["cond_codebook_size"], C)
    k = key.split(".", 1)[1]
    if "to_weight" in k or "self_attn" in k:
        return (C, C) if k.endswith("weight") else (C,)
    if "mlp.gate" in k or "mlp.up" in k:
        return (4 * C, C)
    if "mlp.down" in k:
        return (C, 4 * C)
    name, idx, w = k.split(".")
    cin = M if name == "mel_mlp" else C
    cout = M if name == "mel_out_mlp" else C
    shape = (4 * C, cin) if idx == "0" else (cout, 4 * C)
    return shape if w == "weight" else shape[:1]


def synth_state_dict(hp, seed):
    """Weights for the tests, in the keys' sorted order from one generator: Linear weights at std 0.05 (the initialisation's 0.02 leaves the
    residual stream near the embedding), their biases at 0.02, and ``to_weight`` redrawn (weight std 0.05, bias 1 + 0.1 randn) so that the
    adaptive norms are not the identity their zero initialisation makes them."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key in sorted(state_dict_keys(hp)):
        shape = _shape(hp, key)
        r = torch.randn(shape, generator=g)
        if key == "cond_emb.weight":
            sd[key] = 0.5 * r
        elif "to_weight.bias" in key:
            sd[key] = 1.0 + 0.1 * r
        elif key.endswith("bias"):
            sd[key] = 0.02 * r
        else:
            sd[key] = 0.05 * r
    return {k: sd[k] for k in state_dict_keys(hp)}


def synth_inputs(hp, B, T, seed):
    """(x [B, T, mel], t [B], codes [B, T] int64) for a forward"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, hp["mel_dim"], generator=g)
    t = torch.rand(B, generator=g)
    codes = torch.randint(0, hp["cond_codebook_size"], (B, T), generator=g)
    return x, t, codes


# ---- the pieces ---------------------------------------------------------------------------------------------------------------------------
def rope_cos_sin(T, dk, device="cpu", dtype=torch.float32):
    """[T, dk/2] each, computed in fp32 as LlamaRotaryEmbedding does (inv_freq = theta^(-2i/dk), positions 0 .. T-1) and then cast: the
    tables are an INPUT of the attention, in fp64 too"""
    inv_freq = 1.0 / (THETA ** (torch.arange(0, dk, 2, dtype=torch.int64).to(device=device, dtype=torch.float32) / dk))
    freqs = torch.arange(T, device=device, dtype=torch.float32)[:, None] * inv_freq[None, :]
    return freqs.cos().to(dtype), freqs.sin().to(dtype)


def apply_rope(x, cos, sin, rope="half"):
    """x [B, H, T, dk]; cos, sin [T, dk/2]"""
    half = x.shape[-1] // 2
    if rope == "half":                                   # HF: x * cat(cos, cos) + rotate_half(x) * cat(sin, sin)
        c, s = torch.cat((cos, cos), -1), torch.cat((sin, sin), -1)
        return x * c + torch.cat((-x[..., half:], x[..., :half]), -1) * s
    assert rope == "interleaved"                         # the WRONG variant: pairs (2i, 2i + 1)
    x1, x2 = x[..., 0::2], x[..., 1::2]
    return torch.stack((x1 * cos - x2 * sin, x2 * cos + x1 * sin), -1).flatten(-2)


def rope_attention(q, k, v, cos, sin, key_mask=None, scale=None, rope="half", mask_on="keys"):
    """q, k, v [B, H, T, dk]; key_mask [B, T] (nonzero = valid) or None -> [B, H, T, dk]"""
    dk = q.shape[-1]
    scale = 1.0 / math.sqrt(dk) if scale is None else scale
    s = torch.matmul(apply_rope(q, cos, sin, rope), apply_rope(k, cos, sin, rope).transpose(2, 3)) * scale
    if key_mask is not None:
        bad = key_mask == 0
        bad = bad[:, None, None, :] if mask_on == "keys" else bad[:, None, :, None]
        s = s + torch.zeros_like(s).masked_fill(bad, torch.finfo(s.dtype).min)
    return torch.matmul(torch.softmax(s, dim=-1), v)


def rope_attention_cf(q, k, v, n_heads, cos, sin, key_mask=None, scale=None):
    """the channel-first form of the kernel: q, k, v [B, H*dk, T] -> [B, H*dk, T]"""
    B, C, T = q.shape
    sp = lambda t: t.reshape(B, n_heads, C // n_heads, T).transpose(2, 3)
    return rope_attention(sp(q), sp(k), sp(v), cos, sin, key_mask, scale).transpose(2, 3).reshape(B, C, T)


def adaptive_rms_norm(x, w, eps=EPS):
    """x [B, T, C], w [B, C] -> w * x * rsqrt(mean(x^2) + eps)"""
    return w[:, None, :] * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def mlp2(sd, p, x):
    """nn.Sequential(Linear, SiLU, Linear)"""
    return F.linear(F.silu(F.linear(x, sd[p + ".0.weight"], sd[p + ".0.bias"])), sd[p + ".2.weight"], sd[p + ".2.bias"])


def swiglu_mlp(sd, p, x):
    return F.linear(F.silu(F.linear(x, sd[p + "gate_proj.weight"])) * F.linear(x, sd[p + "up_proj.weight"]), sd[p + "down_proj.weight"])


def sinusoidal_pos_emb(t, dim):
    """SinusoidalPosEmb, llama_nar.py:17-29"""
    half = dim // 2
    e = torch.exp(torch.arange(half, device=t.device) * -(math.log(10000) / (half - 1)))
    e = t[:, None] * e[None, :] * 1.0
    return torch.cat((e.sin(), e.cos()), dim=-1)


def cast(sd, dtype, device=None):
    return {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}


def diffllama_forward(sd, hp, x, t, cond, x_mask=None, prefix="diff_estimator.", rope="half", mask_on="keys", hidden=None):
    """sd already in the working dtype; x [B, T, mel], t [B], cond [B, T, hidden], x_mask [B, T] or None -> [B, T, mel]; ``hidden``: a list
    that receives every layer's output"""
    H = hp["num_heads"]
    B, T, _ = x.shape
    p = prefix
    h = mlp2(sd, p + "mel_mlp", x) + mlp2(sd, p + "cond_mlp", cond)
    step = mlp2(sd, p + "diff_step_mlp", sinusoidal_pos_emb(t, hp["hidden_size"]).to(x.dtype))
    C = h.shape[-1]
    cos, sin = rope_cos_sin(T, C // H, x.device, x.dtype)
    nw = lambda q: F.linear(step, sd[q + ".to_weight.weight"], sd[q + ".to_weight.bias"])
    heads = lambda y: y.reshape(B, T, H, C // H).transpose(1, 2)
    for i in range(hp["num_layers"]):
        q = f"{p}layers.{i}."
        y = adaptive_rms_norm(h, nw(q + "input_layernorm"))
        a = rope_attention(heads(F.linear(y, sd[q + "self_attn.q_proj.weight"])), heads(F.linear(y, sd[q + "self_attn.k_proj.weight"])),
                           heads(F.linear(y, sd[q + "self_attn.v_proj.weight"])), cos, sin, x_mask, rope=rope, mask_on=mask_on)
        h = h + F.linear(a.transpose(1, 2).reshape(B, T, C), sd[q + "self_attn.o_proj.weight"])
        h = h + swiglu_mlp(sd, q + "mlp.", adaptive_rms_norm(h, nw(q + "post_attention_layernorm")))
        if hidden is not None:
            hidden.append(h.clone())
    return mlp2(sd, p + "mel_out_mlp", adaptive_rms_norm(h, nw(p + "norm")))


def reverse_diffusion(sd, hp, cond, prompt, noise, x_mask=None, prompt_mask=None, n_timesteps=10, cfg=1.0, rescale_cfg=0.75, unbiased=True, std=None,
                      **kw):
    """cond [B, Tp + Tt, hidden], prompt [B, Tp, mel], noise [B, Tt, mel] -> [B, Tt, mel].  The std of the classifier-free rescale is
    ``Tensor.std()``: over the whole tensor, batch included, unbiased; ``unbiased=False`` / ``std=<function>`` swap it for a variant."""
    h = 1.0 / n_timesteps
    Tp = prompt.shape[1]
    Tt = cond.shape[1] - Tp
    one = lambda n: torch.ones(cond.shape[0], n, dtype=cond.dtype, device=cond.device)
    x_mask = one(Tt) if x_mask is None else x_mask
    prompt_mask = one(Tp) if prompt_mask is None else prompt_mask
    xt_mask = torch.cat([prompt_mask, x_mask], dim=1)
    xt = noise
    if std is None:
        std = lambda v: v.std() if unbiased else v.std(unbiased=False)
    for i in range(n_timesteps):
        t = (0 + (i + 0.5) * h) * torch.ones(noise.shape[0], dtype=noise.dtype, device=noise.device)
        flow = diffllama_forward(sd, hp, torch.cat([prompt, xt], dim=1), t, cond, xt_mask, **kw)[:, Tp:, :]
        if cfg > 0:
            uncond = diffllama_forward(sd, hp, xt, t, torch.zeros_like(cond)[:, :Tt, :], x_mask, **kw)
            pos_std = std(flow)
            flow_cfg = flow + cfg * (flow - uncond)
            flow = rescale_cfg * (flow_cfg * pos_std / std(flow_cfg)) + (1 - rescale_cfg) * flow_cfg
        xt = xt + flow * h
    return xt
