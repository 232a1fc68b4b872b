"""Plain torch statements of the VITS element-wise / frame-rate ops, one per exported entry point (include/amphion_hip.h), written
from the reference's formulas.  Every function computes in the dtype of its floating inputs: called on ``.double()`` tensors it is
the fp64 reference of tests/test_gpu_vits_ops.py, called on the fp32 tensors themselves it is "the same formula in fp32 on the
CPU" that sizes the bound of the transcendental ops and the exact counterpart of the ops that only move data or do one fp32
operation.  What oracle/ already states (LayerNorm over channels, the relative attention, the spline, generate_path) is reused,
not restated; tests/test_vits_ops_ref.py ties the WN / posterior / coupling pieces to the oracle's golden-pinned modules."""
import math

import torch
import torch.nn.functional as F

from oracle import vits_infer_oracle as vio


def seq_mask(lens, B, T, dtype=torch.bool):
    """sequence_mask(lens) utils/util.py:618-622 as [B, 1, T]; ``lens`` None = every column valid"""
    if lens is None:
        return torch.ones(B, 1, T, dtype=dtype)
    return (torch.arange(T).view(1, 1, T) < torch.as_tensor(lens).view(B, 1, 1)).to(dtype)


def wn_gate(a, cond=None):
    """fused_add_tanh_sigmoid_multiply utils/util.py:602-609 with a time-constant condition: a [B, 2H, T], cond [B, 2H] -> [B, H, T]"""
    H = a.shape[1] // 2
    in_act = a if cond is None else a + cond.unsqueeze(-1)
    return torch.tanh(in_act[:, :H]) * torch.sigmoid(in_act[:, H:])


def wn_accumulate(x, out, rs, lens, first, last):
    """modules/flow/modules.py:144-151 -> (x, out); ``first`` starts out from zero (:127), whatever it held"""
    B, H, T = x.shape
    if first:
        out = torch.zeros_like(x)
    if last:
        return x, out + rs
    return (x + rs[:, :H]) * seq_mask(lens, B, T, x.dtype), out + rs[:, H:]


def sequence_mask(x, lens):
    """x * x_mask, as an assignment of zero (NaN beyond the length does not survive)"""
    return torch.where(seq_mask(lens, x.shape[0], x.shape[2]), x, torch.zeros_like(x))


def coupling_apply(x, m, lens, reverse):
    """mean-only ResidualCouplingLayer modules/flow/modules.py:390-397 on x [B, 2h, T], m [B, h, T] (m unspecified beyond the length)"""
    B, C, T = x.shape
    h = C // 2
    x0, x1 = x[:, :h], x[:, h:]
    v = x1 - m if reverse else m + x1
    valid = seq_mask(lens, B, T)
    return torch.cat([x0, torch.where(valid, v, torch.zeros_like(v))], 1)


def flip_channels(x):
    """Flip.forward modules/flow/modules.py:314-321"""
    return torch.flip(x, [1])


def posterior_sample(stats, eps, lens):
    """vits.py:150-151: stats = [m ; logs] [B, 2C, T] -> z = (m + eps * exp(logs)) * mask"""
    B, C2, T = stats.shape
    m, logs = stats[:, :C2 // 2], stats[:, C2 // 2:]
    return (m + eps * torch.exp(logs)) * seq_mask(lens, B, T, stats.dtype)


def affine_reverse(x, m, logs, lens):
    """ElementwiseAffine reverse modules/flow/modules.py:338-340; m, logs [C]"""
    B, C, T = x.shape
    return (x - m.view(1, C, 1)) * torch.exp(-logs.view(1, C, 1)) * seq_mask(lens, B, T, x.dtype)


def embed_tokens(tokens, weight, lens, scale):
    """TextEncoder.forward vits.py:58-62: emb(tokens) * sqrt(hidden), [B, hidden, T], masked"""
    B, T = tokens.shape
    return (weight[tokens] * scale).transpose(1, 2) * seq_mask(lens, B, T, weight.dtype)


def gauss_sample(m, logs, noise, noise_scale):
    """vits.py:355 (not masked there)"""
    return m + noise * torch.exp(logs) * noise_scale


def add_channel_bias(x, cb):
    """x + cond(g) for a length-1 condition: cb [B, C] or [B, C, 1]"""
    return x + cb.reshape(x.shape[0], x.shape[1], 1)


def layer_norm_c_ragged(x, res, gamma, beta, post, lens, eps=1e-5, gelu=False):
    """post + act(LN(x + res)) over channels (base_module.py:20-23, modules/flow/modules.py:64-70), zero beyond the lengths whatever
    the inputs hold there"""
    B, C, T = x.shape
    valid = seq_mask(lens, B, T).expand(B, C, T)
    clean = lambda t: None if t is None else torch.where(valid, t, torch.zeros_like(t))  # noqa: E731
    x, res, post = clean(x), clean(res), clean(post)
    y = vio.layer_norm_channels(x if res is None else x + res, gamma, beta, eps)
    if gelu:
        y = F.gelu(y)
    if post is not None:
        y = post + y
    return torch.where(valid, y, torch.zeros_like(y))


def attention_operands(x):
    """q, k, v for the attention tests as three EXACT channel maps of one tensor, so that the oracle's attention (which projects a
    single x through conv_q / conv_k / conv_v) sees the very numbers the kernel is given: q = x, k = 0.5 * flip(x), v = -2 * roll(x).
    -> (q, k, v, {conv weights for vio.relative_self_attention under prefix "a"})"""
    C = x.shape[1]
    eye = torch.eye(C, dtype=x.dtype)
    wk, wv = 0.5 * torch.flip(eye, [0]), -2.0 * torch.roll(eye, 1, 0)
    sd = {"a.conv_q.weight": eye.unsqueeze(-1), "a.conv_k.weight": wk.unsqueeze(-1), "a.conv_v.weight": wv.unsqueeze(-1),
          "a.conv_o.weight": eye.unsqueeze(-1)}
    for n in "qkvo":
        sd[f"a.conv_{n}.bias"] = torch.zeros(C, dtype=x.dtype)
    return x, 0.5 * torch.flip(x, [1]), -2.0 * torch.roll(x, 1, 1), sd


def rel_attention(x, emb_k, emb_v, lens, n_heads, window):
    """amp_rel_attention on attention_operands(x): attentions.py:232-272 through the oracle; only queries below the length are specified"""
    B, C, T = x.shape
    _, _, _, sd = attention_operands(x)
    sd["a.emb_rel_k"], sd["a.emb_rel_v"] = emb_k.unsqueeze(0).to(x.dtype), emb_v.unsqueeze(0).to(x.dtype)
    return vio.relative_self_attention(sd, "a", x, seq_mask(lens, B, T, x.dtype), n_heads, window)


def expand_path(src, w_ceil, xlens, ylens, t_y):
    """attn = generate_path(w_ceil, x_mask (x) y_mask) and attn @ src (utils/util.py:625-640, vits.py:345-353): src [B, D, Tx],
    w_ceil [B, 1, Tx] -> (out [B, D, t_y], attn [B, 1, t_y, Tx])"""
    B, D, Tx = src.shape
    xm = seq_mask(xlens, B, Tx, src.dtype)
    ym = seq_mask(ylens, B, t_y, src.dtype)
    attn = vio.generate_path(w_ceil.to(src.dtype), xm.unsqueeze(2) * ym.unsqueeze(-1))
    return torch.matmul(attn.squeeze(1), src.transpose(1, 2)).transpose(1, 2), attn


def dwconv(x, weight, bias, lens, dilation):
    """DDSConv.convs_sep modules/flow/modules.py:46-56,63 on x * mask"""
    B, C, T = x.shape
    K = weight.shape[-1]
    xm = torch.where(seq_mask(lens, B, T).expand(B, C, T), x, torch.zeros_like(x))
    return F.conv1d(xm, weight, bias, padding=(K * dilation - dilation) // 2, dilation=dilation, groups=C)


def spline_flow(z, h, lens, num_bins, filter_channels, tail_bound, inverse, flip_in=False, flip_out=False):
    """ConvFlow's spline step modules/flow/modules.py:435-458 through the oracle's rq_spline, the neighbouring Flips folded in"""
    B, _, T = z.shape
    K = num_bins
    mask = seq_mask(lens, B, T, z.dtype)
    if flip_in:
        z = torch.flip(z, [1])
    hm = (h * mask).reshape(B, 1, 3 * K - 1, T).permute(0, 1, 3, 2)
    s = 1.0 / math.sqrt(filter_channels)
    y1 = vio.rq_spline(z[:, 1:], hm[..., :K] * s, hm[..., K:2 * K] * s, hm[..., 2 * K:], inverse, tail_bound)
    out = torch.cat([z[:, :1], y1], 1) * mask
    return torch.flip(out, [1]) if flip_out else out


def durations(logw, lens, length_scale):
    """vits.py:341-343 + the cumsum of generate_path -> (w_ceil [B, 1, T], cum [B, T] int64, y_len [B] int64)"""
    B, _, T = logw.shape
    w_ceil = torch.ceil(torch.exp(logw) * seq_mask(lens, B, T, logw.dtype) * length_scale)
    cum = torch.cumsum(w_ceil[:, 0].to(torch.int64), -1)
    return w_ceil, cum, torch.clamp_min(cum[:, -1], 1)
