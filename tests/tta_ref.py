"""AudioLDM text-to-audio restated in plain torch ops on the CPU (models/tta of the reference): the 3 x 3 conv with its run-time options, GroupNorm,
GEGLU, attention, the UNet, the AutoencoderKL decoder and the sampling loop, as functions of a state_dict.  Every function computes in the
dtype of its inputs, so the same text gives the fp64 reference and the fp32 CPU evaluation whose distance from it sets the GPU tests' bound.
No GPU import; tests/test_oracle_tta.py checks this file against goldens written from the real classes (tests/golden/make_golden_tta.py)."""
from __future__ import annotations

import math
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F


def small_hp():
    """the small UNet of the goldens: head dimensions 32 / 64 / 128 at the three levels, like the recipe's"""
    return dict(image_size=32, in_channels=4, out_channels=4, model_channels=64, attention_resolutions=[4, 2, 1], num_res_blocks=2,
                channel_mult=[1, 2, 4], num_heads=2, use_spatial_transformer=True, transformer_depth=1, context_dim=48, use_checkpoint=True,
                legacy=False)


def small_vae_hp():
    return dict(ch=32, ch_mult=[1, 1, 2, 2, 4], num_res_blocks=2, in_channels=1, z_channels=4, out_ch=1, double_z=True)


class Cfg(dict):
    """a dict read by attribute, as the reference reads its configuration"""
    __getattr__ = dict.__getitem__


def synth_state_dict(shapes, seed):
    """name -> fp32 tensor for ``shapes`` (name -> shape), each drawn from a generator of its own seeded by (seed, name): norm weights around 1,
    other vectors small, matrices and conv weights at 1 / sqrt(fan_in).  Every weight is drawn -- the ``zero_module`` layers of the reference
    (each ResBlock's last conv, ``proj_out``, ``out.2``) too, which leave ``__init__`` at zero and would hide everything before them."""
    sd = {}
    for name, shape in shapes.items():
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
        shape = tuple(shape)
        if len(shape) == 1:
            is_norm_w = name.endswith("weight")
            sd[name] = (1.0 + 0.1 * torch.randn(shape, generator=g)) if is_norm_w else 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            sd[name] = torch.randn(shape, generator=g) / math.sqrt(fan_in)
    return sd


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


# ---- ops ------------------------------------------------------------------------------------------------------------------------------------
def group_norm_stats_ref(x, eps):
    """x [B, C, ...] -> mean | rstd [B, 32, 2], biased variance"""
    B = x.shape[0]
    g = x.reshape(B, 32, -1)
    mean = g.mean(dim=2)
    var = ((g - mean[:, :, None]) ** 2).mean(dim=2)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], dim=2)


def group_norm_ref(x, gamma, beta, eps, silu=False):
    """GroupNorm(32) written out (F.group_norm refuses a group of one value, which the 1 x 1 feature map of 32 channels is)"""
    B, C = x.shape[:2]
    mr = group_norm_stats_ref(x, eps)
    shape = (B, 32, 1) + (1,) * (x.dim() - 2)
    y = ((x.reshape((B, 32, C // 32) + tuple(x.shape[2:])) - mr[:, :, 0].reshape(shape)) * mr[:, :, 1].reshape(shape)).reshape(x.shape)
    cshape = (1, C) + (1,) * (x.dim() - 2)
    y = y * gamma.reshape(cshape) + beta.reshape(cshape)
    return F.silu(y) if silu else y


def conv2d_ref(x, w, b, stride=1, up2=False, norm=None, row_add=None, residual=None, wrong_padding=False):
    """the conv of amp_conv2d_forward.  norm = (gamma, beta, eps): GroupNorm(32) + SiLU first.  wrong_padding: the mistake the bound must tell
    apart -- the padding taken from the UN-activated x (zero there, so the border taps see silu(beta-ish) instead of 0)"""
    a = x
    if norm is not None:
        gamma, beta, eps = norm
        if wrong_padding:
            # pad x with zeros FIRST and normalise the padded tensor with the statistics of the unpadded one
            mr = group_norm_stats_ref(x, eps)
            B, C = x.shape[:2]
            xp = F.pad(x, (1, 1, 1, 1))
            gsz = C // 32
            mean = mr[:, :, 0].repeat_interleave(gsz, dim=1)[:, :, None, None]
            rstd = mr[:, :, 1].repeat_interleave(gsz, dim=1)[:, :, None, None]
            ap = F.silu((xp - mean) * rstd * gamma[None, :, None, None] + beta[None, :, None, None])
            if up2:
                raise ValueError("wrong_padding with up2 is not stated")
            y = F.conv2d(ap, w, b, stride=stride, padding=0)
            if row_add is not None:
                y = y + row_add[:, :, None, None]
            return y if residual is None else y + residual
        a = group_norm_ref(x, gamma, beta, eps, silu=True)
    if up2:
        a = a.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    y = F.conv2d(a, w, b, stride=stride, padding=1)
    if row_add is not None:
        y = y + row_add[:, :, None, None]
    if residual is not None:
        y = y + residual
    return y


def geglu_ref(u):
    """u [B, 2F, T] -> value * gelu(gate), the first half the value"""
    Fh = u.shape[1] // 2
    return u[:, :Fh] * F.gelu(u[:, Fh:])


def attention_cf(q, k, v, H, scale=None):
    """q [B, H*dk, Tq], k, v [B, H*dk, Tk] channel-first, heads as row blocks -> [B, H*dk, Tq]"""
    B, C, Tq = q.shape
    dk = C // H
    scale = dk ** -0.5 if scale is None else scale
    qq = q.reshape(B, H, dk, Tq).transpose(2, 3)
    kk = k.reshape(B, H, dk, -1)
    vv = v.reshape(B, H, dk, -1).transpose(2, 3)
    p = torch.softmax((qq @ kk) * scale, dim=-1)
    return (p @ vv).transpose(2, 3).reshape(B, C, Tq)


# ---- the UNet -------------------------------------------------------------------------------------------------------------------------------
def timestep_embedding(t, dim, dtype):
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half).to(t.device)      # the reference forms the table in fp32
    args = t[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1).to(dtype)


def unet_layout(hp):
    """(input blocks, middle block, output blocks), each block a list of ("conv",) | ("res", cin, cout) | ("attn", ch) | ("down", ch) | ("up", ch)"""
    mc, cm, nrb, ar = hp["model_channels"], hp["channel_mult"], hp["num_res_blocks"], hp["attention_resolutions"]
    inp, chans, ch, ds = [[("conv",)]], [mc], mc, 1
    for level, mult in enumerate(cm):
        for _ in range(nrb):
            blk = [("res", ch, mult * mc)]
            ch = mult * mc
            if ds in ar:
                blk.append(("attn", ch))
            inp.append(blk)
            chans.append(ch)
        if level != len(cm) - 1:
            inp.append([("down", ch)])
            chans.append(ch)
            ds *= 2
    mid = [("res", ch, ch), ("attn", ch), ("res", ch, ch)]
    out = []
    for level, mult in list(enumerate(cm))[::-1]:
        for i in range(nrb + 1):
            ich = chans.pop()
            blk = [("res", ch + ich, mc * mult)]
            ch = mc * mult
            if ds in ar:
                blk.append(("attn", ch))
            if level and i == nrb:
                blk.append(("up", ch))
                ds //= 2
            out.append(blk)
    return inp, mid, out


def resblock_ref(sd, p, x, emb):
    """x [B, C, H, W], emb [B, 4 * model_channels] (time_embed's output).  The embedding is added BEFORE the second norm."""
    h = conv2d_ref(x, sd[p + "in_layers.2.weight"], sd[p + "in_layers.2.bias"], norm=(sd[p + "in_layers.0.weight"], sd[p + "in_layers.0.bias"], 1e-5))
    e = F.linear(F.silu(emb), sd[p + "emb_layers.1.weight"], sd[p + "emb_layers.1.bias"])
    h = h + e[:, :, None, None]
    h = conv2d_ref(h, sd[p + "out_layers.3.weight"], sd[p + "out_layers.3.bias"], norm=(sd[p + "out_layers.0.weight"], sd[p + "out_layers.0.bias"], 1e-5))
    if p + "skip_connection.weight" in sd:
        x = F.conv2d(x, sd[p + "skip_connection.weight"], sd[p + "skip_connection.bias"])
    return x + h


def _cross_attn(sd, p, x, ctx, heads):
    """x [B, N, C], ctx [B, M, Cc]"""
    q, k, v = x @ sd[p + "to_q.weight"].T, ctx @ sd[p + "to_k.weight"].T, ctx @ sd[p + "to_v.weight"].T
    o = attention_cf(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), heads).transpose(1, 2)
    return o @ sd[p + "to_out.0.weight"].T + sd[p + "to_out.0.bias"]


def transformer_block_ref(sd, p, x, ctx, heads):
    C = x.shape[-1]
    ln = lambda n, t: F.layer_norm(t, (C,), sd[p + n + ".weight"], sd[p + n + ".bias"], 1e-5)
    n1 = ln("norm1", x)
    x = _cross_attn(sd, p + "attn1.", n1, n1, heads) + x
    x = _cross_attn(sd, p + "attn2.", ln("norm2", x), ctx, heads) + x
    u = ln("norm3", x) @ sd[p + "ff.net.0.proj.weight"].T + sd[p + "ff.net.0.proj.bias"]
    val, gate = u.chunk(2, dim=-1)
    return (val * F.gelu(gate)) @ sd[p + "ff.net.2.weight"].T + sd[p + "ff.net.2.bias"] + x


def spatial_transformer_ref(sd, p, x, ctx, heads, depth=1):
    B, C, H, W = x.shape
    t = group_norm_ref(x, sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-6)
    t = F.conv2d(t, sd[p + "proj_in.weight"], sd[p + "proj_in.bias"]).reshape(B, -1, H * W).transpose(1, 2)
    for d in range(depth):
        t = transformer_block_ref(sd, f"{p}transformer_blocks.{d}.", t, ctx, heads)
    t = t.transpose(1, 2).reshape(B, -1, H, W)
    return F.conv2d(t, sd[p + "proj_out.weight"], sd[p + "proj_out.bias"]) + x


def _run_block(sd, p, layers, h, emb, ctx, hp):
    for j, layer in enumerate(layers):
        q = f"{p}{j}."
        if layer[0] == "conv":
            h = F.conv2d(h, sd[q + "weight"], sd[q + "bias"], padding=1)
        elif layer[0] == "res":
            h = resblock_ref(sd, q, h, emb)
        elif layer[0] == "attn":
            h = spatial_transformer_ref(sd, q, h, ctx, hp["num_heads"], hp["transformer_depth"])
        elif layer[0] == "down":
            h = F.conv2d(h, sd[q + "op.weight"], sd[q + "op.bias"], stride=2, padding=1)
        else:
            h = conv2d_ref(h, sd[q + "conv.weight"], sd[q + "conv.bias"], up2=True)
    return h


def unet_forward(sd, hp, x, timesteps, context, prefix="unet."):
    """AudioLDM.forward(x, timesteps, context) in the dtype of ``sd`` / ``x``"""
    inp, mid, out = unet_layout(hp)
    dt = x.dtype
    te = timestep_embedding(timesteps, hp["model_channels"], dt)
    emb = F.linear(F.silu(F.linear(te, sd[prefix + "time_embed.0.weight"], sd[prefix + "time_embed.0.bias"])), sd[prefix + "time_embed.2.weight"],
                   sd[prefix + "time_embed.2.bias"])
    hs, h = [], x
    for i, layers in enumerate(inp):
        h = _run_block(sd, f"{prefix}input_blocks.{i}.", layers, h, emb, context, hp)
        hs.append(h)
    h = _run_block(sd, f"{prefix}middle_block.", mid, h, emb, context, hp)
    for i, layers in enumerate(out):
        skip = hs.pop()
        h = h[:, :, : skip.shape[2], : skip.shape[3]]
        h = _run_block(sd, f"{prefix}output_blocks.{i}.", layers, torch.cat([h, skip], dim=1), emb, context, hp)
    return conv2d_ref(h, sd[prefix + "out.2.weight"], sd[prefix + "out.2.bias"], norm=(sd[prefix + "out.0.weight"], sd[prefix + "out.0.bias"], 1e-5))


# ---- the AutoencoderKL decoder ------------------------------------------------------------------------------------------------------------------
def resnet_block_ref(sd, p, x):
    h = conv2d_ref(x, sd[p + "conv1.weight"], sd[p + "conv1.bias"], norm=(sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6))
    h = conv2d_ref(h, sd[p + "conv2.weight"], sd[p + "conv2.bias"], norm=(sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6))
    if p + "nin_shortcut.weight" in sd:
        x = F.conv2d(x, sd[p + "nin_shortcut.weight"], sd[p + "nin_shortcut.bias"])
    return x + h


def decode_ref(sd, hp, z):
    """AutoencoderKL.decode(z)"""
    h = F.conv2d(z, sd["post_quant_conv.weight"], sd["post_quant_conv.bias"])
    p = "decoder."
    h = F.conv2d(h, sd[p + "conv_in.weight"], sd[p + "conv_in.bias"], padding=1)
    h = resnet_block_ref(sd, p + "mid.block_2.", resnet_block_ref(sd, p + "mid.block_1.", h))
    for lvl in reversed(range(len(hp["ch_mult"]))):
        for j in range(hp["num_res_blocks"] + 1):
            h = resnet_block_ref(sd, f"{p}up.{lvl}.block.{j}.", h)
        if lvl != 0:
            h = conv2d_ref(h, sd[f"{p}up.{lvl}.upsample.conv.weight"], sd[f"{p}up.{lvl}.upsample.conv.bias"], up2=True)
    return conv2d_ref(h, sd[p + "conv_out.weight"], sd[p + "conv_out.bias"], norm=(sd[p + "norm_out.weight"], sd[p + "norm_out.bias"], 1e-6))


# ---- the sampling loop ----------------------------------------------------------------------------------------------------------------------
class TestScheduler:
    """A deterministic DDIM-style scheduler with diffusers' duck-typed interface, FOR TESTS ONLY (the reference uses diffusers' PNDMScheduler,
    which is not re-implemented).  Coefficients are Python floats, so ``step`` computes in the dtype of its tensors."""
    __test__ = False

    def __init__(self, num_train=1000, beta_start=0.00085, beta_end=0.012):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train, dtype=torch.float64) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0)
        self.num_train = num_train

    def set_timesteps(self, n):
        self.stride = self.num_train // n
        self.timesteps = torch.arange(n - 1, -1, -1) * self.stride + 1

    def scale_model_input(self, x, timestep=None):
        return x

    def step(self, eps, t, x):
        t = int(t)
        a_t = float(self.alphas_cumprod[t])
        a_p = float(self.alphas_cumprod[max(t - self.stride, 0)])
        x0 = (x - math.sqrt(1.0 - a_t) * eps) / math.sqrt(a_t)
        return SimpleNamespace(prev_sample=math.sqrt(a_p) * x0 + math.sqrt(1.0 - a_p) * eps)


def generate_latents_ref(sd, hp, text_embeddings, num_steps, guidance_scale, latents):
    sch = TestScheduler()
    sch.set_timesteps(num_steps)
    for t in sch.timesteps:
        eps = unet_forward(sd, hp, torch.cat([latents] * 2), torch.stack([t, t]), text_embeddings)
        eu, et = eps.chunk(2)
        latents = sch.step(eu + guidance_scale * (et - eu), t, latents).prev_sample
    return latents
