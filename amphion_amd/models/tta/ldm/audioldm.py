"""AudioLDM's denoiser (models/tta/ldm/audioldm.py) in eval mode on the HIP kernels, under the reference's names, constructor arguments and
state_dict keys (prefix ``unet.``).  Only the configuration family of ``config/audioldm.json`` is built: a 2-D UNet with spatial
transformers, ``legacy = false``, ``num_head_channels = -1``, no scale-shift norm, no resblock up / down, no class labels.

Launch plan of one evaluation:
  * ``timestep_embedding`` (cos | sin) is torch on the device; ``time_embed`` and the ``emb_layers`` Linear of ALL ResBlocks are T = 1 products:
    the latter one stacked weight, one ``amp_pw_forward_vec`` per evaluation.
  * a ResBlock is stats -> conv2d (GroupNorm + SiLU on load, ``row_add`` = its embedding rows) -> stats -> conv2d (norm on load, residual =
    x or ``skip_connection(x)``).  The embedding is added BEFORE the second norm, so it enters that norm's statistics.
  * ``Downsample`` is the conv with stride 2, ``Upsample`` the conv reading the x2 nearest up-sampling in place.
  * the context's k | v of all ``attn2`` layers come from one GEMM per context (``prepare_context``), cached on the tensor's identity and
    version.
  * the crop before each skip concatenation and the concatenation itself are torch slicing and ``torch.cat``."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import param_sig
from amphion_amd.modules.hip_ops import Conv2d3x3, group_norm_stats, pw_forward_vec, silu

from .attention import SpatialTransformer, StackedPw, _cf, _lin


def timestep_embedding(timesteps, dim, max_period=10000, repeat_only=False):
    """[N] -> [N, dim]: cos | sin of t * exp(-ln(max_period) * i / half), half = dim // 2 (audioldm.py:81-105)"""
    if repeat_only:
        raise NotImplementedError("timestep_embedding: repeat_only is not built")
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half).to(device=timesteps.device)
    args = timesteps[:, None].float() * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


def _vec(pw, weights, biases, x):
    """the stacked Linear on x [B, cin] as a T = 1 product -> [B, cout]"""
    B = x.shape[0]
    x = x.reshape(B, -1, 1)
    if B <= 8:
        h = pw.get(weights, biases, x.device)
        return pw_forward_vec(h, pw.cout, x)[:, :, 0]
    return pw(weights, biases, x.contiguous())[:, :, 0]


class _EmbRows:
    """the ``emb_layers`` output of every ResBlock of a UNet for one evaluation: [B, sum of out_channels], one row block per block"""

    def __init__(self, rows, offsets):
        self.rows, self.offsets = rows, offsets

    def of(self, block):
        lo, hi = self.offsets[id(block)]
        return self.rows[:, lo:hi]


class _ContextKV:
    """the k | v of every ``attn2`` layer for one context: ``of(transformer)`` is the list a ``SpatialTransformer`` takes"""

    def __init__(self, kv, offsets):
        self.kv, self.offsets = kv, offsets

    def of(self, transformer):
        return [self.kv[:, lo:hi] for lo, hi in self.offsets[id(transformer)]]


class TimestepBlock(nn.Module):
    pass


class TimestepEmbedSequential(nn.Sequential, TimestepBlock):
    def forward(self, x, emb, context=None):
        for layer in self:
            if isinstance(layer, TimestepBlock):
                x = layer(x, emb)
            elif isinstance(layer, SpatialTransformer):
                x = layer(x, context.of(layer) if isinstance(context, _ContextKV) else context)
            elif isinstance(layer, nn.Conv2d):
                x = layer._hip(x, layer.weight, layer.bias)
            else:
                x = layer(x)
        return x


def _conv3(cin, cout, **kw):
    """an nn.Conv2d 3 x 3, padding 1, that holds the parameters; ``_hip`` runs it"""
    c = nn.Conv2d(cin, cout, 3, padding=1, **kw)
    c._hip = Conv2d3x3()
    return c


class Upsample(nn.Module):
    """nearest x2, then ``conv``: the conv reads the up-sampled tensor in place (``up2``)"""

    def __init__(self, channels, use_conv, dims=2, out_channels=None, padding=1):
        super().__init__()
        if dims != 2 or not use_conv or padding != 1:
            raise NotImplementedError("Upsample: only dims=2, use_conv=True, padding=1 is on the HIP path")
        self.channels = channels
        self.out_channels = out_channels or channels
        self.use_conv, self.dims = use_conv, dims
        self.conv = _conv3(self.channels, self.out_channels)

    def forward(self, x):
        return self.conv._hip(x, self.conv.weight, self.conv.bias, up2=True)


class Downsample(nn.Module):
    """``op``: the conv with stride 2 and padding 1"""

    def __init__(self, channels, use_conv, dims=2, out_channels=None, padding=1):
        super().__init__()
        if dims != 2 or not use_conv or padding != 1:
            raise NotImplementedError("Downsample: only dims=2, use_conv=True, padding=1 is on the HIP path")
        self.channels = channels
        self.out_channels = out_channels or channels
        self.use_conv, self.dims = use_conv, dims
        self.op = _conv3(self.channels, self.out_channels, stride=2)

    def forward(self, x):
        return self.op._hip(x, self.op.weight, self.op.bias, stride=2)


class ResBlock(TimestepBlock):
    def __init__(self, channels, emb_channels, dropout, out_channels=None, use_conv=False, use_scale_shift_norm=False, dims=2,
                 use_checkpoint=False, up=False, down=False):
        super().__init__()
        for name, bad in (("use_conv", use_conv), ("use_scale_shift_norm", use_scale_shift_norm), ("dims", dims != 2), ("up", up), ("down", down)):
            if bad:
                raise NotImplementedError(f"ResBlock: {name} is not on the HIP path")
        self.channels = channels
        self.emb_channels = emb_channels
        self.dropout = dropout
        self.out_channels = out_channels or channels
        self.use_checkpoint = use_checkpoint        # runs the function under no_grad in the reference: no effect on values
        self.in_layers = nn.Sequential(nn.GroupNorm(32, channels), nn.SiLU(), _conv3(channels, self.out_channels))
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_channels, self.out_channels))
        self.out_layers = nn.Sequential(nn.GroupNorm(32, self.out_channels), nn.SiLU(), nn.Dropout(p=dropout), _conv3(self.out_channels, self.out_channels))
        for p in self.out_layers[3].parameters():
            p.detach().zero_()
        self.skip_connection = nn.Identity() if self.out_channels == channels else nn.Conv2d(channels, self.out_channels, 1)
        self._emb, self._skip = StackedPw(), StackedPw()

    def forward(self, x, emb):
        """x [B, C, H, W]; emb [B, emb_channels], or the evaluation's ``_EmbRows``"""
        if self.training:
            raise NotImplementedError("ResBlock: training mode is not on the HIP path: call .eval()")
        x = _lib.require_device_tensor(x, "ResBlock input")
        B, C, H, W = x.shape
        if isinstance(emb, _EmbRows):
            rows = emb.of(self)
        else:
            lin = self.emb_layers[1]
            rows = _vec(self._emb, [lin.weight], [lin.bias], silu(_lib.require_device_tensor(emb, "ResBlock emb")))
        n1, c1 = self.in_layers[0], self.in_layers[2]
        n2, c2 = self.out_layers[0], self.out_layers[3]
        h = c1._hip(x, c1.weight, c1.bias, norm=(group_norm_stats(x, n1.eps), n1.weight.detach(), n1.bias.detach()), row_add=rows)
        if isinstance(self.skip_connection, nn.Identity):
            skip = x
        else:
            skip = _lin(self._skip, self.skip_connection, x.reshape(B, C, H * W)).reshape(B, self.out_channels, H, W)
        return c2._hip(h, c2.weight, c2.bias, norm=(group_norm_stats(h, n2.eps), n2.weight.detach(), n2.bias.detach()), residual=skip)


class UNetModel(nn.Module):
    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False, use_fp16=False, num_heads=-1,
                 num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False, use_spatial_transformer=False, transformer_depth=1, context_dim=None, n_embed=None,
                 legacy=True):
        super().__init__()
        for name, bad in (("use_spatial_transformer", not use_spatial_transformer), ("legacy", legacy), ("num_head_channels", num_head_channels != -1),
                          ("num_heads", num_heads == -1), ("num_heads_upsample", num_heads_upsample not in (-1, num_heads)),
                          ("use_scale_shift_norm", use_scale_shift_norm), ("resblock_updown", resblock_updown), ("dims", dims != 2),
                          ("num_classes", num_classes is not None), ("conv_resample", not conv_resample), ("use_fp16", use_fp16),
                          ("n_embed", n_embed is not None), ("context_dim", context_dim is None or isinstance(context_dim, (list, tuple)))):
            if bad:
                raise NotImplementedError(f"UNetModel: {name} is outside the configuration family of config/audioldm.json that the HIP path builds")
        self.image_size = image_size
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = attention_resolutions
        self.dropout = dropout
        self.channel_mult = channel_mult
        self.conv_resample = conv_resample
        self.num_classes = num_classes
        self.use_checkpoint = use_checkpoint
        self.dtype = torch.float32
        self.num_heads = num_heads
        self.num_head_channels = num_head_channels
        self.num_heads_upsample = num_heads
        self.predict_codebook_ids = False

        def res(cin, cout):
            return ResBlock(cin, time_embed_dim, dropout, out_channels=cout, dims=dims, use_checkpoint=use_checkpoint)

        def transformer(ch):
            return SpatialTransformer(ch, num_heads, ch // num_heads, depth=transformer_depth, context_dim=context_dim)

        time_embed_dim = model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(model_channels, time_embed_dim), nn.SiLU(), nn.Linear(time_embed_dim, time_embed_dim))
        self.input_blocks = nn.ModuleList([TimestepEmbedSequential(_conv3(in_channels, model_channels))])
        input_block_chans = [model_channels]
        ch, ds = model_channels, 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [res(ch, mult * model_channels)]
                ch = mult * model_channels
                if ds in attention_resolutions:
                    layers.append(transformer(ch))
                self.input_blocks.append(TimestepEmbedSequential(*layers))
                input_block_chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(TimestepEmbedSequential(Downsample(ch, conv_resample, dims=dims, out_channels=ch)))
                input_block_chans.append(ch)
                ds *= 2
        self.middle_block = TimestepEmbedSequential(res(ch, ch), transformer(ch), res(ch, ch))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = input_block_chans.pop()
                layers = [res(ch + ich, model_channels * mult)]
                ch = model_channels * mult
                if ds in attention_resolutions:
                    layers.append(transformer(ch))
                if level and i == num_res_blocks:
                    layers.append(Upsample(ch, conv_resample, dims=dims, out_channels=ch))
                    ds //= 2
                self.output_blocks.append(TimestepEmbedSequential(*layers))
        self.out = nn.Sequential(nn.GroupNorm(32, ch), nn.SiLU(), _conv3(model_channels, out_channels))
        for p in self.out[2].parameters():
            p.detach().zero_()
        self._te0, self._te2, self._embs, self._ctx = StackedPw(), StackedPw(), StackedPw(), StackedPw()
        self._ctx_cache = None          # (signature, _ContextKV, the context tensor)
        # the step-level products' operands, gathered once (plain lists: not registered a second time)
        self._res_list = [m for m in self.modules() if isinstance(m, ResBlock)]
        self._st_list = [m for m in self.modules() if isinstance(m, SpatialTransformer)]
        self._kv_weights = [w for st in self._st_list for blk in st.transformer_blocks for w in (blk.attn2.to_k.weight, blk.attn2.to_v.weight)]

    # ---- the two step-level products ----
    def _emb_rows(self, timesteps):
        t_emb = timestep_embedding(timesteps, self.model_channels).contiguous()
        l0, l2 = self.time_embed[0], self.time_embed[2]
        e = _vec(self._te2, [l2.weight], [l2.bias], silu(_vec(self._te0, [l0.weight], [l0.bias], t_emb).contiguous()))
        blocks = self._res_list
        lins = [b.emb_layers[1] for b in blocks]
        rows = _vec(self._embs, [l.weight for l in lins], [l.bias for l in lins], silu(e.contiguous()))
        offsets, lo = {}, 0
        for b in blocks:
            offsets[id(b)] = (lo, lo + b.out_channels)
            lo += b.out_channels
        return _EmbRows(rows, offsets)

    def prepare_context(self, context):
        """k | v of every ``attn2`` layer for ``context`` [B, Tk, context_dim] in one GEMM.  The result is kept for the tensor's identity and
        in-place version (and the weights'): the sampler's loop forms it once."""
        sts, weights = self._st_list, self._kv_weights
        sig = param_sig([context] + weights, tuple(context.shape), str(context.device), _lib.get_precision())
        if self._ctx_cache is not None and self._ctx_cache[0] == sig:
            return self._ctx_cache[1]
        ctx = _cf(context.transpose(1, 2).contiguous(), "UNetModel context")
        kv = self._ctx(weights, [None] * len(weights), ctx)
        offsets, lo = {}, 0
        for st in sts:
            offsets[id(st)] = []
            for blk in st.transformer_blocks:
                offsets[id(st)].append((lo, lo + 2 * blk.attn2.inner_dim))
                lo += 2 * blk.attn2.inner_dim
        out = _ContextKV(kv, offsets)
        self._ctx_cache = (sig, out, context)      # holding the tensor keeps its address from being reused by another
        return out

    def forward(self, x, timesteps=None, context=None, y=None, **kwargs):
        """x [N, C, H, W], timesteps [N], context [N, Tk, context_dim] -> [N, out_channels, H, W]"""
        if self.training:
            raise NotImplementedError("UNetModel: training mode is not on the HIP path: call .eval()")
        if y is not None:
            raise NotImplementedError("UNetModel: y (class labels) is not built")
        if context is None:
            raise NotImplementedError("UNetModel: context=None is not built (AudioLDM always conditions on text)")
        x = _lib.require_device_tensor(x, "UNetModel input")
        emb = self._emb_rows(timesteps.to(x.device))
        ctx = self.prepare_context(context)
        hs = []
        h = x
        for module in self.input_blocks:
            h = module(h, emb, ctx)
            hs.append(h)
        h = self.middle_block(h, emb, ctx)
        for module in self.output_blocks:
            skip = hs.pop()
            if h.shape != skip.shape:            # an odd extent halved and doubled: crop to the skip's (audioldm.py:891-896)
                h = h[:, :, : skip.shape[-2], : skip.shape[-1]]
            h = module(torch.cat([h, skip], dim=1), emb, ctx)
        n, c = self.out[0], self.out[2]
        return c._hip(h, c.weight, c.bias, norm=(group_norm_stats(h, n.eps), n.weight.detach(), n.bias.detach()))


class AudioLDM(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.unet = UNetModel(image_size=cfg.image_size, in_channels=cfg.in_channels, out_channels=cfg.out_channels,
                              model_channels=cfg.model_channels, attention_resolutions=list(cfg.attention_resolutions),
                              num_res_blocks=cfg.num_res_blocks, channel_mult=list(cfg.channel_mult), num_heads=cfg.num_heads,
                              use_spatial_transformer=cfg.use_spatial_transformer, transformer_depth=cfg.transformer_depth,
                              context_dim=cfg.context_dim, use_checkpoint=cfg.use_checkpoint, legacy=cfg.legacy)

    def prepare_context(self, context):
        return self.unet.prepare_context(context)

    def forward(self, x, timesteps=None, context=None, y=None):
        return self.unet(x=x, timesteps=timesteps, context=context, y=y)
