"""Thin torch-tensor wrappers over the op-level C ABI (conv + VITS element-wise kernels)."""
from __future__ import annotations

import ctypes

import torch

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import ptr as _ptr
from amphion_amd.models.vocoders.gan.generator._engine import ConvParams


class HipConv1d(ConvParams):
    """A Conv1d / ConvTranspose1d whose forward is the fused gfx950 implicit-GEMM kernel:
    ``y = lrelu_out(conv(lrelu_in(x)) + bias + res)``.  Parameters keep torch's key names
    (``weight``/``bias`` or ``weight_g``/``weight_v`` under weight-norm); the packed device copy is
    rebuilt lazily when they change."""

    def __init__(self, *a, pad_mode="zeros", tanh=False, **k):
        super().__init__(*a, **k)
        if pad_mode not in ("zeros", "reflect"):
            raise ValueError(f"pad_mode must be 'zeros' or 'reflect', got {pad_mode!r}")
        self.pad_mode, self.tanh = pad_mode, bool(tanh)
        self._cache, self._gated = HandleCache("amp_conv_destroy"), HandleCache("amp_conv_destroy")

    def _param_sig(self):
        """identity + version of every parameter (a leaf module: its own ``_parameters`` only -- ``named_parameters()`` walks the
        module tree with prefixes and costs several microseconds per launch)"""
        return tuple((n, p.data_ptr(), p._version) for n, p in self._parameters.items() if p is not None)

    def _ensure(self, device):
        # keyed on the parameters and the device, NOT on the precision (every other cache is): a handle keeps the arithmetic it was built
        # with (amphion_hip.h) and ``_prec`` records it.  The look-up is HandleCache.get spelled out: this is the per-launch path
        c, sig = self._cache, self._param_sig() + (device,)
        return c.handle if sig == c.sig else c.build(sig, self._build, device)

    def _build(self, device):
        w, b = host_f32(self.folded_weight()), host_f32(self.bias)
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_conv_create(int(self.transposed), self.cin, self.cout, self.k, self.stride,
                                                  self.dilation, self.padding, _ptr(w), _ptr(b), ctypes.byref(h)))
            self._cache.adopt(h)
            if self.pad_mode == "reflect":
                _lib.check(_lib.lib().amp_conv_set_option(h, _lib.AMP_CONV_OPT_PAD_REFLECT, 1))
            if self.tanh:
                _lib.check(_lib.lib().amp_conv_set_option(h, _lib.AMP_CONV_OPT_TANH, 1))
        self._prec = _lib.get_precision()
        return h

    def _ensure_gated(self, device):
        """A second handle with the 2H rows packed for the gate epilogue of the fused WN layer
        (``amp_conv_create_gated``); None when this conv / arithmetic is outside what that kernel covers."""
        c, sig = self._gated, self._param_sig() + (device, _lib.get_precision())
        return c.handle if sig == c.sig else c.build(sig, self._build_gated, device)

    def _build_gated(self, device):
        if (_lib.get_precision() != "f16x3" or self.transposed or self.cout != 2 * self.cin or self.cin % 32 or self.cin > 256 or self.cout <= 64
                or self.k not in (1, 3, 5) or self.stride != 1 or 2 * self.padding != self.dilation * (self.k - 1)
                or (self.k - 1) * self.dilation > 64 or self.pad_mode != "zeros" or self.tanh):
            return None
        w, b = host_f32(self.folded_weight()), host_f32(self.bias)
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_conv_create_gated(self.cin, self.k, self.dilation, self.padding, _ptr(w), _ptr(b), ctypes.byref(h)))
        return h

    def forward(self, x, *, slope_in=1.0, res=None, slope_out=1.0, out=None, x_batch_stride=None, T=None, lens=None):
        """x [B, cin, T] (or a channel slice of a wider tensor when ``x_batch_stride`` is given).  ``lens`` (int32 [B] on the
        device): conv(x * mask) with the mask taken by the kernel -- output columns beyond an item's length are UNSPECIFIED
        (``amp_conv_forward_ragged``)."""
        x = _lib.require_device_tensor(x, "conv input") if x_batch_stride is None else x
        dev = x.device
        B = x.shape[0]
        T = x.shape[-1] if T is None else T
        L = _lib.lib()
        h = self._ensure(dev)
        # amp_conv_out_len, without the call
        Tout = (T - 1) * self.stride - 2 * self.padding + self.k if self.transposed else T + 2 * self.padding - self.dilation * (self.k - 1)
        if out is None:
            out = torch.empty((B, self.cout, Tout), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            if lens is not None:
                _lib.check(L.amp_conv_forward_ragged(h, _ptr(x), int(x_batch_stride or 0), B, T, _ptr(lens), slope_in, _ptr(res),
                                                     slope_out, _ptr(out), _lib.current_stream_ptr(dev)))
            elif x_batch_stride is None:
                _lib.check(L.amp_conv_forward(h, _ptr(x), B, T, slope_in, _ptr(res), slope_out, _ptr(out),
                                              _lib.current_stream_ptr(dev)))
            else:
                _lib.check(L.amp_conv_forward_strided(h, _ptr(x), int(x_batch_stride), B, T, slope_in, _ptr(res),
                                                      slope_out, _ptr(out), _lib.current_stream_ptr(dev)))
        return out


class MergedConv1d:
    """Several ``HipConv1d`` that read the same input (the q / k / v projections of an attention layer), run as ONE launch: their
    folded weights stacked along the output rows in one handle -> [B, sum(cout), T].  Not a module and it owns no parameters: the
    convs are passed at every call, this object only caches the packed device copy (rebuilt when a parameter changes; a copy /
    pickle of the owning module starts with an empty cache)."""

    def __init__(self):
        self._cache = HandleCache("amp_conv_destroy")

    def _ensure(self, convs, device):
        # like HipConv1d._ensure: not keyed on the precision, and spelled out for the per-launch path
        cache, sig = self._cache, tuple(c._param_sig() for c in convs) + (device,)
        return cache.handle if sig == cache.sig else cache.build(sig, self._build, convs, device)

    def _build(self, convs, device):
        c0 = convs[0]
        if any(c.transposed or (c.cin, c.k, c.stride, c.dilation, c.padding) != (c0.cin, c0.k, c0.stride, c0.dilation, c0.padding)
               or (c.bias is None) != (c0.bias is None) for c in convs):
            raise ValueError("MergedConv1d: the convs must be Conv1d of one geometry")
        w = torch.cat([host_f32(c.folded_weight()) for c in convs], dim=0)
        b = torch.cat([host_f32(c.bias) for c in convs]) if c0.bias is not None else None
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_conv_create(0, c0.cin, w.shape[0], c0.k, c0.stride, c0.dilation, c0.padding, _ptr(w), _ptr(b),
                                                  ctypes.byref(h)))
        return h

    def __call__(self, convs, x, lens=None):
        x = _lib.require_device_tensor(x, "conv input")
        B, _, T = x.shape
        h = self._ensure(convs, x.device)
        out = torch.empty((B, sum(c.cout for c in convs), T), dtype=torch.float32, device=x.device)
        with _lib.on_device(x.device):
            _lib.check(_lib.lib().amp_conv_forward_ragged(h, _ptr(x), 0, B, T, _ptr(lens), 1.0, None, 1.0, _ptr(out),
                                                          _lib.current_stream_ptr(x.device)))
        return out


def lens_tensor(lengths, device):
    """int32 device tensor of valid lengths (sequence_mask argument), or None."""
    if lengths is None:
        return None
    return torch.as_tensor(lengths).to(device=device, dtype=torch.int32).contiguous()


def wn_fused(in_layers, res_skip_layers, x, cond, lens, out, acts):
    """The whole WN stack on the fused kernels (``amp_wn_forward``): two launches per layer.  ``x`` is modified.
    Returns False (nothing launched) when a layer is outside what the fused kernels cover -- the caller then runs the
    unfused ops."""
    dev = x.device
    n = len(in_layers)
    H = x.shape[1]
    hi, hr = [], []
    for i in range(n):
        rs = res_skip_layers[i]
        if (rs.k != 1 or rs.cin != H or rs.cout != (2 * H if i < n - 1 else H) or rs.cout <= 64 or rs.bias is None or rs.transposed or rs.tanh
                or rs.pad_mode != "zeros"):      # cout <= 64: fewer than the 128 rows the whole-K kernel's workgroups cover (H <= 64)
            return False
        g = in_layers[i]._ensure_gated(dev)
        if g is None:
            return False
        hr_i = rs._ensure(dev)
        if getattr(rs, "_prec", None) != "f16x3":       # a res_skip handle built while the exact-fp32 mode was selected
            return False
        hi.append(g.value)
        hr.append(hr_i.value)
    B, _, T = x.shape
    arr_i = (ctypes.c_void_p * n)(*hi)
    arr_r = (ctypes.c_void_p * n)(*hr)
    bs = cond.stride(0) if cond is not None else 0
    with _lib.on_device(dev):
        _lib.check(_lib.lib().amp_wn_forward(arr_i, arr_r, n, _ptr(x), _ptr(cond), bs, _ptr(lens), B, T, _ptr(acts), _ptr(out),
                                             _lib.current_stream_ptr(dev)))
    return True


def wn_gate(a, cond, out):
    B, H2, T = a.shape
    bs = cond.stride(0) if cond is not None else 0
    _lib.check(_lib.lib().amp_wn_gate(_ptr(a), _ptr(cond), bs, _ptr(out), B, H2 // 2, T, _lib.current_stream_ptr(a.device)))
    return out


def wn_accumulate(x, out, rs, lens, first, last):
    B, H, T = x.shape
    _lib.check(_lib.lib().amp_wn_accumulate(_ptr(x), _ptr(out), _ptr(rs), _ptr(lens), B, H, T, int(first), int(last),
                                            _lib.current_stream_ptr(x.device)))


def sequence_mask_(x, lens):
    B, C, T = x.shape
    _lib.check(_lib.lib().amp_sequence_mask(_ptr(x), _ptr(lens), B, C, T, _lib.current_stream_ptr(x.device)))
    return x


def coupling_apply_(x, m, lens, reverse):
    B, C, T = x.shape
    _lib.check(_lib.lib().amp_coupling_apply(_ptr(x), _ptr(m), _ptr(lens), B, C // 2, T, int(reverse),
                                             _lib.current_stream_ptr(x.device)))
    return x


def flip_channels(x):
    B, C, T = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.lib().amp_flip_channels(_ptr(x), _ptr(y), B, C, T, _lib.current_stream_ptr(x.device)))
    return y


def posterior_sample(stats, eps, lens):
    B, C2, T = stats.shape
    z = torch.empty((B, C2 // 2, T), dtype=torch.float32, device=stats.device)
    _lib.check(_lib.lib().amp_posterior_sample(_ptr(stats), _ptr(eps), _ptr(lens), _ptr(z), B, C2 // 2, T,
                                               _lib.current_stream_ptr(stats.device)))
    return z


# ---- frame-rate ops of VITS' text -> duration -> alignment front ----------------
def _stream(t):
    return _lib.current_stream_ptr(t.device)


def layer_norm_c(x, gamma, beta, res=None, post=None, eps=1e-5, gelu=False, lens=None):
    """post + act(LN(x + res)) over the channel axis; with ``lens`` the columns beyond an item's length are written as zero
    (whatever x / res hold there)"""
    B, C, T = x.shape
    y = torch.empty_like(x)
    if lens is None:
        _lib.check(_lib.lib().amp_layer_norm_c(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(post), B, C, T, float(eps), int(gelu),
                                               _ptr(y), _stream(x)))
    else:
        _lib.check(_lib.lib().amp_layer_norm_c_ragged(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(post), _ptr(lens), B, C, T,
                                                      float(eps), int(gelu), _ptr(y), _stream(x)))
    return y


def layer_norm_c_style(x, style, res=None, eps=1e-5):
    """style[b, :C] * LN(x + res) + style[b, C:] over the channel axis, LN without an affine: x [B, C, T], style [B, 2C] (or [B, 2C, 1]), one
    scale | shift row per item (``amp_layer_norm_c_style``)"""
    x = _lib.require_device_tensor(x, "layer_norm_c_style input")
    style = _lib.require_device_tensor(style, "style")
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError(f"layer_norm_c_style: expected a non-empty [B, C, T] input, got {tuple(x.shape)}")
    B, C, T = x.shape
    if style.numel() != B * 2 * C or style.shape[0] != B or style.device != x.device:
        raise ValueError(f"layer_norm_c_style: expected a style of shape {(B, 2 * C)} on {x.device}, got {tuple(style.shape)} on {style.device}")
    if res is not None:
        res = _lib.require_device_tensor(res, "layer_norm_c_style residual")
        if res.shape != x.shape or res.device != x.device:
            raise ValueError(f"layer_norm_c_style: the residual must be {tuple(x.shape)} on {x.device}, got {tuple(res.shape)} on {res.device}")
    y = torch.empty_like(x)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().amp_layer_norm_c_style(_ptr(x), _ptr(res), _ptr(style), B, C, T, float(eps), _ptr(y), _stream(x)))
    return y


_embed_sum_flags = {}     # device -> the int32 word that amp_embed_sum_c raises for an index outside its table


def _embed_sum_flag(dev):
    flag = _embed_sum_flags.get(dev)
    if flag is None:
        flag = _embed_sum_flags[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return flag


def embed_sum_check(device):
    """Synchronise the current stream of ``device`` and raise ``AmpError`` (AMP_ERR_INVALID) if an ``embed_sum_c(..., check=False)`` since the
    last check met an index outside its table (``amp_embed_sum_check``; the flag is cleared)"""
    device = torch.device(device)
    with _lib.on_device(device):
        _lib.check(_lib.lib().amp_embed_sum_check(_ptr(_embed_sum_flag(device)), _lib.current_stream_ptr(device)))


def embed_sum_c(codes, tables, init=None, check=True):
    """codes integers [N, B, T], tables: N weights [rows_n, D] -> ((init + W_0[codes[0]]) + W_1[codes[1]]) + ... as [B, D, T], the fp32 adds
    left to right (``amp_embed_sum_c``: torch's ``emb_0(c_0) + emb_1(c_1) + ...`` transposed, bit for bit).  ``init`` [B, D, T] or None.  An
    index outside its table raises ``AmpError`` (AMP_ERR_INVALID) -- here, or with ``check=False`` at the caller's ``embed_sum_check``, which a
    caller of several sums runs once behind them (the check synchronises)."""
    N = len(tables)
    if not isinstance(codes, torch.Tensor) or codes.dim() != 3 or codes.shape[0] != N or codes.shape[1] < 1 or codes.shape[2] < 1:
        raise ValueError(f"embed_sum_c: expected codes [{N}, B, T], got {tuple(codes.shape) if isinstance(codes, torch.Tensor) else type(codes)}")
    if not 1 <= N <= 8:
        raise ValueError(f"embed_sum_c: {N} tables (1..8)")
    if codes.dtype.is_floating_point or codes.dtype == torch.bool:
        raise TypeError(f"embed_sum_c: the codes must be integers, got {codes.dtype}")
    if not codes.is_cuda:
        raise RuntimeError("embed_sum_c: the codes must be a tensor on a ROCm device (there is no CPU fallback)")
    dev = codes.device
    tables = [_lib.require_device_tensor(w.detach(), "embedding table") for w in tables]
    D = tables[0].shape[-1]
    if any(w.dim() != 2 or w.shape[1] != D or w.shape[0] < 1 or w.device != dev for w in tables):
        raise ValueError(f"embed_sum_c: every table must be [rows, {D}] on {dev}, got {[(tuple(w.shape), str(w.device)) for w in tables]}")
    codes = codes.to(torch.int64).contiguous()
    _, B, T = codes.shape
    if init is not None:
        init = _lib.require_device_tensor(init, "embed_sum_c init")
        if tuple(init.shape) != (B, D, T) or init.device != dev:
            raise ValueError(f"embed_sum_c: init must be {(B, D, T)} on {dev}, got {tuple(init.shape)} on {init.device}")
    flag = _embed_sum_flag(dev)
    y = torch.empty((B, D, T), dtype=torch.float32, device=dev)
    ptrs = (ctypes.c_void_p * N)(*[w.data_ptr() for w in tables])
    rows = (ctypes.c_int * N)(*[w.shape[0] for w in tables])
    with _lib.on_device(dev):
        st = _lib.current_stream_ptr(dev)
        _lib.check(_lib.lib().amp_embed_sum_c(_ptr(codes), N, ptrs, rows, D, _ptr(init), B, T, _ptr(y), _ptr(flag), st))
        if check:
            _lib.check(_lib.lib().amp_embed_sum_check(_ptr(flag), st))
    return y


def dwconv_layer_norm_c(x, weight, bias, dilation, gamma, beta, lens=None, eps=1e-5, gelu=False):
    """act(LN(dwconv(x * mask))) in one launch (DDSConv's convs_sep + norms_1, modules/flow/modules.py:63-65); K = 3"""
    B, C, T = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.lib().amp_dwconv_layer_norm_c(_ptr(x), _ptr(weight), _ptr(bias), weight.shape[-1], int(dilation), _ptr(gamma),
                                                  _ptr(beta), _ptr(lens), B, C, T, float(eps), int(gelu), _ptr(y), _stream(x)))
    return y


def dds_seam(y, x, n2, sep, n1, lens=None):
    """The seam between DDSConv layers i and i + 1 in one launch: ``x_new = x + gelu(n2(y))``; ``z = gelu(n1(sep(x_new * mask)))``
    -> (x_new, z), or None when the shape is outside the fused kernel (depthwise K = 3, C <= 192)."""
    B, C, T = y.shape
    w = sep.weight.detach()
    if w.shape[-1] != 3 or C > 192:
        return None
    xo, zo = torch.empty_like(y), torch.empty_like(y)
    _lib.check(_lib.lib().amp_dds_seam(_ptr(y), _ptr(x), _ptr(n2.gamma.detach()), _ptr(n2.beta.detach()), float(n2.eps), _ptr(w.contiguous()),
                                       _ptr(sep.bias.detach()), 3, int(sep.dilation), _ptr(n1.gamma.detach()), _ptr(n1.beta.detach()),
                                       float(n1.eps), _ptr(lens), B, C, T, _ptr(xo), _ptr(zo), _stream(y)))
    return xo, zo


def add_channel_bias_(x, cb):
    """x [B, C, T] += cb [B, C, 1] in place (x + cond(g) for a length-1 condition)"""
    B, C, T = x.shape
    _lib.check(_lib.lib().amp_add_channel_bias(_ptr(x), _ptr(cb.reshape(B, C).contiguous()), B, C, T, _stream(x)))
    return x


def rel_attention(q, k, v, emb_k, emb_v, lens, n_heads, window):
    B, C, T = q.shape
    out = torch.empty_like(q)
    _lib.check(_lib.lib().amp_rel_attention(_ptr(q), _ptr(k), _ptr(v), _ptr(emb_k), _ptr(emb_v), _ptr(lens), B, n_heads, C // n_heads, T,
                                            int(window), _ptr(out), _stream(q)))
    return out


def rel_attention_qkv(qkv, emb_k, emb_v, lens, n_heads, window):
    """the same on the output [B, 3C, T] of a merged q | k | v projection (no copies: the three slices share a batch stride)"""
    B, C3, T = qkv.shape
    C = C3 // 3
    out = torch.empty((B, C, T), dtype=torch.float32, device=qkv.device)
    p = qkv.data_ptr()
    step = C * T * 4
    _lib.check(_lib.lib().amp_rel_attention_strided(ctypes.c_void_p(p), ctypes.c_void_p(p + step), ctypes.c_void_p(p + 2 * step), C3 * T,
                                                    _ptr(emb_k), _ptr(emb_v), _ptr(lens), B, n_heads, C // n_heads, T, int(window),
                                                    _ptr(out), _stream(qkv)))
    return out


def dwconv(x, weight, bias, lens, dilation):
    B, C, T = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.lib().amp_dwconv(_ptr(x), _ptr(weight), _ptr(bias), _ptr(lens), B, C, T, weight.shape[-1], int(dilation), _ptr(y), _stream(x)))
    return y


def spline_flow(z, h, lens, num_bins, filter_channels, tail_bound, inverse, flip_in=False, flip_out=False):
    B, _, T = z.shape
    out = torch.empty_like(z)
    _lib.check(_lib.lib().amp_spline_flow(_ptr(z), _ptr(h), _ptr(lens), B, T, int(num_bins), int(filter_channels), float(tail_bound),
                                          int(inverse), int(flip_in), int(flip_out), _ptr(out), _stream(z)))
    return out


def spline_flow_proj(z, hc, proj_w, proj_b, lens, num_bins, filter_channels, tail_bound, inverse, flip_in=False, flip_out=False):
    """ConvFlow's ``proj`` (1 x 1 conv to the 3K - 1 spline parameters) and the spline step in one launch; hc [B, C, T] is the DDSConv
    output (its columns beyond the lengths are never used)"""
    B, _, T = z.shape
    C = hc.shape[1]
    out = torch.empty_like(z)
    _lib.check(_lib.lib().amp_spline_flow_proj(_ptr(z), _ptr(hc), _ptr(proj_w), _ptr(proj_b), _ptr(lens), B, C, T, int(num_bins),
                                               int(filter_channels), float(tail_bound), int(inverse), int(flip_in), int(flip_out), _ptr(out),
                                               _stream(z)))
    return out


def affine_reverse(x, m, logs, lens):
    B, C, T = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.lib().amp_affine_reverse(_ptr(x), _ptr(m), _ptr(logs), _ptr(lens), B, C, T, _ptr(y), _stream(x)))
    return y


def embed_tokens(tokens, weight, lens, scale):
    B, T = tokens.shape
    n_vocab, hidden = weight.shape
    y = torch.empty((B, hidden, T), dtype=torch.float32, device=weight.device)
    _lib.check(_lib.lib().amp_embed_tokens(_ptr(tokens), _ptr(weight), _ptr(lens), B, T, hidden, n_vocab, float(scale), _ptr(y), _stream(weight)))
    return y


def durations(logw, lens, length_scale):
    """-> (w_ceil [B, 1, T] float, cum [B, T] int32, y_lengths [B] int32)"""
    B, _, T = logw.shape
    w_ceil = torch.empty_like(logw)
    cum = torch.empty((B, T), dtype=torch.int32, device=logw.device)
    ylen = torch.empty((B,), dtype=torch.int32, device=logw.device)
    _lib.check(_lib.lib().amp_durations(_ptr(logw), _ptr(lens), B, T, float(length_scale), _ptr(w_ceil), _ptr(cum), _ptr(ylen), _stream(logw)))
    return w_ceil, cum, ylen


def expand_path(src, cum, xlens, ylens, t_y, want_attn=False):
    """src [B, D, Tx]: contiguous, or a channel slice of a wider [B, D', Tx] tensor (the halves of the text encoder's stats) --
    read in place through its batch stride"""
    B, D, Tx = src.shape
    if src.stride(2) != 1 or src.stride(1) != Tx or (B > 1 and src.stride(0) < D * Tx):
        src = src.contiguous()
    out = torch.empty((B, D, t_y), dtype=torch.float32, device=src.device)
    attn = torch.empty((B, 1, t_y, Tx), dtype=torch.float32, device=src.device) if want_attn else None
    _lib.check(_lib.lib().amp_expand_path_strided(_ptr(src), int(src.stride(0)) if B > 1 else D * Tx, _ptr(cum), _ptr(xlens), _ptr(ylens), B, D,
                                                  Tx, int(t_y), _ptr(out), _ptr(attn), _stream(src)))
    return out, attn


def gauss_sample(m, logs, noise, noise_scale):
    out = torch.empty_like(m)
    _lib.check(_lib.lib().amp_gauss_sample(_ptr(m), _ptr(logs), _ptr(noise), m.numel(), float(noise_scale), _ptr(out), _stream(m)))
    return out


# ---- the non-autoregressive Llama of Vevo / MaskGCT (csrc/llama_nar.hip) ----------------
def silu(x, out=None):
    """nn.SiLU element-wise (``amp_silu``); ``out`` may be ``x``"""
    x = _lib.require_device_tensor(x, "silu input")
    if x.numel() == 0:
        raise ValueError(f"silu: empty input {tuple(x.shape)}")
    out = _out_like("silu", out, x)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().amp_silu(_ptr(x), x.numel(), _ptr(out), _stream(x)))
    return out


def swiglu(gu):
    """gu [B, 2F, T], the output of one stacked gate | up GEMM -> silu(gu[:, :F]) * gu[:, F:] [B, F, T] (``amp_swiglu``)"""
    gu = _lib.require_device_tensor(gu, "swiglu input")
    if gu.dim() != 3 or gu.numel() == 0 or gu.shape[1] % 2:
        raise ValueError(f"swiglu: expected a non-empty [B, 2F, T] input, got {tuple(gu.shape)}")
    B, F2, T = gu.shape
    y = torch.empty((B, F2 // 2, T), dtype=torch.float32, device=gu.device)
    with _lib.on_device(gu.device):
        _lib.check(_lib.lib().amp_swiglu(_ptr(gu), B, F2 // 2, T, _ptr(y), _stream(gu)))
    return y


def rms_norm_c_adaptive(x, w, eps=1e-6):
    """w[b, c] * x[b, c, t] * rsqrt(mean_c x[b, :, t]^2 + eps): x [B, C, T]; w [B, C] or [B, C, 1], one row per item, which may be a slice
    of a wider tensor -- it is read in place through its batch stride (``amp_rms_norm_c_adaptive``)"""
    x = _lib.require_device_tensor(x, "rms_norm_c_adaptive input")
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError(f"rms_norm_c_adaptive: expected a non-empty [B, C, T] input, got {tuple(x.shape)}")
    B, C, T = x.shape
    if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.float32 or w.device != x.device:
        raise ValueError(f"rms_norm_c_adaptive: the weight must be a float32 tensor on {x.device}")
    if w.dim() == 3 and w.shape[2] == 1:
        w = w[:, :, 0]
    if w.dim() != 2 or tuple(w.shape) != (B, C):
        raise ValueError(f"rms_norm_c_adaptive: expected a weight of shape {(B, C)}, got {tuple(w.shape)}")
    w, wbs = _rows_2d(w, C)
    y = torch.empty_like(x)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().amp_rms_norm_c_adaptive(_ptr(x), _ptr(w), wbs, B, C, T, float(eps), _ptr(y), _stream(x)))
    return y


_rope_tables = {}     # (T, dk, theta, device) -> (cos, sin) [T, dk / 2]


def rope_tables(T, dk, device, theta=10000.0):
    """cos, sin [T, dk/2] fp32 as HF's ``LlamaRotaryEmbedding`` computes them (inv_freq = theta^(-2i/dk), positions 0 .. T-1, fp32), once
    per (T, dk, theta, device)"""
    key = (int(T), int(dk), float(theta), str(device))
    t = _rope_tables.get(key)
    if t is None:
        inv_freq = 1.0 / (theta ** (torch.arange(0, dk, 2, dtype=torch.int64).to(device=device, dtype=torch.float32) / dk))
        freqs = torch.arange(T, device=device, dtype=torch.float32)[:, None] * inv_freq[None, :]
        if len(_rope_tables) >= 64:
            _rope_tables.clear()
        t = _rope_tables[key] = (freqs.cos().contiguous(), freqs.sin().contiguous())
    return t


def _rows_view(t, C, T, bstride):
    """is ``t`` [B, C, T] laid out as the kernel reads it: unit column stride, rows T apart, batch stride ``bstride``"""
    return t.stride(2) == 1 and (C == 1 or t.stride(1) == T) and (t.shape[0] == 1 or t.stride(0) == bstride)


def _row_blocks(tensors, C, T):
    """``tensors`` [B, C, T] as a kernel with ONE batch stride for all of them reads them -> (tensors, batch stride): in place when every one
    is contiguous or a row block of a wider tensor (``_rows_view``) at one batch stride >= C * T, else contiguous copies of all of them"""
    t0 = tensors[0]
    bstride = t0.stride(0) if t0.shape[0] > 1 else max(t0.stride(0), C * T)
    if bstride >= C * T:
        for t in tensors:
            if not _rows_view(t, C, T, bstride):
                break
        else:
            return tensors, bstride
    return [t.contiguous() for t in tensors], C * T


def _rows_2d(t, C):
    """``t`` [B, C], one row per item, as a kernel reads it -> (t, batch stride): in place when the rows are contiguous and at least C apart
    (a slice of a wider tensor), else a contiguous copy.  The stride of a single row is C"""
    B = t.shape[0]
    if (C > 1 and t.stride(1) != 1) or (B > 1 and t.stride(0) < C):
        t = t.contiguous()
    return t, int(t.stride(0)) if B > 1 else C


def _f32_dev(t, name, who):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be a float32 tensor on a ROCm device (the HIP path has no CPU fallback)")
    return t


def _key_mask_u8(who, key_mask, B, Tk, device):
    """a key mask [B, Tk] (nonzero = valid) as the contiguous bytes the attention kernels read; None stays None"""
    if key_mask is None:
        return None
    if not isinstance(key_mask, torch.Tensor) or tuple(key_mask.shape) != (B, Tk) or key_mask.device != device:
        raise ValueError(f"{who}: key_mask must be a {(B, Tk)} tensor on {device}")
    if key_mask.dtype != torch.uint8:
        key_mask = (key_mask != 0).to(torch.uint8)
    return key_mask.contiguous()


def _heads(who, C, n_heads, dks):
    """(H, dk) of C channels in ``n_heads`` heads, for a kernel that covers the head dimensions ``dks``"""
    H = int(n_heads)
    if H < 1 or C % H:
        raise ValueError(f"{who}: {C} channels do not divide into {H} heads")
    dk = C // H
    if dk not in dks:
        raise ValueError(f"{who}: head dimension {dk} is not covered (dk = {' / '.join(map(str, dks))})")
    return H, dk


def _sdpa_cf(q, k, v, H, mask, scale):
    """the exact-fp32 route of the attention functions: ``scaled_dot_product_attention`` on channel-first q [B, H*dk, Tq] and k, v
    [B, H*dk, Tk] under the boolean ``mask`` (broadcastable to [B, H, Tq, Tk], True = visible, or None) -> [B, H*dk, Tq].  q and k may come
    with their heads split already, as [B, H, T, dk] (``rope_attention`` rotates them in that form)"""
    B, C, Tq = v.shape[0], v.shape[1], q.shape[-1] if q.dim() == 3 else q.shape[2]
    qq, kk, vv = (t if t.dim() == 4 else t.reshape(B, H, C // H, t.shape[2]).transpose(2, 3) for t in (q, k, v))
    o = torch.nn.functional.scaled_dot_product_attention(qq, kk, vv, attn_mask=mask, scale=scale)
    return o.transpose(2, 3).reshape(B, C, Tq).contiguous()


def _out_like(who, out, x):
    """the ``out`` argument of an element-wise op on x: a new tensor, or the caller's contiguous float32 tensor of x's shape on x's device"""
    if out is None:
        return torch.empty_like(x)
    if out.shape != x.shape or out.device != x.device or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous float32 {tuple(x.shape)} on {x.device}")
    return out


def _vec_input(who, x):
    """the [B, cin, 1] column of the T = 1 Linears -> (x, B, cin, batch stride): read in place when it is a row block of a wider tensor"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
        _f32_dev(x, "x", who)
    if x.dim() != 3 or x.shape[2] != 1 or x.numel() == 0:
        raise ValueError(f"{who}: expected a [B, cin, 1] input, got {tuple(x.shape)}")
    B, cin = x.shape[0], x.shape[1]
    # _rows_2d's rule, spelled out: every Linear of a decode step comes through here, and the step is bound by host work per launch
    if (cin > 1 and x.stride(1) != 1) or (B > 1 and x.stride(0) < cin):
        x = x.contiguous()
    return x, B, cin, int(x.stride(0)) if B > 1 else cin


def rope_attention(q, k, v, n_heads, cos, sin, key_mask=None, scale=None, causal=False):
    """Non-causal multi-head self-attention with rotary position embedding (HF's rotate-half form) and a KEY mask (``amp_rope_attention``).

    q, k, v [B, H*dk, T] channel-first: contiguous tensors, or the three row blocks of one stacked [B, 3*H*dk, T] GEMM output (read in
    place: no copy).  cos, sin [T, dk/2] (``rope_tables``).  key_mask [B, T] bool / uint8, 1 = valid, any pattern, at least one valid key
    per item; None = all valid.  -> [B, H*dk, T].  dk = 64 or 96.  Under the "f32" precision the same formula runs as RoPE in torch plus
    ``scaled_dot_product_attention`` (not the hot path).  ``causal=True``: key j is visible to query i iff j <= i and the mask admits it
    (``amp_rope_attention_causal``, the prefill of the autoregressive transformer)."""
    for t, name in ((q, "q"), (k, "k"), (v, "v"), (cos, "cos"), (sin, "sin")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise TypeError(f"rope_attention: {name} must be a float32 tensor on a ROCm device (the HIP path has no CPU fallback)")
    if q.dim() != 3 or q.shape != k.shape or q.shape != v.shape or k.device != q.device or v.device != q.device:
        raise ValueError(f"rope_attention: q, k, v must be [B, H*dk, T] tensors of one shape on one device, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    B, C, T = q.shape
    H, dk = _heads("rope_attention", C, n_heads, (64, 96))
    if B < 1 or T < 1:
        raise ValueError(f"rope_attention: empty input {tuple(q.shape)}")
    if tuple(cos.shape) != (T, dk // 2) or tuple(sin.shape) != (T, dk // 2) or cos.device != q.device or sin.device != q.device:
        raise ValueError(f"rope_attention: cos and sin must be {(T, dk // 2)} on {q.device}, got {tuple(cos.shape)} and {tuple(sin.shape)}")
    cos, sin = cos.contiguous(), sin.contiguous()
    key_mask = _key_mask_u8("rope_attention", key_mask, B, T, q.device)
    scale = 1.0 / (dk ** 0.5) if scale is None else float(scale)
    with _lib.on_device(q.device):
        if _lib.get_precision() == "f32":
            def rope(x):                                     # -> [B, H, T, dk], contiguous
                x = x.reshape(B, H, dk, T).transpose(2, 3)
                c, s = torch.cat((cos, cos), -1), torch.cat((sin, sin), -1)
                return x * c + torch.cat((-x[..., dk // 2:], x[..., : dk // 2]), -1) * s
            m = None if key_mask is None else key_mask.bool()[:, None, None, :]
            if causal:
                tri = torch.ones((T, T), dtype=torch.bool, device=q.device).tril()[None, None]
                m = tri if m is None else m & tri
            return _sdpa_cf(rope(q), rope(k), v, H, m, scale)
        (q, k, v), bstride = _row_blocks((q, k, v), C, T)
        out = torch.empty((B, C, T), dtype=torch.float32, device=q.device)
        entry = _lib.lib().amp_rope_attention_causal if causal else _lib.lib().amp_rope_attention
        _lib.check(entry(_ptr(q), _ptr(k), _ptr(v), int(bstride), _ptr(cos), _ptr(sin), _ptr(key_mask), B, H, dk, T, scale, _ptr(out), _stream(q)))
    return out


# ---- MaskGCT's decoding step (csrc/maskgct.hip) ----------------
def mask_sample(logits, k, u=None, temperature=1.0):
    """One decoding step's sampler (``amp_mask_sample``; maskgct_t2s.py: ``top_k``, ``gumbel_sample``, ``softmax().gather()``).

    logits [B, V, T] channel-first, the pointwise GEMM's output: contiguous, or a row block of a wider tensor (read in place through its
    batch stride).  k: how many of a frame's largest logits stay, ``ceil((1 - filter_thres) * V)``.  u [B, T, V] uniform noise in the
    reference's own shape, or None for the greedy step (``temperature`` is then ignored).
    -> (ids [B, T] int64, score [B, T]): the argmax over the kept entries of ``l / max(temperature, 1e-10) - log(-log(u + 1e-10) + 1e-10)``
    and the softmax of the filtered logits (temperature 1) at that id.  Ties go to the lower index.  2 <= V <= 8192."""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != torch.float32:
        raise TypeError("mask_sample: logits must be a float32 tensor on a ROCm device (the HIP path has no CPU fallback)")
    if logits.dim() != 3 or logits.numel() == 0:
        raise ValueError(f"mask_sample: expected non-empty [B, V, T] logits, got {tuple(logits.shape)}")
    B, V, T = logits.shape
    k = int(k)
    if not 2 <= V <= 8192 or not 1 <= k <= V:
        raise ValueError(f"mask_sample: V={V} (2..8192), k={k} (1..V)")
    (logits,), bstride = _row_blocks((logits,), V, T)
    if u is not None:
        if not isinstance(u, torch.Tensor) or u.device != logits.device or u.dtype != torch.float32 or tuple(u.shape) != (B, T, V):
            raise ValueError(f"mask_sample: u must be a float32 {(B, T, V)} tensor on {logits.device}")
        u = u.contiguous()
    ids = torch.empty((B, T), dtype=torch.int64, device=logits.device)
    score = torch.empty((B, T), dtype=torch.float32, device=logits.device)
    with _lib.on_device(logits.device):
        _lib.check(_lib.lib().amp_mask_sample(_ptr(logits), int(bstride), B, V, T, k, _ptr(u), float(temperature), _ptr(ids), _ptr(score),
                                              _stream(logits)))
    return ids, score


# ---- the autoregressive transformer's decode step (csrc/llama_ar.hip; the T = 1 Linear: csrc/pw_vec.hip) ----------------
def kv_cache(B, n_heads, dk, Lmax, device):
    """one layer's (K, V) cache, two fp32 [B, H*dk, Lmax] buffers (K holds rope(k))"""
    shape = (int(B), int(n_heads) * int(dk), int(Lmax))
    return torch.zeros(shape, dtype=torch.float32, device=device), torch.zeros(shape, dtype=torch.float32, device=device)


def kv_append(k, v, n_heads, cos, sin, pos0, kcache, vcache):
    """rope(k) and v of the T columns of k, v [B, H*dk, T] (contiguous, or row blocks of one stacked GEMM output) into columns
    [pos0, pos0 + T) of the caches [B, H*dk, Lmax] (``amp_kv_append``); cos, sin [>= pos0 + T, dk/2] are the tables from row 0"""
    for t, name in ((k, "k"), (v, "v"), (cos, "cos"), (sin, "sin"), (kcache, "kcache"), (vcache, "vcache")):
        _f32_dev(t, name, "kv_append")
    if k.dim() != 3 or k.shape != v.shape or k.numel() == 0:
        raise ValueError(f"kv_append: k and v must be non-empty [B, H*dk, T] tensors of one shape, got {tuple(k.shape)} and {tuple(v.shape)}")
    B, C, T = k.shape
    H = int(n_heads)
    if H < 1 or C % H or C // H not in (64, 96):
        raise ValueError(f"kv_append: {C} channels in {H} heads is not a head dimension of 64 or 96")
    dk, pos0 = C // H, int(pos0)
    if kcache.dim() != 3 or kcache.shape != vcache.shape or tuple(kcache.shape[:2]) != (B, C) or not kcache.is_contiguous() or not vcache.is_contiguous():
        raise ValueError(f"kv_append: the caches must be contiguous [{B}, {C}, Lmax] tensors, got {tuple(kcache.shape)} and {tuple(vcache.shape)}")
    Lmax = kcache.shape[2]
    if pos0 < 0 or pos0 + T > Lmax:
        raise ValueError(f"kv_append: columns [{pos0}, {pos0 + T}) do not fit a cache of {Lmax}")
    if cos.dim() != 2 or cos.shape != sin.shape or cos.shape[1] != dk // 2 or cos.shape[0] < pos0 + T:
        raise ValueError(f"kv_append: cos and sin must be [>= {pos0 + T}, {dk // 2}], got {tuple(cos.shape)} and {tuple(sin.shape)}")
    cos, sin = cos.contiguous(), sin.contiguous()
    (k, v), bstride = _row_blocks((k, v), C, T)
    with _lib.on_device(k.device):
        _lib.check(_lib.lib().amp_kv_append(_ptr(k), _ptr(v), int(bstride), _ptr(cos), _ptr(sin), B, H, dk, T, pos0, Lmax, _ptr(kcache), _ptr(vcache),
                                            _stream(k)))


_decode_ws = {}     # (device, bytes) -> workspace


def _workspace(device, nbytes):
    key = (str(device), int(nbytes))
    t = _decode_ws.get(key)
    if t is None:
        if len(_decode_ws) >= 64:
            _decode_ws.clear()
        t = _decode_ws[key] = torch.empty(max(1, (int(nbytes) + 3) // 4), dtype=torch.float32, device=device)
    return t


def attention_decode(q, n_heads, cos, sin, L, kcache, vcache, scale=None):
    """One decode step's attention (``amp_attention_decode``): q [B, H*dk] or [B, H*dk, 1], un-rotated (a row block of the stacked GEMM
    output is read in place), at position L - 1 over cache columns [0, L) -> [B, H*dk, 1].  cos, sin [>= L, dk/2] from row 0."""
    for t, name in ((q, "q"), (cos, "cos"), (sin, "sin"), (kcache, "kcache"), (vcache, "vcache")):
        _f32_dev(t, name, "attention_decode")
    if q.dim() == 3 and q.shape[2] == 1:
        q = q[:, :, 0]
    if q.dim() != 2 or q.numel() == 0:
        raise ValueError(f"attention_decode: q must be [B, H*dk] or [B, H*dk, 1], got {tuple(q.shape)}")
    B, C = q.shape
    H, L = int(n_heads), int(L)
    if H < 1 or C % H or C // H not in (64, 96):
        raise ValueError(f"attention_decode: {C} channels in {H} heads is not a head dimension of 64 or 96")
    dk = C // H
    if kcache.dim() != 3 or kcache.shape != vcache.shape or tuple(kcache.shape[:2]) != (B, C) or not kcache.is_contiguous() or not vcache.is_contiguous():
        raise ValueError(f"attention_decode: the caches must be contiguous [{B}, {C}, Lmax] tensors, got {tuple(kcache.shape)} and {tuple(vcache.shape)}")
    Lmax = kcache.shape[2]
    if not 1 <= L <= Lmax:
        raise ValueError(f"attention_decode: L={L} is outside [1, {Lmax}]")
    if cos.dim() != 2 or cos.shape != sin.shape or cos.shape[1] != dk // 2 or cos.shape[0] < L:
        raise ValueError(f"attention_decode: cos and sin must be [>= {L}, {dk // 2}], got {tuple(cos.shape)} and {tuple(sin.shape)}")
    cos, sin = cos.contiguous(), sin.contiguous()
    q, qbs = _rows_2d(q, C)
    scale = 1.0 / (dk ** 0.5) if scale is None else float(scale)
    out = torch.empty((B, C, 1), dtype=torch.float32, device=q.device)
    with _lib.on_device(q.device):
        L_ = _lib.lib()
        nbytes = L_.amp_attention_decode_workspace_bytes(B, H, dk, Lmax)
        ws = _workspace(q.device, nbytes)
        _lib.check(L_.amp_attention_decode(_ptr(q), qbs, _ptr(cos), _ptr(sin), _ptr(kcache), _ptr(vcache), B, H, dk, L, Lmax, scale, _ptr(out),
                                           _ptr(ws), nbytes, _stream(q)))
    return out


def pw_forward_vec(h, cout, x, gamma=None, res=None, out=None):
    """``amp_pw_forward_vec``: the Linear of the ``amp_pw`` handle ``h`` on x [B, cin, 1] (B <= 8; contiguous, or a row block of a wider
    [B, C, 1] tensor) -> [B, cout, 1]; with ``res`` (and ``gamma`` [cout]) the ``res + gamma * (Wx + b)`` epilogue"""
    x, B, cin, xbs = _vec_input("pw_forward_vec", x)
    if out is None:
        out = torch.empty((B, int(cout), 1), dtype=torch.float32, device=x.device)
    epi = 0 if res is None else 2
    with _lib.on_device(x.device):
        L_ = _lib.lib()
        nbytes = L_.amp_pw_forward_vec_workspace_bytes(h, B)
        ws = _workspace(x.device, nbytes)
        _lib.check(L_.amp_pw_forward_vec(h, _ptr(x), xbs, B, epi, _ptr(gamma), _ptr(res), _ptr(out), _ptr(ws), nbytes, _stream(x)))
    return out


def ar_sample(logits, q, ids, n_ids, eos_id, suppress_eos, temperature=1.0, top_k=50, top_p=1.0, repetition_penalty=1.0):
    """One decode step's sampler (``amp_ar_sample``): HF's repetition penalty -> EOS suppression -> temperature -> top-k -> top-p chain on
    logits [B, V] / [B, V, 1] and the race ``argmax p / q`` against the Exp(1) noise q [B, V].  ids [B, capacity] int64 holds the ids so
    far in columns [0, n_ids) (the penalty's history); the drawn id is written to column n_ids.  Returns ``ids``."""
    _f32_dev(logits, "logits", "ar_sample")
    _f32_dev(q, "q", "ar_sample")
    if logits.dim() == 3 and logits.shape[2] == 1:
        logits = logits[:, :, 0]
    if logits.dim() != 2 or logits.numel() == 0:
        raise ValueError(f"ar_sample: logits must be [B, V] or [B, V, 1], got {tuple(logits.shape)}")
    B, V = logits.shape
    logits, lbs = _rows_2d(logits, V)
    if tuple(q.shape) != (B, V) or q.device != logits.device:
        raise ValueError(f"ar_sample: q must be a {(B, V)} tensor on {logits.device}, got {tuple(q.shape)}")
    q = q.contiguous()
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.device != logits.device or ids.dim() != 2 or ids.shape[0] != B \
            or not ids.is_contiguous():
        raise ValueError(f"ar_sample: ids must be a contiguous int64 [{B}, capacity] tensor on {logits.device}")
    with _lib.on_device(logits.device):
        _lib.check(_lib.lib().amp_ar_sample(_ptr(logits), lbs, B, V, _ptr(q), _ptr(ids), ids.shape[1], int(n_ids),
                                            int(eos_id), 1 if suppress_eos else 0, float(temperature), int(top_k), float(top_p),
                                            float(repetition_penalty), _stream(logits)))
    return ids


# ---- FastSpeech2 / JETS inference (csrc/fastspeech.hip; the attention is llama_nar.hip's kernel without rotation) ----------------
def mh_attention(q, k, v, n_heads, key_mask=None, scale=None):
    """``ScaledDotProductAttention`` inside the FFT block's ``MultiHeadAttention`` (``amp_mh_attention``): non-causal, no positional rotation.

    q, k, v [B, H*dk, T] channel-first: contiguous tensors, or the three row blocks of one stacked [B, 3*H*dk, T] GEMM output (read in
    place: no copy).  key_mask [B, T] bool / uint8, 1 = VALID (the reference's mask is 1 = padded: pass its negation), any pattern, at least
    one valid key per item; None = all valid.  scale = 1 / temperature, default 1 / sqrt(dk).  -> [B, H*dk, T].  dk = 128.  Under the "f32"
    precision the same formula runs as ``scaled_dot_product_attention`` in torch (not the hot path)."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        _f32_dev(t, name, "mh_attention")
    if q.dim() != 3 or q.shape != k.shape or q.shape != v.shape or k.device != q.device or v.device != q.device:
        raise ValueError(f"mh_attention: q, k, v must be [B, H*dk, T] tensors of one shape on one device, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    B, C, T = q.shape
    H, dk = _heads("mh_attention", C, n_heads, (128,))
    if B < 1 or T < 1:
        raise ValueError(f"mh_attention: empty input {tuple(q.shape)}")
    key_mask = _key_mask_u8("mh_attention", key_mask, B, T, q.device)
    scale = 1.0 / (dk ** 0.5) if scale is None else float(scale)
    with _lib.on_device(q.device):
        if _lib.get_precision() == "f32":
            return _sdpa_cf(q, k, v, H, None if key_mask is None else key_mask.bool()[:, None, None, :], scale)
        (q, k, v), bstride = _row_blocks((q, k, v), C, T)
        out = torch.empty((B, C, T), dtype=torch.float32, device=q.device)
        _lib.check(_lib.lib().amp_mh_attention(_ptr(q), _ptr(k), _ptr(v), int(bstride), _ptr(key_mask), B, H, dk, T, scale, _ptr(out), _stream(q)))
    return out


def fs2_durations(log_d, d_control=1.0):
    """log_d [B, T] -> (d_rounded [B, T] fp32 = ``clamp(round(exp(log_d) - 1) * d_control, min=0)``, cum [B, T] int32, the running sum of
    ``int(d_rounded)`` in the layout ``expand_path`` takes, mel_len [B] int32) (``amp_fs2_durations``)"""
    log_d = _lib.require_device_tensor(log_d, "fs2_durations input")
    if log_d.dim() != 2 or log_d.numel() == 0:
        raise ValueError(f"fs2_durations: expected a non-empty [B, T] input, got {tuple(log_d.shape)}")
    B, T = log_d.shape
    d = torch.empty_like(log_d)
    cum = torch.empty((B, T), dtype=torch.int32, device=log_d.device)
    mel_len = torch.empty((B,), dtype=torch.int32, device=log_d.device)
    with _lib.on_device(log_d.device):
        _lib.check(_lib.lib().amp_fs2_durations(_ptr(log_d), B, T, float(d_control), _ptr(d), _ptr(cum), _ptr(mel_len), _stream(log_d)))
    return d, cum, mel_len


def bucketize_embed_add(x, pred, control, bins, table, out=None):
    """``x + embedding(bucketize(pred * control, bins))`` at every column, bit for bit torch's (``amp_bucketize_embed_add``): x [B, D, T]
    channel-first, pred [B, T], bins [n_bins - 1] ascending, table [n_bins, D].  ``out`` may be ``x``.  -> (y [B, D, T], pred * control)"""
    x = _lib.require_device_tensor(x, "bucketize_embed_add input")
    pred = _lib.require_device_tensor(pred, "bucketize_embed_add prediction")
    bins = _lib.require_device_tensor(bins.detach(), "bucketize_embed_add boundaries")
    table = _lib.require_device_tensor(table.detach(), "bucketize_embed_add table")
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError(f"bucketize_embed_add: expected a non-empty [B, D, T] input, got {tuple(x.shape)}")
    B, D, T = x.shape
    if tuple(pred.shape) != (B, T) or bins.dim() != 1 or table.dim() != 2 or table.shape[1] != D or table.shape[0] < bins.shape[0] + 1 or bins.shape[0] < 1:
        raise ValueError(f"bucketize_embed_add: expected pred {(B, T)}, n boundaries and a table [>= n + 1, {D}], got {tuple(pred.shape)}, "
                         f"{tuple(bins.shape)}, {tuple(table.shape)}")
    if any(t.device != x.device for t in (pred, bins, table)):
        raise ValueError(f"bucketize_embed_add: every tensor must be on {x.device}")
    out = _out_like("bucketize_embed_add", out, x)
    scaled = torch.empty_like(pred)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().amp_bucketize_embed_add(_ptr(pred), float(control), _ptr(bins), bins.shape[0], _ptr(table), table.shape[0], _ptr(x), B, D,
                                                      T, _ptr(out), _ptr(scaled), _stream(x)))
    return out, scaled


def layer_norm_c_head(x, gamma, beta, w, b0, lens=None, eps=1e-5):
    """``Linear(C, 1)(LN_c(x))`` as [B, T], 0 where ``t >= lens[b]`` (``amp_layer_norm_c_head``): x [B, C, T], gamma / beta / w [C], b0 a float"""
    x = _lib.require_device_tensor(x, "layer_norm_c_head input")
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError(f"layer_norm_c_head: expected a non-empty [B, C, T] input, got {tuple(x.shape)}")
    B, C, T = x.shape
    gamma, beta, w = (_lib.require_device_tensor(t.detach().reshape(-1), n) for t, n in ((gamma, "gamma"), (beta, "beta"), (w, "head weight")))
    if any(t.numel() != C or t.device != x.device for t in (gamma, beta, w)):
        raise ValueError(f"layer_norm_c_head: gamma, beta and w must hold {C} values on {x.device}")
    if lens is not None and (lens.dtype != torch.int32 or tuple(lens.shape) != (B,) or lens.device != x.device):
        raise ValueError(f"layer_norm_c_head: lens must be an int32 [{B}] tensor on {x.device}")
    y = torch.empty((B, T), dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().amp_layer_norm_c_head(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(w), float(b0), _ptr(lens), B, C, T, float(eps), _ptr(y),
                                                    _stream(x)))
    return y


# ---- NaturalSpeech2 inference (csrc/llama_nar.hip: amp_cross_attention; csrc/ns2_layer_f16x3.hip; csrc/ns2.hip) ----------------
def cross_attention(q, k, v, n_heads, key_mask=None, scale=None):
    """Non-causal multi-head attention without rotation at head dimension 64, query and key lengths apart (``amp_cross_attention``).

    q [B, H*dk, Tq]; k, v [B, H*dk, Tk] of one shape and ONE batch stride: contiguous tensors, or row blocks of stacked GEMM outputs read in
    place (k | v of one tensor; for self-attention q | k | v of one tensor).  key_mask [B, Tk] bool / uint8, 1 = VALID, any pattern, at least
    one valid key per item; None = all valid.  scale defaults to 1 / sqrt(dk).  -> [B, H*dk, Tq].  Under the "f32" precision the same formula
    runs as ``scaled_dot_product_attention`` in torch (not the hot path)."""
    return _cross_attention("amp_cross_attention", (64,), q, k, v, n_heads, key_mask, scale)


def _cross_attention(entry, dks, q, k, v, n_heads, key_mask, scale):
    """``cross_attention`` through the C entry ``entry``, which covers the head dimensions ``dks``"""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        _f32_dev(t, name, "cross_attention")
    if q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or q.shape[:2] != k.shape[:2] or k.device != q.device or v.device != q.device:
        raise ValueError(f"cross_attention: q must be [B, H*dk, Tq] and k, v [B, H*dk, Tk] on one device, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    B, C, Tq = q.shape
    Tk = k.shape[2]
    H, dk = _heads("cross_attention", C, n_heads, dks)
    if B < 1 or Tq < 1 or Tk < 1:
        raise ValueError(f"cross_attention: empty input {tuple(q.shape)}, {tuple(k.shape)}")
    key_mask = _key_mask_u8("cross_attention", key_mask, B, Tk, q.device)
    scale = 1.0 / (dk ** 0.5) if scale is None else float(scale)
    with _lib.on_device(q.device):
        if _lib.get_precision() == "f32":
            return _sdpa_cf(q, k, v, H, None if key_mask is None else key_mask.bool()[:, None, None, :], scale)
        (q,), qbs = _row_blocks((q,), C, Tq)
        (k, v), kvbs = _row_blocks((k, v), C, Tk)
        out = torch.empty((B, C, Tq), dtype=torch.float32, device=q.device)
        _lib.check(getattr(_lib.lib(), entry)(_ptr(q), int(qbs), _ptr(k), _ptr(v), int(kvbs), _ptr(key_mask), B, H, dk, Tq, Tk, scale, _ptr(out),
                                                  _stream(q)))
    return out


class Ns2Layer:
    """One residual layer of NaturalSpeech2's WaveNet (``amp_ns2_layer_*``; wavenet.py:96-127 with ``x_mask = None``) over the parameters of
    the reference's ``ResidualBlock``: ``dilated_conv`` (weight [2H, H, 3], bias) and ``out_proj`` (weight [2H, H, 1], bias).  The packed
    device copy is rebuilt when a parameter, the device or the precision changes."""

    def __init__(self, hidden, dilation):
        self.hidden, self.dilation = int(hidden), int(dilation)
        self._cache = HandleCache("amp_ns2_layer_destroy")

    def _build(self, conv_w, conv_b, out_w, out_b, device):
        H = self.hidden
        cw, cb, ow, ob = host_f32(conv_w), host_f32(conv_b), host_f32(out_w), host_f32(out_b)
        if tuple(cw.shape) != (2 * H, H, 3) or ow.numel() != 2 * H * H or (cb is not None and cb.numel() != 2 * H) or (ob is not None and ob.numel() != 2 * H):
            raise ValueError(f"Ns2Layer: expected dilated_conv.weight {(2 * H, H, 3)} and out_proj.weight {(2 * H, H, 1)}, got {tuple(cw.shape)} and "
                             f"{tuple(ow.shape)}")
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_ns2_layer_create(H, self.dilation, _ptr(cw), _ptr(cb), _ptr(ow), _ptr(ob), ctypes.byref(h)))
        return h

    def handle(self, conv_w, conv_b, out_w, out_b, device):
        """the ``amp_ns2_layer`` handle for these parameters on ``device`` under the current precision (built on first use, rebuilt when one of
        them changes).  A caller that runs the layer many times on buffers of its own (``WaveNet.step``) takes the handle once and calls
        ``amp_ns2_layer_forward`` itself; ``__call__`` is the checked form."""
        sig = param_sig((conv_w, conv_b, out_w, out_b), device, _lib.get_precision())
        c = self._cache
        return c.handle if sig == c.sig else c.build(sig, self._build, conv_w, conv_b, out_w, out_b, device)

    def __call__(self, x, dconst, cterm, conv_w, conv_b, out_w, out_b, film=None, skip=None, x_out=None):
        """x [B, H, T]; dconst [H] or [B, H] (rows may be a slice of a wider tensor); cterm [B, 2H, T], contiguous or a row block of a wider
        [B, n, T] tensor; film [B, 4H, T] (gain | bias) or None; skip [B, H, T]: the running skip sum, updated IN PLACE, or None in the first
        layer (a new tensor is returned).  x_out: where the layer's output goes (may be ``x``), default a new tensor.  -> (x_out, skip)"""
        x = _lib.require_device_tensor(x, "ns2 layer input")
        if x.dim() != 3 or x.shape[1] != self.hidden or x.numel() == 0:
            raise ValueError(f"Ns2Layer: expected a non-empty [B, {self.hidden}, T] input, got {tuple(x.shape)}")
        B, H, T = x.shape
        dev = x.device
        _f32_dev(dconst, "dconst", "Ns2Layer")
        _f32_dev(cterm, "cterm", "Ns2Layer")
        if dconst.dim() == 1:
            dconst = dconst[None]
        if dconst.dim() != 2 or dconst.shape[1] != H or dconst.shape[0] not in (1, B) or dconst.device != dev:
            raise ValueError(f"Ns2Layer: dconst must be [{H}] or [{B}, {H}] on {dev}, got {tuple(dconst.shape)}")
        dconst, dbs = _rows_2d(dconst, H)
        if dconst.shape[0] == 1:
            dbs = 0                                          # one row for every item
        if tuple(cterm.shape) != (B, 2 * H, T) or cterm.device != dev:
            raise ValueError(f"Ns2Layer: cterm must be {(B, 2 * H, T)} on {dev}, got {tuple(cterm.shape)}")
        (cterm,), cbs = _row_blocks((cterm,), 2 * H, T)
        if film is not None:
            film = _lib.require_device_tensor(film, "ns2 layer FiLM")
            if tuple(film.shape) != (B, 4 * H, T) or film.device != dev:
                raise ValueError(f"Ns2Layer: film must be {(B, 4 * H, T)} on {dev}, got {tuple(film.shape)}")
        for t, name in ((skip, "skip"), (x_out, "x_out")):
            if t is not None and (not isinstance(t, torch.Tensor) or t.shape != x.shape or t.device != dev or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f"Ns2Layer: {name} must be a contiguous float32 {tuple(x.shape)} on {dev}")
        skip_out = torch.empty_like(x) if skip is None else skip
        x_out = torch.empty_like(x) if x_out is None else x_out
        h = self.handle(conv_w, conv_b, out_w, out_b, dev)
        L = _lib.lib()
        with _lib.on_device(dev):
            nbytes = L.amp_ns2_layer_workspace_bytes(h, B, T)
            ws = _workspace(dev, nbytes)
            _lib.check(L.amp_ns2_layer_forward(h, _ptr(x), _ptr(dconst), dbs, _ptr(cterm), int(cbs), _ptr(film), _ptr(skip), B, T, _ptr(x_out),
                                               _ptr(skip_out), _ptr(ws), nbytes, _stream(x)))
        return x_out, skip_out


def ns2_ode_step(x_eval, x0_pred, x_base, mean_scale, variance, h_beta, inv_sigma2, midpoint_half=False, out=None):
    """The element-wise tail of ``Diffusion.cal_dxt`` and the solver's update in one launch (``amp_ns2_ode_step``):
    ``x_base - dxt(x_eval, x0_pred)``, or ``0.5 * ((x_base - dxt) + x_base)`` with ``midpoint_half`` (the midpoint solver's ``x_mid``).
    The four scalars are Python floats holding fp32 values.  ``out`` may be any of the inputs; default a new tensor."""
    ts = [_lib.require_device_tensor(t, n) for t, n in ((x_eval, "ns2_ode_step x_eval"), (x0_pred, "ns2_ode_step x0_pred"), (x_base, "ns2_ode_step x_base"))]
    if ts[0].numel() == 0 or ts[1].shape != ts[0].shape or ts[2].shape != ts[0].shape or ts[1].device != ts[0].device or ts[2].device != ts[0].device:
        raise ValueError(f"ns2_ode_step: three non-empty tensors of one shape on one device, got {[tuple(t.shape) for t in ts]}")
    out = _out_like("ns2_ode_step", out, ts[0])
    with _lib.on_device(out.device):
        _lib.check(_lib.lib().amp_ns2_ode_step(_ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), ts[0].numel(), float(mean_scale), float(variance), float(h_beta),
                                               float(inv_sigma2), 1 if midpoint_half else 0, _ptr(out), _stream(out)))
    return out


# ---- VALL-E inference (csrc/valle.hip; the prefill attention is llama_nar.hip's causal kernel without rotation) ----------------
def prefix_attention(q, k, v, n_heads, prefix, key_mask=None, scale=None):
    """Self-attention without rotation at head dimension 64 under the prefix-LM rule (``amp_prefix_attention``): key j is visible to query i
    iff ``j < prefix or j <= i`` and the key mask admits it.

    q, k, v [B, H*dk, T] channel-first: contiguous tensors, or the three row blocks of one stacked [B, 3*H*dk, T] GEMM output (read in
    place).  0 <= prefix <= T (0: causal, T: full attention).  key_mask [B, T] bool / uint8, 1 = VALID; None = all valid.  scale defaults to
    1 / sqrt(dk).  -> [B, H*dk, T].  Under the "f32" precision the same formula runs as ``scaled_dot_product_attention`` in torch (not the hot path)."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        _f32_dev(t, name, "prefix_attention")
    if q.dim() != 3 or q.shape != k.shape or q.shape != v.shape or k.device != q.device or v.device != q.device:
        raise ValueError(f"prefix_attention: q, k, v must be [B, H*dk, T] tensors of one shape on one device, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    B, C, T = q.shape
    (H, dk), prefix = _heads("prefix_attention", C, n_heads, (64,)), int(prefix)
    if B < 1 or T < 1:
        raise ValueError(f"prefix_attention: empty input {tuple(q.shape)}")
    if not 0 <= prefix <= T:
        raise ValueError(f"prefix_attention: prefix={prefix} is outside [0, {T}]")
    key_mask = _key_mask_u8("prefix_attention", key_mask, B, T, q.device)
    scale = 1.0 / (dk ** 0.5) if scale is None else float(scale)
    with _lib.on_device(q.device):
        if _lib.get_precision() == "f32":
            j = torch.arange(T, device=q.device)
            m = ((j[None, :] < prefix) | (j[None, :] <= j[:, None]))[None, None]
            if key_mask is not None:
                m = m & key_mask.bool()[:, None, None, :]
            return _sdpa_cf(q, k, v, H, m, scale)
        (q, k, v), bstride = _row_blocks((q, k, v), C, T)
        out = torch.empty((B, C, T), dtype=torch.float32, device=q.device)
        _lib.check(_lib.lib().amp_prefix_attention(_ptr(q), _ptr(k), _ptr(v), int(bstride), _ptr(key_mask), B, H, dk, T, prefix, scale, _ptr(out),
                                                   _stream(q)))
    return out


def pw_forward_vec_ln(h, cout, x, ln_gamma=None, ln_beta=None, eps=1e-5, relu=False, gamma=None, res=None, out=None):
    """``amp_pw_forward_vec_ln``: ``epi(W n(x) + b)`` of the ``amp_pw`` handle ``h`` on x [B, cin, 1] (B <= 8; contiguous, or a row block of a
    wider [B, C, 1] tensor) -> [B, cout, 1].  n = LayerNorm over the cin channels with ``ln_gamma`` / ``ln_beta`` [cin] (both None: n(x) = x);
    epi = bias, bias -> ReLU (``relu``), or ``res + gamma * (.)`` (``res`` and ``gamma`` [cout]; not with ``relu``)."""
    x, B, cin, xbs = _vec_input("pw_forward_vec_ln", x)
    if (ln_gamma is None) != (ln_beta is None):
        raise ValueError("pw_forward_vec_ln: ln_gamma and ln_beta come together")
    for t, name in ((ln_gamma, "ln_gamma"), (ln_beta, "ln_beta")):
        if t is not None and (_f32_dev(t, name, "pw_forward_vec_ln").numel() != cin or t.device != x.device or not t.is_contiguous()):
            raise ValueError(f"pw_forward_vec_ln: {name} must hold {cin} contiguous values on {x.device}")
    if (res is None) != (gamma is None) or (res is not None and relu):
        raise ValueError("pw_forward_vec_ln: the residual epilogue takes res and gamma, and no relu")
    if out is None:
        out = torch.empty((B, int(cout), 1), dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        L_ = _lib.lib()
        nbytes = L_.amp_pw_forward_vec_ln_workspace_bytes(h, B)
        ws = _workspace(x.device, nbytes)
        _lib.check(L_.amp_pw_forward_vec_ln(h, _ptr(x), xbs, B, _ptr(ln_gamma), _ptr(ln_beta), float(eps), 1 if relu else 0, _ptr(gamma), _ptr(res),
                                            _ptr(out), _ptr(ws), nbytes, _stream(x)))
    return out


def embed_pos(tokens, weight, pe, pos0, alpha, x_scale=1.0, check=True):
    """``amp_embed_pos``: ``weight[tokens] * x_scale + alpha * pe[pos0 : pos0 + T]`` channel-first.  tokens int64 [B, T]; weight [rows, D];
    pe [pe_rows, D]; alpha a one-element fp32 tensor on the device.  -> y [B, D, T].  An id outside [0, rows) raises ``AmpError``
    (AMP_ERR_INVALID) -- here, or with ``check=False`` at the caller's ``embed_sum_check`` (the check synchronises; a decode loop runs it
    once behind its steps)."""
    weight, pe, alpha = (_f32_dev(t.detach(), n, "embed_pos") for t, n in ((weight, "weight"), (pe, "pe"), (alpha, "alpha")))
    if not isinstance(tokens, torch.Tensor) or tokens.dtype != torch.int64 or tokens.dim() != 2 or tokens.numel() == 0 or tokens.device != weight.device:
        raise ValueError(f"embed_pos: tokens must be a non-empty int64 [B, T] tensor on {weight.device}")
    if weight.dim() != 2 or pe.dim() != 2 or pe.shape[1] != weight.shape[1] or alpha.numel() != 1 or pe.device != weight.device or alpha.device != weight.device:
        raise ValueError(f"embed_pos: weight [rows, D], pe [pe_rows, D] and a one-element alpha on one device, got {tuple(weight.shape)}, {tuple(pe.shape)}, "
                         f"{tuple(alpha.shape)}")
    B, T = tokens.shape
    rows, D = weight.shape
    pos0 = int(pos0)
    if pos0 < 0 or pos0 + T > pe.shape[0]:
        raise ValueError(f"embed_pos: positions [{pos0}, {pos0 + T}) are beyond a table of {pe.shape[0]} rows")
    tokens, weight, pe = tokens.contiguous(), weight.contiguous(), pe.contiguous()
    flag = _embed_sum_flag(weight.device)
    y = torch.empty((B, D, T), dtype=torch.float32, device=weight.device)
    with _lib.on_device(weight.device):
        _lib.check(_lib.lib().amp_embed_pos(_ptr(tokens), _ptr(weight), rows, D, _ptr(pe), pe.shape[0], pos0, float(x_scale), _ptr(alpha), B, T, _ptr(y),
                                            _ptr(flag), _stream(y)))
        if check:
            _lib.check(_lib.lib().amp_embed_sum_check(_ptr(flag), _stream(y)))
    return y


# ---- AudioLDM text-to-audio (csrc/conv2d_f16x3.hip, csrc/tta.hip; csrc/llama_nar.hip: amp_cross_attention at dk 32 / 64 / 128) ----------------
def group_norm_stats(x, eps):
    """GroupNorm(32) statistics of x [B, C, *] -> mean | rstd [B, 32, 2] (``amp_group_norm_stats``); C a multiple of 32"""
    x = _lib.require_device_tensor(x, "group_norm_stats input")
    if x.dim() < 3 or x.numel() == 0:
        raise ValueError(f"group_norm_stats: expected a non-empty [B, C, ...] input, got {tuple(x.shape)}")
    B, C = x.shape[:2]
    mr = torch.empty((B, 32, 2), dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().amp_group_norm_stats(_ptr(x), B, C, x.numel() // (B * C), float(eps), _ptr(mr), _stream(x)))
    return mr


def group_norm(x, gamma, beta, eps, silu=False, stats=None):
    """GroupNorm(32) of x [B, C, *] with an optional SiLU (``amp_group_norm_stats`` + ``amp_group_norm``); ``stats`` [B, 32, 2] if the caller
    has them already"""
    x = _lib.require_device_tensor(x, "group_norm input")
    B, C = x.shape[:2]
    _f32_dev(gamma, "gamma", "group_norm")
    _f32_dev(beta, "beta", "group_norm")
    if gamma.numel() != C or beta.numel() != C or gamma.device != x.device or beta.device != x.device:
        raise ValueError(f"group_norm: gamma and beta must hold {C} values on {x.device}")
    mr = group_norm_stats(x, eps) if stats is None else stats
    y = torch.empty_like(x)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().amp_group_norm(_ptr(x), _ptr(mr), _ptr(gamma.contiguous()), _ptr(beta.contiguous()), B, C, x.numel() // (B * C), int(bool(silu)),
                                             _ptr(y), _stream(x)))
    return y


def geglu(u):
    """u [B, 2F, T], the output of one stacked value | gate GEMM -> u[:, :F] * gelu(u[:, F:]) [B, F, T] (``amp_geglu``)"""
    u = _lib.require_device_tensor(u, "geglu input")
    if u.dim() != 3 or u.numel() == 0 or u.shape[1] % 2:
        raise ValueError(f"geglu: expected a non-empty [B, 2F, T] input, got {tuple(u.shape)}")
    B, F2, T = u.shape
    y = torch.empty((B, F2 // 2, T), dtype=torch.float32, device=u.device)
    with _lib.on_device(u.device):
        _lib.check(_lib.lib().amp_geglu(_ptr(u), B, F2 // 2, T, _ptr(y), _stream(u)))
    return y


def cross_attention_hd(q, k, v, n_heads, key_mask=None, scale=None):
    """``cross_attention`` at head dimension 32, 64 or 128 (``amp_cross_attention_hd``): the spatial transformer of AudioLDM"""
    return _cross_attention("amp_cross_attention_hd", (32, 64, 128), q, k, v, n_heads, key_mask, scale)


def conv2d_out_size(H, W, stride=1, up2=False):
    return (2 * H, 2 * W) if up2 else ((H - 1) // stride + 1, (W - 1) // stride + 1)


class Conv2d3x3:
    """A 3 x 3 ``nn.Conv2d`` with padding 1 on the HIP path (``amp_conv2d_*``) over the parameters of the reference's module: weight
    [Cout, Cin, 3, 3] and bias.  The packed device copy is rebuilt when a parameter, the device or the precision changes.  Under the "f32"
    precision the same function runs as torch ops on the same device (not the hot path)."""

    def __init__(self):
        self._cache = HandleCache("amp_conv2d_destroy")

    def _build(self, weight, bias, device):
        w, b = host_f32(weight), host_f32(bias)
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or (b is not None and b.numel() != w.shape[0]):
            raise ValueError(f"Conv2d3x3: expected a weight [Cout, Cin, 3, 3] and a bias [Cout], got {tuple(w.shape)}")
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_conv2d_create(w.shape[1], w.shape[0], _ptr(w), _ptr(b), ctypes.byref(h)))
        return h

    def handle(self, weight, bias, device):
        sig = param_sig((weight, bias), str(device), _lib.get_precision())
        c = self._cache
        return c.handle if sig == c.sig else c.build(sig, self._build, weight, bias, device)

    def plan(self, weight, bias, device, H, W, stride=1, up2=False):
        """(K slices, row blocks a wave owns, channels of a K chunk) of this conv on an H x W map (``amp_conv2d_plan``): 1 slice is the single
        launch with the epilogue on the accumulators.  A function of the conv and the map alone, never of the batch."""
        ks, mi, kc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.lib().amp_conv2d_plan(self.handle(weight, bias, device), int(H), int(W), int(stride), int(bool(up2)), ctypes.byref(ks), ctypes.byref(mi),
                                              ctypes.byref(kc)))
        return ks.value, mi.value, kc.value

    def __call__(self, x, weight, bias, stride=1, up2=False, norm=None, row_add=None, residual=None):
        """x [B, Cin, H, W] -> [B, Cout, Ho, Wo].  norm = (mean_rstd [B, 32, 2], gamma [Cin], beta [Cin]): GroupNorm(32) + SiLU on load;
        row_add [B, Cout] (or [B, Cout, 1, 1]; a column block of a wider [B, n] tensor is read in place); residual [B, Cout, Ho, Wo]."""
        x = _lib.require_device_tensor(x, "conv2d input")
        if x.dim() != 4 or x.numel() == 0 or x.shape[1] != weight.shape[1]:
            raise ValueError(f"Conv2d3x3: expected a non-empty [B, {weight.shape[1]}, H, W] input, got {tuple(x.shape)}")
        B, Cin, H, W = x.shape
        Cout = weight.shape[0]
        dev = x.device
        stride, up2 = int(stride), bool(up2)
        if stride not in (1, 2) or (up2 and stride != 1):
            raise ValueError(f"Conv2d3x3: stride={stride} up2={up2} is not covered")
        Ho, Wo = conv2d_out_size(H, W, stride, up2)
        rbs = 0                                              # the row stride of an absent row_add / of a single item
        if row_add is not None:
            _f32_dev(row_add, "row_add", "Conv2d3x3")
            if row_add.dim() == 4 and tuple(row_add.shape[2:]) == (1, 1):
                row_add = row_add[:, :, 0, 0]
            if tuple(row_add.shape) != (B, Cout) or row_add.device != dev:
                raise ValueError(f"Conv2d3x3: row_add must be {(B, Cout)} on {dev}, got {tuple(row_add.shape)}")
            row_add, rbs = _rows_2d(row_add, Cout)
            if B == 1:
                rbs = 0
        if residual is not None:
            residual = _lib.require_device_tensor(residual, "conv2d residual")
            if tuple(residual.shape) != (B, Cout, Ho, Wo) or residual.device != dev:
                raise ValueError(f"Conv2d3x3: residual must be {(B, Cout, Ho, Wo)} on {dev}, got {tuple(residual.shape)}")
        if norm is not None:
            mr, gamma, beta = norm
            for t, name, shape in ((mr, "mean_rstd", (B, 32, 2)), (gamma, "gamma", (Cin,)), (beta, "beta", (Cin,))):
                _f32_dev(t, name, "Conv2d3x3")
                if tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                    raise ValueError(f"Conv2d3x3: {name} must be a contiguous {shape} tensor on {dev}, got {tuple(t.shape)}")
        if _lib.get_precision() == "f32":
            a = x
            if norm is not None:
                g = Cin // 32
                a = (x.reshape(B, 32, g, H * W) - mr[:, :, 0, None, None]) * mr[:, :, 1, None, None]
                a = torch.nn.functional.silu(a.reshape(B, Cin, H, W) * gamma.detach()[None, :, None, None] + beta.detach()[None, :, None, None])
            if up2:
                a = torch.nn.functional.interpolate(a, scale_factor=2, mode="nearest")
            y = torch.nn.functional.conv2d(a, weight.detach(), None if bias is None else bias.detach(), stride=stride, padding=1)
            if row_add is not None:
                y = y + row_add[:, :, None, None]
            if residual is not None:
                y = y + residual
            return y
        h = self.handle(weight, bias, dev)
        y = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=dev)
        L = _lib.lib()
        with _lib.on_device(dev):
            nbytes = L.amp_conv2d_workspace_bytes(h, B, H, W, stride, int(up2))
            # the K slices' partial sums: a tensor of this call (the caching allocator hands the block back to later work of the same
            # stream only), so no conv leaves memory held behind it
            ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev) if nbytes else None
            mr, gamma, beta = norm if norm is not None else (None, None, None)
            _lib.check(L.amp_conv2d_forward(h, _ptr(x), B, H, W, stride, int(up2), _ptr(mr), _ptr(gamma), _ptr(beta), _ptr(row_add), rbs, _ptr(residual),
                                            _ptr(y), _ptr(ws), nbytes, _stream(x)))
        return y
