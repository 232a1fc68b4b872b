"""ctypes-level helpers for the GPU parity tests (call the C ABI with raw device pointers)."""
import ctypes

import torch

from amphion_amd import _lib


def conv_forward(w, b, x, *, transposed=False, stride=1, dilation=1, padding=0, slope_in=1.0, res=None,
                 slope_out=1.0, options=()):
    """Run amp_conv_* on cuda:0.  w/b are CPU tensors (folded weight), x a CPU tensor [B, Cin, T].
    options: (amp_conv_option, value) pairs for amp_conv_set_option, applied to the new handle before the forward."""
    L = _lib.lib()
    h = ctypes.c_void_p()
    w = w.contiguous().float()
    cin = w.shape[0] if transposed else w.shape[1]
    cout = w.shape[1] if transposed else w.shape[0]
    bptr = ctypes.c_void_p(b.contiguous().float().data_ptr()) if b is not None else None
    _lib.check(L.amp_conv_create(int(transposed), cin, cout, w.shape[2], stride, dilation, padding,
                                 ctypes.c_void_p(w.data_ptr()), bptr, ctypes.byref(h)))
    try:
        for option, value in options:
            _lib.check(L.amp_conv_set_option(h, int(option), int(value)))
        xd = x.contiguous().float().cuda()
        B, _, T = xd.shape
        Tout = L.amp_conv_out_len(h, T)
        # (T_out <= 0 is the library's to refuse: amp_conv_forward still gets a real pointer)
        y = torch.full((B, cout, Tout if Tout > 0 else 1), float("nan"), device="cuda")
        rd = res.contiguous().float().cuda() if res is not None else None
        _lib.check(L.amp_conv_forward(h, ctypes.c_void_p(xd.data_ptr()), B, T, slope_in,
                                      ctypes.c_void_p(rd.data_ptr()) if rd is not None else None, slope_out,
                                      ctypes.c_void_p(y.data_ptr()), _lib.current_stream_ptr(xd.device)))
        torch.cuda.synchronize()
        return y.cpu()
    finally:
        L.amp_conv_destroy(h)


def pair_forward(w1, b1, w2, b2, x, *, dilation, slope=0.1):
    """amp_pair_forward on cuda:0: y = x + c2(lrelu(c1(lrelu(x))))  (fused ResBlock1 pair)."""
    L = _lib.lib()
    C, _, k = w1.shape
    hs = []
    try:
        for w, b, d in ((w1, b1, dilation), (w2, b2, 1)):
            h = ctypes.c_void_p()
            w = w.contiguous().float()
            b = b.contiguous().float()
            _lib.check(L.amp_conv_create(0, C, C, k, 1, d, (k * d - d) // 2, ctypes.c_void_p(w.data_ptr()),
                                         ctypes.c_void_p(b.data_ptr()), ctypes.byref(h)))
            hs.append(h)
        xd = x.contiguous().float().cuda()
        B, _, T = xd.shape
        y = torch.full_like(xd, float("nan"))
        _lib.check(L.amp_pair_forward(hs[0], hs[1], ctypes.c_void_p(xd.data_ptr()), B, T, slope,
                                      ctypes.c_void_p(y.data_ptr()), _lib.current_stream_ptr(xd.device)))
        torch.cuda.synchronize()
        return y.cpu()
    finally:
        for h in hs:
            L.amp_conv_destroy(h)


def resblock_forward(ws1, bs1, ws2, bs2, x, *, dilations, slope=0.1, fused=True):
    """ResBlock1 on cuda:0 from per-pair weights: fused=True -> amp_resblock_forward (ONE launch, csrc/rb_f16x3.hip),
    fused=False -> len(dilations) x amp_pair_forward (the fused pairs)."""
    L = _lib.lib()
    C, _, k = ws1[0].shape
    n = len(dilations)
    h1, h2 = [], []
    try:
        for ws, bs, hs, ds in ((ws1, bs1, h1, dilations), (ws2, bs2, h2, [1] * n)):
            for w, b, d in zip(ws, bs, ds):
                h = ctypes.c_void_p()
                w, b = w.contiguous().float(), b.contiguous().float()
                _lib.check(L.amp_conv_create(0, C, C, k, 1, d, (k * d - d) // 2, ctypes.c_void_p(w.data_ptr()),
                                             ctypes.c_void_p(b.data_ptr()), ctypes.byref(h)))
                hs.append(h)
        xd = x.contiguous().float().cuda()
        B, _, T = xd.shape
        st = _lib.current_stream_ptr(xd.device)
        if fused:
            y = torch.full_like(xd, float("nan"))
            a1, a2 = (ctypes.c_void_p * n)(*[h.value for h in h1]), (ctypes.c_void_p * n)(*[h.value for h in h2])
            _lib.check(L.amp_resblock_forward(a1, a2, n, ctypes.c_void_p(xd.data_ptr()), B, T, slope, ctypes.c_void_p(y.data_ptr()), st))
        else:
            cur = xd
            for p in range(n):
                y = torch.full_like(xd, float("nan"))
                _lib.check(L.amp_pair_forward(h1[p], h2[p], ctypes.c_void_p(cur.data_ptr()), B, T, slope, ctypes.c_void_p(y.data_ptr()), st))
                cur = y
        torch.cuda.synchronize()
        return y.cpu()
    finally:
        for h in h1 + h2:
            L.amp_conv_destroy(h)


def act1d_forward(x, alpha, beta, logscale, fu, fd):
    L = _lib.lib()
    xd = x.contiguous().float().cuda()
    B, C, T = xd.shape
    y = torch.full_like(xd, float("nan"))
    ad = alpha.contiguous().float().cuda()
    bd = beta.contiguous().float().cuda() if beta is not None else None
    fu = fu.contiguous().float()
    fd = fd.contiguous().float()
    _lib.check(L.amp_antialias_snake(ctypes.c_void_p(xd.data_ptr()), B, C, T, ctypes.c_void_p(ad.data_ptr()),
                                     ctypes.c_void_p(bd.data_ptr()) if bd is not None else None, int(logscale),
                                     ctypes.c_void_p(fu.data_ptr()), ctypes.c_void_p(fd.data_ptr()),
                                     ctypes.c_void_p(y.data_ptr()), _lib.current_stream_ptr(xd.device)))
    torch.cuda.synchronize()
    return y.cpu()


def ampblock_forward(ws1, bs1, ws2, bs2, alphas, betas, logscale, fu, fd, x, *, dilations, fused=True, mode=0, div=1.0, y0=None):
    """AMPBlock1 (bigvgan.py:137-146) on cuda:0 from per-pair weights and per-activation parameters (``alphas`` / ``betas``
    [2 * n, C]; ``betas`` None -> Snake).  fused=True -> ``amp_ampblock_forward`` (ONE launch, csrc/ampb_f16x3.hip);
    fused=False -> the launches it replaces: ``amp_antialias_snake`` -> ``amp_conv_forward`` -> ``amp_antialias_snake`` ->
    ``amp_conv_forward`` (with the residual; the last conv through ``amp_conv_forward_mrf`` with the MRF ``mode``, bigvgan.py:320-327).
    ``y0``: the running MRF sum for modes 1 / 2.  CPU tensors in and out."""
    L = _lib.lib()
    C, _, k = ws1[0].shape
    n = len(dilations)
    h1, h2 = [], []
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    try:
        for ws, bs, hs, ds in ((ws1, bs1, h1, dilations), (ws2, bs2, h2, [1] * n)):
            for w, b, d in zip(ws, bs, ds):
                h = ctypes.c_void_p()
                w, b = w.contiguous().float(), b.contiguous().float()
                _lib.check(L.amp_conv_create(0, C, C, k, 1, d, (k * d - d) // 2, p(w), p(b), ctypes.byref(h)))
                hs.append(h)
        xd = x.contiguous().float().cuda()
        B, _, T = xd.shape
        st = _lib.current_stream_ptr(xd.device)
        ad = alphas.contiguous().float().cuda()
        bd = betas.contiguous().float().cuda() if betas is not None else None
        fu, fd = fu.contiguous().float(), fd.contiguous().float()
        y = y0.contiguous().float().cuda().clone() if y0 is not None else torch.full_like(xd, float("nan"))
        if fused:
            a1, a2 = (ctypes.c_void_p * n)(*[h.value for h in h1]), (ctypes.c_void_p * n)(*[h.value for h in h2])
            _lib.check(L.amp_ampblock_forward(a1, a2, n, p(ad), p(bd), int(logscale), p(fu), p(fd), p(xd), B, T, p(y), mode, div, st))
        else:
            act = torch.empty_like(xd)
            xt = torch.empty_like(xd)
            cur = xd
            for i in range(n):
                for j, h in ((0, h1[i]), (1, h2[i])):
                    s = 2 * i + j
                    src = cur if j == 0 else xt
                    _lib.check(L.amp_antialias_snake(p(src), B, C, T, p(ad[s]), p(bd[s]) if bd is not None else None, int(logscale),
                                                     p(fu), p(fd), p(act), st))
                    if j == 0:
                        _lib.check(L.amp_conv_forward(h, p(act), B, T, 1.0, None, 1.0, p(xt), st))
                    elif i + 1 < n:
                        nxt = torch.empty_like(xd)
                        _lib.check(L.amp_conv_forward(h, p(act), B, T, 1.0, p(cur), 1.0, p(nxt), st))
                        cur = nxt
                    else:
                        _lib.check(L.amp_conv_forward_mrf(h, p(act), B, T, 1.0, p(cur), p(y), mode, div, st))
        torch.cuda.synchronize()
        return y.cpu()
    finally:
        for h in h1 + h2:
            L.amp_conv_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------
# the codec ops (amp_tconv_*, amp_sconv_*, amp_codec_unit_*, amp_aa_unit_*): CPU tensors in and out, like conv_forward.  Every output and
# workspace lies inside a larger NaN-filled buffer with SENTINEL floats in front and behind: after the call the sentinels must be untouched
# and every output element finite (a dropped store is a NaN).  `xs` may be one tensor or a list of them (one handle, one call each; a list
# comes back).  `info`, when given, receives the handle's route ("fused") and the library's output lengths ("out_len": {T: T_out}).
# ------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 64
_NAN_BITS = int(torch.full((1,), float("nan")).view(torch.int32).item())


class Guarded:
    """a NaN-filled device tensor of `shape` between two runs of SENTINEL NaN floats; 16-byte aligned"""

    def __init__(self, shape):
        self.n = 1
        for v in shape:
            self.n *= int(v)
        self.buf = torch.full((self.n + 2 * SENTINEL,), float("nan"), device="cuda")
        self.t = self.buf[SENTINEL:SENTINEL + self.n].view(*shape)
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def check(self, what, finite=True):
        bits = self.buf.view(torch.int32)
        for name, part in (("in front of", bits[:SENTINEL]), ("behind", bits[SENTINEL + self.n:])):
            hit = (part != _NAN_BITS).nonzero().flatten().tolist()
            assert not hit, f"{what}: the sentinel floats {hit[:8]} {name} the tensor were written"
        if finite:
            bad = (~torch.isfinite(self.t)).nonzero()
            assert bad.numel() == 0, (f"{what}: {bad.shape[0]} of {self.n} outputs were not written or are not finite; first at "
                                      f"{bad[:6].tolist()} of {tuple(self.t.shape)}")


def _cp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _host(t):
    return t.detach().contiguous().float().cpu() if t is not None else None


def _as_list(xs):
    return (list(xs), True) if isinstance(xs, (list, tuple)) else ([xs], False)


class _Fusion:
    """amp_set_*_fusion(mode) around a create; back to the policy afterwards"""

    def __init__(self, setter, mode):
        self.setter, self.mode = setter, mode

    def __enter__(self):
        if self.mode is not None:
            _lib.check(self.setter(int(self.mode)))

    def __exit__(self, *exc):
        if self.mode is not None:
            _lib.check(self.setter(-1))


def tconv_forward(w, b, xs, alpha=None, *, stride, padding, output_padding=0, fusion=None, info=None):
    """amp_tconv_*: y = ConvTranspose1d(k = 2 stride, stride, padding, output_padding)([snake](x)).  w [cin, cout, 2 stride] folded, b [cout] or
    None, alpha [cin] or None; fusion: amp_set_tconv_fusion's mode for this handle."""
    L = _lib.lib()
    w, b, alpha = _host(w), _host(b), _host(alpha)
    cin, cout, k = w.shape
    assert k == 2 * stride
    xs, many = _as_list(xs)
    h = ctypes.c_void_p()
    with _Fusion(L.amp_set_tconv_fusion, fusion):
        _lib.check(L.amp_tconv_create(cin, cout, stride, padding, output_padding, _cp(w), _cp(b), ctypes.byref(h)))
    try:
        if info is not None:
            info.update(fused=int(L.amp_tconv_fused(h)), out_len={})
        ad = alpha.reshape(-1).cuda() if alpha is not None else None
        out = []
        for x in xs:
            xd = _host(x).cuda()
            B, _, T = xd.shape
            Tout = L.amp_tconv_out_len(h, T)
            if info is not None:
                info["out_len"][T] = Tout
            y = Guarded((B, cout, Tout if Tout > 0 else 1))       # (T_out <= 0 is the library's to refuse: it still gets a real pointer)
            need = L.amp_tconv_workspace_bytes(h, B, T)
            ws = Guarded(((need + 3) // 4,)) if need else None
            _lib.check(L.amp_tconv_forward(h, _cp(xd), B, T, _cp(ad), ws.ptr if ws else None, need, y.ptr, _lib.current_stream_ptr(xd.device)))
            torch.cuda.synchronize()
            y.check(f"amp_tconv_forward B={B} T={T}")
            if ws:
                ws.check(f"amp_tconv_forward workspace B={B} T={T}", finite=False)
            out.append(y.t.cpu())
        return out if many else out[0]
    finally:
        L.amp_tconv_destroy(h)


def sconv_forward(w, b, xs, alpha=None, *, stride, padding, info=None):
    """amp_sconv_*: y = Conv1d(k = 2 stride, stride, padding)([snake](x)).  w [cout, cin, 2 stride] folded, b [cout] or None, alpha [cin] or None"""
    L = _lib.lib()
    w, b, alpha = _host(w), _host(b), _host(alpha)
    cout, cin, k = w.shape
    assert k == 2 * stride
    xs, many = _as_list(xs)
    h = ctypes.c_void_p()
    _lib.check(L.amp_sconv_create(cin, cout, stride, padding, _cp(w), _cp(b), ctypes.byref(h)))
    try:
        if info is not None:
            info.update(out_len={})
        ad = alpha.reshape(-1).cuda() if alpha is not None else None
        out = []
        for x in xs:
            xd = _host(x).cuda()
            B, _, T = xd.shape
            Tout = L.amp_sconv_out_len(h, T)
            if info is not None:
                info["out_len"][T] = Tout
            y = Guarded((B, cout, Tout if Tout > 0 else 1))
            need = L.amp_sconv_workspace_bytes(h, B, T)
            ws = Guarded((max(1, (need + 3) // 4),))
            _lib.check(L.amp_sconv_forward(h, _cp(xd), B, T, _cp(ad), ws.ptr, need, y.ptr, _lib.current_stream_ptr(xd.device)))
            torch.cuda.synchronize()
            y.check(f"amp_sconv_forward B={B} T={T}")
            ws.check(f"amp_sconv_forward workspace B={B} T={T}", finite=need > 0)     # the repack kernel writes every workspace element
            out.append(y.t.cpu())
        return out if many else out[0]
    finally:
        L.amp_sconv_destroy(h)


def _unit_calls(L, h, prefix, xs, C, info):
    fwd, wsb = getattr(L, prefix + "_forward"), getattr(L, prefix + "_workspace_bytes")
    if info is not None:
        info.update(fused=int(getattr(L, prefix + "_fused")(h)))
    out = []
    for x in xs:
        xd = _host(x).cuda()
        B, _, T = xd.shape
        y = Guarded((B, C, T))
        need = wsb(h, B, T)
        ws = Guarded(((need + 3) // 4,)) if need else None
        _lib.check(fwd(h, _cp(xd), B, T, y.ptr, ws.ptr if ws else None, need, _lib.current_stream_ptr(xd.device)))
        torch.cuda.synchronize()
        y.check(f"{prefix}_forward B={B} T={T}")
        if ws:
            ws.check(f"{prefix}_forward workspace B={B} T={T}")
        out.append(y.t.cpu())
    return out


def codec_unit_forward(alpha1, w1, b1, alpha2, w2, b2, xs, *, dilation, fusion=None, info=None):
    """amp_codec_unit_*: y = x + conv1x1(snake_2(conv7(snake_1(x)))).  alpha* [C], w1 [C, C, 7] and w2 [C, C, 1] folded, b* [C]"""
    L = _lib.lib()
    t = [_host(v) for v in (alpha1, w1, b1, alpha2, w2, b2)]
    C = t[1].shape[0]
    xs, many = _as_list(xs)
    h = ctypes.c_void_p()
    with _Fusion(L.amp_set_codec_unit_fusion, fusion):
        _lib.check(L.amp_codec_unit_create(C, dilation, *[_cp(v) for v in t], ctypes.byref(h)))
    try:
        out = _unit_calls(L, h, "amp_codec_unit", xs, C, info)
        return out if many else out[0]
    finally:
        L.amp_codec_unit_destroy(h)


def aa_unit_forward(alpha1, beta1, w1, b1, alpha2, beta2, w2, b2, fu, fd, xs, *, dilation, logscale=True, fusion=None, info=None):
    """amp_aa_unit_*: y = x + conv1x1(A2(conv7(A1(x)))), A = Activation1d(SnakeBeta | Snake: beta* None).  fu / fd: the two 12-tap filters"""
    L = _lib.lib()
    t = [_host(v) for v in (alpha1, beta1, w1, b1, alpha2, beta2, w2, b2)]
    f = [_host(fu).reshape(-1), _host(fd).reshape(-1)]
    C = t[2].shape[0]
    xs, many = _as_list(xs)
    h = ctypes.c_void_p()
    with _Fusion(L.amp_set_aa_unit_fusion, fusion):
        _lib.check(L.amp_aa_unit_create(C, dilation, *[_cp(v) for v in t], int(logscale), _cp(f[0]), _cp(f[1]), ctypes.byref(h)))
    try:
        out = _unit_calls(L, h, "amp_aa_unit", xs, C, info)
        return out if many else out[0]
    finally:
        L.amp_aa_unit_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------
# the mel / STFT entry points with raw pointers (tests/test_gpu_stft_geometry.py).  These return the status instead of raising, so a refusal can
# be looked at; `Fenced` is `Guarded` with a choice of fill (a finite sentinel where NaN is a legitimate input) and of alignment.
# ------------------------------------------------------------------------------------------------------------------------------
class Fenced:
    """a device tensor of `shape`, `offset` floats off a 16-byte boundary, filled with `fill` and between two runs of SENTINEL floats of it"""

    def __init__(self, shape, offset=0, fill=float("nan")):
        self.n = 1
        for v in shape:
            self.n *= int(v)
        self.fill = fill
        self.lo = SENTINEL + offset
        self.buf = torch.full((self.n + 2 * SENTINEL + offset,), fill, device="cuda")
        self.t = self.buf[self.lo:self.lo + self.n].view(*shape)
        assert self.t.data_ptr() % 16 == 4 * (offset % 4)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def untouched(self, part):
        return torch.isnan(part) if self.fill != self.fill else part == self.fill

    def check_fences(self, what):
        torch.cuda.synchronize()
        for name, part in (("in front of", self.buf[:self.lo]), ("behind", self.buf[self.lo + self.n:])):
            hit = (~self.untouched(part)).nonzero().flatten().tolist()
            assert not hit, f"{what}: the sentinel floats {hit[:8]} {name} the tensor were written"

    def check_written(self, what):
        self.check_fences(what)
        bad = (~torch.isfinite(self.t) | self.untouched(self.t)).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {self.n} elements were not written or are not finite; first at {bad[:4].tolist()}"
        return self.t


def mel_desc(n_fft, win, hop, n_mel=0, pad_mode=0, mag_eps=0.0, log_clip=0.0):
    return _lib.amp_mel_desc(n_fft, win, hop, n_mel, pad_mode, mag_eps, log_clip, None)


def _raw(t):
    """c_void_p of a tensor, a Fenced, or None"""
    if t is None:
        return None
    return t.ptr if isinstance(t, Fenced) else ctypes.c_void_p(t.data_ptr())


def _st():
    return _lib.current_stream_ptr(torch.device("cuda:0"))


def last_error():
    return _lib.lib().amp_last_error().decode("utf-8", "replace")


def istft_call(mode, d, a, b, B, F, window, den, frames, wav, stride=0, clip=0.0):
    """amp_istft_forward (a, b = mag, phase) / amp_istft_same (re, im) / amp_istft_same_polar (a = head) -> status"""
    L = _lib.lib()
    if mode == "forward":
        return L.amp_istft_forward(ctypes.byref(d), _raw(a), _raw(b), B, F, _raw(window), _raw(den), _raw(frames), _raw(wav), _st())
    if mode == "same":
        return L.amp_istft_same(ctypes.byref(d), _raw(a), _raw(b), B, F, _raw(window), _raw(den), _raw(frames), _raw(wav), _st())
    return L.amp_istft_same_polar(ctypes.byref(d), _raw(a), int(stride), B, F, float(clip), _raw(window), _raw(den), _raw(frames), _raw(wav), _st())


def mel_forward_call(d, wav, lens, B, Ln, window, basis, mel, mag, re, im):
    """amp_mel_forward_ragged (lens None: full rows) -> status"""
    return _lib.lib().amp_mel_forward_ragged(ctypes.byref(d), _raw(wav), _raw(lens), B, Ln, _raw(window), _raw(basis), _raw(mel), _raw(mag),
                                             _raw(re), _raw(im), _st())


def mel_backward_call(d, lens, B, Ln, window, basis, mel_lin, mag, re, im, g, spec_ws, frames_ws, gw):
    """amp_mel_backward -> status"""
    return _lib.lib().amp_mel_backward(ctypes.byref(d), _raw(lens), B, Ln, _raw(window), _raw(basis), _raw(mel_lin), _raw(mag), _raw(re),
                                       _raw(im), _raw(g), _raw(spec_ws), _raw(frames_ws), _raw(gw), _st())
