"""Vocos drop-in (models/codec/amphion_codec/vocos.py:84-167,319-359,470-526,720-783,824-881) on the gfx950 kernels.

Same constructors (``Vocos(input_channels=..., ..., cfg=None)``: ``Vocos(cfg=cfg.model.vocos)`` and the codec decoder's keyword
call), same ``state_dict`` keys (the persistent ``head.istft.window`` buffer included), same ``forward(x[B, C_in, F]) ->
[B, 1, F * hop]``.  Everything runs at frame rate on channel-first [B, C, F] activations:

    embed (Conv1d k = 7)                      implicit-GEMM conv kernel (HipConv1d)
    norm, final_layer_norm                    channel LayerNorm (amp_layer_norm_c)
    per ConvNeXt block:
      dwconv (k = 7, groups = C) -> norm      one launch (amp_dwconv_layer_norm_c, K = 7)
      pwconv1 -> GELU                         pointwise f16x3 GEMM, GELU epilogue (amp_pw_forward)
      pwconv2 -> gamma * . + residual         pointwise f16x3 GEMM, layer-scale + residual epilogue, in place
    head.out                                  pointwise GEMM, bias epilogue -> [B, n_fft + 2, F]
    exp / clip / cos / sin + ISTFT "same"     read in place by the inverse-FFT frame kernel (amp_istft_same_polar)

3 * num_layers + 5 launches on the current stream (+ the inverse's overlap-add).  Work buffers are allocated once per
(B, F, device).  After the forward the op-level f16x3 range flag is checked (``_lib.range_check``): an activation beyond the
split-f16 operand range raises ``AmpError`` (AMP_ERR_RANGE) -- re-run with ``_lib.set_precision("f32")``.
Not on the HIP path (``NotImplementedError``): ``padding="center"`` and AdaLayerNorm (``adanorm_num_embeddings``).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.modules.hip_ops import HipConv1d

MAG_CLIP = 1e2          # ISTFTHead: torch.clip(exp(mag), max=1e2) (vocos.py:349-352)
LN_EPS = 1e-6


class _PwHandle:
    """The packed device copy of one nn.Linear for ``amp_pw_forward``, rebuilt when the parameters, the device or the precision
    change (a handle keeps the arithmetic it was created with)."""

    def __init__(self):
        self._cache = HandleCache("amp_pw_destroy")

    def get(self, lin: nn.Linear, device):
        return self._cache.get(param_sig((lin.weight, lin.bias), str(device), _lib.get_precision()), self._build, lin, device)

    def _build(self, lin, device):
        w, b = host_f32(lin.weight), host_f32(lin.bias)
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_pw_create(lin.in_features, lin.out_features, _p(w), _p(b), ctypes.byref(h)))
        return h


def pw_forward(handle, lin: nn.Linear, x, epilogue, out, gamma=None, res=None, x_batch_stride=0):
    """out[b] = epi(lin.weight @ x[b] + lin.bias) on [B, C, T] tensors (``amp_pw_forward``)"""
    dev = x.device
    B, T = x.shape[0], x.shape[-1]
    h = handle.get(lin, dev)
    with _lib.on_device(dev):
        _lib.check(_lib.lib().amp_pw_forward(h, _p(x), int(x_batch_stride), B, T, int(epilogue), _p(gamma), _p(res), _p(out),
                                             _lib.current_stream_ptr(dev)))
    return out


def _check_tensors(module, dev, who):
    """Every parameter and buffer of `module` whose pointer goes to a kernel must be a contiguous float32 tensor on `dev` (the
    kernels read them through raw device pointers: a host or other-device tensor would be a fault, not an error)."""
    for name, t in list(module.named_parameters()) + list(module.named_buffers()):
        if t.device != dev:
            raise RuntimeError(f"{who}: {name} is on {t.device} but the input is on {dev}: move the module to the input's device")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError(f"{who}: {name} must be contiguous")


def _check_input(x, channels, who):
    x = _lib.require_device_tensor(x, f"{who} input")
    if x.dim() != 3:
        raise ValueError(f"{who}: expected a [B, C, T] input, got {tuple(x.shape)}")
    if x.shape[1] != channels:
        raise ValueError(f"{who}: expected {channels} input channels, got {x.shape[1]}")
    if x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f"{who}: empty input {tuple(x.shape)}")
    return x


def _no_adanorm(adanorm_num_embeddings):
    if adanorm_num_embeddings is not None:
        raise NotImplementedError("Vocos with AdaLayerNorm (adanorm_num_embeddings) is not on the HIP path: no reference config sets it")


class ISTFT(nn.Module):
    """vocos.py:84-167, ``padding="same"`` only; ``forward(spec)`` takes the complex spectrogram [B, n_fft/2+1, F] like the
    reference.  The Vocos forward does not build the complex tensor: ``forward_head`` reads the head Linear's output in place."""

    def __init__(self, n_fft: int, hop_length: int, win_length: int, padding: str = "same"):
        super().__init__()
        if padding not in ["center", "same"]:
            raise ValueError("Padding must be 'center' or 'same'.")
        if padding != "same":
            raise NotImplementedError("ISTFT padding='center' (torch.istft) is not on the HIP path: only 'same' runs on the MI355X")
        if win_length != n_fft:
            raise NotImplementedError("the HIP ISTFT needs win_length == n_fft (what ISTFTHead builds)")
        self.padding = padding
        self.n_fft = n_fft
        self.hop_length = hop_length
        self.win_length = win_length
        self.register_buffer("window", torch.hann_window(win_length))
        self._env = {}

    def envelope(self, F, dev):
        """overlap-added window^2 (vocos.py:152-161), uncropped, cached per (F, device)"""
        key = (F, str(dev), self.window.data_ptr(), self.window._version)
        env = self._env.get(key)
        if env is None:
            w2 = self.window.detach().double().cpu().numpy() ** 2
            e = np.zeros((F - 1) * self.hop_length + self.win_length, dtype=np.float64)
            for f in range(F):
                e[f * self.hop_length: f * self.hop_length + self.win_length] += w2
            pad = (self.win_length - self.hop_length) // 2
            if not (e[pad: len(e) - pad] > 1e-11).all():
                raise ValueError("ISTFT: the window envelope vanishes inside the output (vocos.py:164)")
            env = torch.from_numpy(e.astype(np.float32)).to(dev)
            self._env = {k: v for k, v in self._env.items() if k[1] != str(dev)}
            self._env[key] = env
        return env

    def _desc(self):
        return _lib.amp_mel_desc(self.n_fft, self.win_length, self.hop_length, 0, 1, 0.0, 0.0)

    def forward_head(self, head, out, frames, head_batch_stride=0):
        """head [B, n_fft + 2, F] (log-magnitude rows, then phase rows) -> out [B, F * hop]"""
        B, _, F = head.shape
        dev = head.device
        env = self.envelope(F, dev)
        d = self._desc()
        with _lib.on_device(dev):
            _lib.check(_lib.lib().amp_istft_same_polar(ctypes.byref(d), _p(head), int(head_batch_stride), B, F, MAG_CLIP, _p(self.window),
                                                       _p(env), _p(frames), _p(out), _lib.current_stream_ptr(dev)))
        return out

    def forward(self, spec):
        if not isinstance(spec, torch.Tensor) or not spec.is_cuda:
            raise RuntimeError("ISTFT: the spectrogram must be a tensor on a ROCm device (there is no CPU fallback)")
        if spec.dim() != 3 or spec.shape[1] != self.n_fft // 2 + 1 or spec.shape[2] < 1:
            raise ValueError(f"ISTFT: expected a [B, {self.n_fft // 2 + 1}, F] spectrogram, got {tuple(spec.shape)}")
        B, N, F = spec.shape
        dev = spec.device
        _check_tensors(self, dev, "ISTFT")
        re = spec.real.float().contiguous()
        im = spec.imag.float().contiguous()
        env = self.envelope(F, dev)
        frames = torch.empty((B, F, self.n_fft), device=dev)
        out = torch.empty((B, F * self.hop_length), device=dev)
        d = self._desc()
        with _lib.on_device(dev):
            _lib.check(_lib.lib().amp_istft_same(ctypes.byref(d), _p(re), _p(im), B, F, _p(self.window), _p(env), _p(frames), _p(out),
                                                 _lib.current_stream_ptr(dev)))
        return out


class ISTFTHead(nn.Module):
    """vocos.py:319-359: Linear(dim, n_fft + 2) -> exp / clip(1e2) magnitude, cos / sin phase -> ISTFT."""

    def __init__(self, dim: int, n_fft: int, hop_length: int, padding: str = "same"):
        super().__init__()
        out_dim = n_fft + 2
        self.out = torch.nn.Linear(dim, out_dim)
        self.istft = ISTFT(n_fft=n_fft, hop_length=hop_length, win_length=n_fft, padding=padding)
        self._pw = _PwHandle()

    def forward_cf(self, x, head_buf, frames, out):
        """x [B, dim, F] channel-first -> out [B, F * hop]"""
        pw_forward(self._pw, self.out, x, _lib.AMP_PW_BIAS, head_buf)
        return self.istft.forward_head(head_buf, out, frames)

    def forward(self, x):
        """x [B, L, H] as the reference takes it -> audio [B, L * hop]"""
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError("ISTFTHead: expected a [B, L, H] input")
        x = _check_input(x.transpose(1, 2), self.out.in_features, "ISTFTHead")
        B, _, F = x.shape
        dev = x.device
        _check_tensors(self, dev, "ISTFTHead")
        head = torch.empty((B, self.out.out_features, F), device=dev)
        frames = torch.empty((B, F, self.istft.n_fft), device=dev)
        out = torch.empty((B, F * self.istft.hop_length), device=dev)
        return self.forward_cf(x, head, frames, out)


class ConvNeXtBlock(nn.Module):
    """vocos.py:470-526 on [B, C, T]: x + gamma * pwconv2(gelu(pwconv1(LN(dwconv(x)))))."""

    def __init__(self, dim: int, intermediate_dim: int, layer_scale_init_value: float, adanorm_num_embeddings: Optional[int] = None):
        super().__init__()
        _no_adanorm(adanorm_num_embeddings)
        self.dwconv = nn.Conv1d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.adanorm = False
        self.norm = nn.LayerNorm(dim, eps=LN_EPS)
        self.pwconv1 = nn.Linear(dim, intermediate_dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(intermediate_dim, dim)
        self.gamma = (nn.Parameter(layer_scale_init_value * torch.ones(dim), requires_grad=True) if layer_scale_init_value > 0 else None)
        self._pw1, self._pw2 = _PwHandle(), _PwHandle()
        self._ones = {}

    def run(self, x, y, h):
        """x [B, dim, T] updated in place; y [B, dim, T] and h [B, intermediate, T] are scratch"""
        B, C, T = x.shape
        dev = x.device
        _lib.check(_lib.lib().amp_dwconv_layer_norm_c(_p(x), _p(self.dwconv.weight), _p(self.dwconv.bias), 7, 1, _p(self.norm.weight),
                                                      _p(self.norm.bias), None, B, C, T, LN_EPS, 0, _p(y), _lib.current_stream_ptr(dev)))
        pw_forward(self._pw1, self.pwconv1, y, _lib.AMP_PW_BIAS_GELU, h)
        gamma = self.gamma
        if gamma is None:
            gamma = self._ones.get(str(dev))
            if gamma is None:
                gamma = self._ones[str(dev)] = torch.ones(C, device=dev)
        pw_forward(self._pw2, self.pwconv2, h, _lib.AMP_PW_SCALE_RES, x, gamma=gamma, res=x)
        return x

    def forward(self, x, cond_embedding_id=None):
        x = _check_input(x, self.dwconv.in_channels, "ConvNeXtBlock").clone()
        _check_tensors(self, x.device, "ConvNeXtBlock")
        y = torch.empty_like(x)
        h = torch.empty((x.shape[0], self.pwconv1.out_features, x.shape[2]), device=x.device)
        with _lib.on_device(x.device):
            return self.run(x, y, h)


class VocosBackbone(nn.Module):
    """vocos.py:720-783: embed -> LayerNorm -> ConvNeXt blocks -> final LayerNorm; ``forward`` returns [B, T, dim] like the reference."""

    def __init__(self, input_channels: int, dim: int, intermediate_dim: int, num_layers: int, layer_scale_init_value: Optional[float] = None,
                 adanorm_num_embeddings: Optional[int] = None):
        super().__init__()
        _no_adanorm(adanorm_num_embeddings)
        self.input_channels = input_channels
        self.embed = HipConv1d(input_channels, dim, 7, padding=3, weight_norm=False)
        self.adanorm = False
        self.norm = nn.LayerNorm(dim, eps=LN_EPS)
        layer_scale_init_value = layer_scale_init_value or 1 / num_layers
        self.convnext = nn.ModuleList([ConvNeXtBlock(dim=dim, intermediate_dim=intermediate_dim, layer_scale_init_value=layer_scale_init_value)
                                       for _ in range(num_layers)])
        self.final_layer_norm = nn.LayerNorm(dim, eps=LN_EPS)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, (nn.Conv1d, nn.Linear, HipConv1d)):
            nn.init.trunc_normal_(m.weight, std=0.02)
            nn.init.constant_(m.bias, 0)

    def forward_cf(self, x, bufs):
        """x [B, C_in, F] -> [B, dim, F] channel-first, in bufs["y"]"""
        B, _, F = x.shape
        dev = x.device
        C = self.norm.normalized_shape[0]
        st = _lib.current_stream_ptr(dev)
        L = _lib.lib()
        a, y, h = bufs["a"], bufs["y"], bufs["h"]
        self.embed(x, out=y)
        _lib.check(L.amp_layer_norm_c(_p(y), None, _p(self.norm.weight), _p(self.norm.bias), None, B, C, F, LN_EPS, 0, _p(a), st))
        for blk in self.convnext:
            blk.run(a, y, h)
        _lib.check(L.amp_layer_norm_c(_p(a), None, _p(self.final_layer_norm.weight), _p(self.final_layer_norm.bias), None, B, C, F,
                                      LN_EPS, 0, _p(y), st))
        return y

    def forward(self, x, **kwargs):
        x = _check_input(x, self.input_channels, "VocosBackbone")
        _check_tensors(self, x.device, "VocosBackbone")
        B, _, F = x.shape
        C = self.norm.normalized_shape[0]
        inter = self.convnext[0].pwconv1.out_features if len(self.convnext) else 1
        bufs = {"a": x.new_empty((B, C, F)), "y": x.new_empty((B, C, F)), "h": x.new_empty((B, inter, F))}
        with _lib.on_device(x.device):
            return self.forward_cf(x, bufs).transpose(1, 2)


class Vocos(nn.Module):
    """vocos.py:824-881."""

    def __init__(self, input_channels: int = 256, dim: int = 384, intermediate_dim: int = 1152, num_layers: int = 8, n_fft: int = 800,
                 hop_size: int = 200, padding: str = "same", adanorm_num_embeddings=None, cfg=None):
        super().__init__()

        def pick(name, default):
            return getattr(cfg, name) if cfg is not None and hasattr(cfg, name) else default

        input_channels = pick("input_channels", input_channels)
        dim = pick("dim", dim)
        intermediate_dim = pick("intermediate_dim", intermediate_dim)
        num_layers = pick("num_layers", num_layers)
        adanorm_num_embeddings = pick("adanorm_num_embeddings", adanorm_num_embeddings)
        n_fft = pick("n_fft", n_fft)
        hop_size = pick("hop_size", hop_size)
        padding = pick("padding", padding)
        self.backbone = VocosBackbone(input_channels=input_channels, dim=dim, intermediate_dim=intermediate_dim, num_layers=num_layers,
                                      adanorm_num_embeddings=adanorm_num_embeddings)
        self.head = ISTFTHead(dim, n_fft, hop_size, padding)
        self._bufs = {}

    def _buffers_for(self, B, F, dev):
        key = (B, F, str(dev))
        bufs = self._bufs.get(key)
        if bufs is None:
            C = self.backbone.norm.normalized_shape[0]
            inter = self.backbone.convnext[0].pwconv1.out_features if len(self.backbone.convnext) else 1
            n_fft, hop = self.head.istft.n_fft, self.head.istft.hop_length
            mk = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
            bufs = {"a": mk(B, C, F), "y": mk(B, C, F), "h": mk(B, inter, F), "head": mk(B, n_fft + 2, F), "frames": mk(B, F, n_fft),
                    }
            self._bufs = {k: v for k, v in self._bufs.items() if k[2] != str(dev)}    # one shape per device
            self._bufs[key] = bufs
        return bufs

    def forward(self, x):
        """x [B, input_channels, F] -> audio [B, 1, F * hop], a fresh tensor (the work buffers stay inside)"""
        x = _check_input(x, self.backbone.input_channels, "Vocos")
        B, _, F = x.shape
        dev = x.device
        _check_tensors(self, dev, "Vocos")
        bufs = self._buffers_for(B, F, dev)
        wav = torch.empty((B, F * self.head.istft.hop_length), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            feat = self.backbone.forward_cf(x, bufs)
            wav = self.head.forward_cf(feat, bufs["head"], bufs["frames"], wav)
        _lib.range_check(dev)
        return wav[:, None, :]
