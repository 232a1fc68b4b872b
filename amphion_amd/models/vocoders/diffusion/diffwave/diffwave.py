"""DiffWave drop-in (models/vocoders/diffusion/diffwave/diffwave.py:127-179) on the gfx950 kernels.

Same constructor (``DiffWave(cfg)``, including the ``cfg.model.diffwave.noise_schedule`` it writes, :131-135), same sub-module and
parameter names, same ``forward(audio[B, L], diffusion_step[1 | B], spectrogram[B, n_mel, F]) -> [B, 1, L]``.  Inference only.

    spectrogram_upsampler                     2 launches, once per utterance (``condition``)
    diffusion_embedding + N x diffusion_projection   1 launch -> a [N, C] table of per-channel constants
    relu(input_projection)                    1 launch
    N x ResidualBlock                         1 launch each (csrc/dw_layer_f16x3.hip)
    skip / sqrt(N) -> skip_projection -> relu -> output_projection    1 launch; ``sample_step`` fuses the sampler update into it

The packed weights live in one ``amp_dw`` handle, rebuilt when a parameter, the device or the precision changes.  After ``forward``
the op-level f16x3 range flag is checked (``_lib.range_check``): an activation beyond the split-f16 operand range raises ``AmpError``
(AMP_ERR_RANGE).  The sampler (diffusion_vocoder_inference.py) checks once per call and repeats in exact fp32.
"""
from __future__ import annotations

import ctypes
from math import sqrt  # noqa: F401  (the reference module exports it)

import numpy as np
import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import ptr as _p


def Conv1d(*args, **kwargs):
    layer = nn.Conv1d(*args, **kwargs)
    nn.init.kaiming_normal_(layer.weight)
    return layer


class DiffusionEmbedding(nn.Module):
    """diffwave.py:33-65 (parameters and the non-persistent table; the arithmetic runs in dw_embed_kernel)"""

    def __init__(self, max_steps):
        super().__init__()
        self.register_buffer("embedding", self._build_embedding(max_steps), persistent=False)
        self.projection1 = nn.Linear(128, 512)
        self.projection2 = nn.Linear(512, 512)

    def _build_embedding(self, max_steps):
        steps = torch.arange(max_steps).unsqueeze(1)
        dims = torch.arange(64).unsqueeze(0)
        table = steps * 10.0 ** (dims * 4.0 / 63.0)
        return torch.cat([torch.sin(table), torch.cos(table)], dim=1)


class SpectrogramUpsampler(nn.Module):
    """diffwave.py:68-93"""

    def __init__(self, upsample_factors):
        super().__init__()
        u0, u1 = upsample_factors[0], upsample_factors[1]
        self.conv1 = nn.ConvTranspose2d(1, 1, [3, u0 * 2], stride=[1, u0], padding=[1, u0 // 2])
        self.conv2 = nn.ConvTranspose2d(1, 1, [3, u1 * 2], stride=[1, u1], padding=[1, u1 // 2])


class ResidualBlock(nn.Module):
    """diffwave.py:96-124"""

    def __init__(self, n_mels, residual_channels, dilation):
        super().__init__()
        self.dilated_conv = Conv1d(residual_channels, 2 * residual_channels, 3, padding=dilation, dilation=dilation)
        self.diffusion_projection = nn.Linear(512, residual_channels)
        self.conditioner_projection = Conv1d(n_mels, 2 * residual_channels, 1)
        self.output_projection = Conv1d(residual_channels, 2 * residual_channels, 1)


class DiffWave(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        dw = cfg.model.diffwave
        dw.noise_schedule = np.linspace(dw.noise_schedule_factors[0], dw.noise_schedule_factors[1], dw.noise_schedule_factors[2]).tolist()
        C = dw.residual_channels
        self.input_projection = Conv1d(1, C, 1)
        self.diffusion_embedding = DiffusionEmbedding(len(dw.noise_schedule))
        self.spectrogram_upsampler = SpectrogramUpsampler(dw.upsample_factors)
        self.residual_layers = nn.ModuleList(
            [ResidualBlock(cfg.preprocess.n_mel, C, 2 ** (i % dw.dilation_cycle_length)) for i in range(dw.residual_layers)])
        self.skip_projection = Conv1d(C, C, 1)
        self.output_projection = Conv1d(C, 1, 1)
        nn.init.zeros_(self.output_projection.weight)
        self._cache = HandleCache("amp_dw_destroy")
        self._ws = {}

    # ---- geometry ----
    @property
    def hop(self):
        u = self.cfg.model.diffwave.upsample_factors
        return int(u[0]) * int(u[1])

    @property
    def max_steps(self):
        return self.diffusion_embedding.embedding.shape[0]

    def _desc(self):
        dw = self.cfg.model.diffwave
        return _lib.amp_dw_desc(int(dw.residual_channels), int(dw.residual_layers), int(dw.dilation_cycle_length), int(self.cfg.preprocess.n_mel),
                                int(dw.upsample_factors[0]), int(dw.upsample_factors[1]), int(self.max_steps))

    def handle(self, device):
        """the ``amp_dw`` handle holding this module's weights on ``device`` in the current precision"""
        tensors = list(self.state_dict().items()) + [("diffusion_embedding.embedding", self.diffusion_embedding.embedding)]
        return self._cache.get(param_sig([t for _, t in tensors], str(device), _lib.get_precision()), self._build, tensors, device)

    def _build(self, tensors, device):
        h = ctypes.c_void_p()
        d = self._desc()
        L = _lib.lib()
        with torch.cuda.device(device):
            _lib.check(L.amp_dw_create(ctypes.byref(d), ctypes.byref(h)))
            self._cache.adopt(h)      # from here on a failure destroys it (HandleCache.build)
            for k, t in tensors:
                w = host_f32(t)
                _lib.check(L.amp_dw_set_weight(h, k.encode(), _p(w), w.numel()))
            _lib.check(L.amp_dw_finalize(h))
        return h

    def workspace(self, B, F, device):
        key = (B, F, str(device))
        ws = self._ws.get(key)
        if ws is None:
            n = int(_lib.lib().amp_dw_workspace_bytes(self.handle(device), B, F))
            ws = torch.empty(n // 4, dtype=torch.float32, device=device)
            self._ws = {k: v for k, v in self._ws.items() if k[2] != str(device)}     # one shape per device
            self._ws[key] = ws
        return ws

    # ---- checks: everything is refused before a launch ----
    def _check_mel(self, spectrogram):
        mel = _lib.require_device_tensor(spectrogram, "DiffWave spectrogram")
        n_mel = int(self.cfg.preprocess.n_mel)
        if mel.dim() != 3 or mel.shape[1] != n_mel or mel.shape[0] < 1 or mel.shape[2] < 1:
            raise ValueError(f"DiffWave: expected a [B, {n_mel}, F] spectrogram, got {tuple(mel.shape)}")
        hop = getattr(self.cfg.preprocess, "hop_size", None)
        if hop is not None and int(hop) != self.hop:
            raise ValueError(f"DiffWave: cfg.preprocess.hop_size = {hop} but the upsample factors give {self.hop} (diffwave.py:117 would fail)")
        return mel

    def condition(self, spectrogram):
        """SpectrogramUpsampler: [B, n_mel, F] -> a fresh [B, n_mel, F * hop] conditioner (once per utterance)"""
        mel = self._check_mel(spectrogram)
        B, M, F = mel.shape
        dev = mel.device
        h = self.handle(dev)
        ws = self.workspace(B, F, dev)
        cond = torch.empty((B, M, F * self.hop), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().amp_dw_condition(h, _p(mel), B, F, _p(cond), _p(ws), ws.numel() * 4, _lib.current_stream_ptr(dev)))
        return cond

    def _check_audio(self, audio, mel):
        audio = _lib.require_device_tensor(audio, "DiffWave audio")
        B, _, F = mel.shape
        if audio.device != mel.device:
            raise RuntimeError(f"DiffWave: audio on {audio.device}, spectrogram on {mel.device}")
        if audio.dim() != 2 or audio.shape[0] != B:
            raise ValueError(f"DiffWave: expected [B = {B}, L] audio, got {tuple(audio.shape)}")
        if audio.shape[1] != F * self.hop:
            raise ValueError(f"DiffWave: audio length {audio.shape[1]} != {F} frames x hop {self.hop}")
        return audio

    def predict(self, audio, steps, cond, F, out=None):
        """eps [B, L] from a conditioner ``condition`` returned; ``steps``: float32 device tensor [1] or [B]"""
        B, L = audio.shape
        dev = audio.device
        h = self.handle(dev)
        ws = self.workspace(B, F, dev)
        eps = torch.empty((B, L), dtype=torch.float32, device=dev) if out is None else out
        with _lib.on_device(dev):
            _lib.check(_lib.lib().amp_dw_forward(h, _p(audio), L, _p(steps), steps.numel(), _p(cond), B, F, _p(eps), _p(ws), ws.numel() * 4,
                                                 _lib.current_stream_ptr(dev)))
        return eps

    def sample_step(self, audio, step, c1, c2, sigma, noise, cond, F, h=None, ws=None):
        """one sampler step in place on ``audio`` (diffusion_vocoder_inference.py:58-71); ``h`` / ``ws``: the handle and workspace when the
        caller already holds them (the sampler looks them up once per call, not once per step)"""
        B, L = audio.shape
        dev = audio.device
        h = self.handle(dev) if h is None else h
        ws = self.workspace(B, F, dev) if ws is None else ws
        with _lib.on_device(dev):
            _lib.check(_lib.lib().amp_dw_sample_step(h, _p(audio), L, float(step), float(c1), float(c2), float(sigma), _p(noise), _p(cond), B, F,
                                                     _p(ws), ws.numel() * 4, _lib.current_stream_ptr(dev)))
        return audio

    def forward(self, audio, diffusion_step, spectrogram):
        mel = self._check_mel(spectrogram)
        audio = self._check_audio(audio, mel)
        B = mel.shape[0]
        if not isinstance(diffusion_step, torch.Tensor) or diffusion_step.dim() != 1 or diffusion_step.numel() not in (1, B):
            raise ValueError(f"DiffWave: diffusion_step must be a tensor of shape [1] or [{B}]")
        host = diffusion_step.detach().to("cpu", torch.float64)
        if not bool(((host >= 0) & (host <= self.max_steps - 1)).all()):
            raise IndexError(f"DiffWave: diffusion_step {host.tolist()} outside [0, {self.max_steps - 1}]")
        steps = host.to(torch.float32).to(mel.device)
        cond = self.condition(mel)
        eps = self.predict(audio, steps, cond, mel.shape[2])
        _lib.range_check(mel.device)
        return eps[:, None, :]
