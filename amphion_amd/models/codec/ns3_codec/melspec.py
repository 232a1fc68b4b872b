"""``MelSpectrogram`` drop-in (models/codec/ns3_codec/melspec.py:39-102) on the fused mel front-end kernel (``amp_mel_forward``): reflect pad
(n_fft - hop) / 2, the Hann window of ``win_size`` centred in the n_fft frame as ``torch.stft`` places it, |X| = sqrt(re^2 + im^2 + 1e-9), the
mel filterbank, log(clamp(., 1e-5)) -- one launch.  Same constructor, the same persistent buffers ``mel_basis`` and ``hann_window``."""
from __future__ import annotations

import types

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.utils import mel as _mel


class MelSpectrogram(nn.Module):
    def __init__(self, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
        super().__init__()
        if center:
            raise NotImplementedError("MelSpectrogram: center=True is not on the HIP path (FACodec builds it with center=False)")
        if win_size > n_fft:
            raise ValueError(f"MelSpectrogram: win_size {win_size} exceeds n_fft {n_fft}")
        self.n_fft = n_fft
        self.hop_size = hop_size
        self.win_size = win_size
        self.sampling_rate = sampling_rate
        self.num_mels = num_mels
        self.fmin = fmin
        self.fmax = fmax
        self.center = center
        mel = _mel.librosa_mel_fn(sr=sampling_rate, n_fft=n_fft, n_mels=num_mels, fmin=fmin, fmax=fmax)
        self.register_buffer("mel_basis", torch.from_numpy(mel).float())
        self.register_buffer("hann_window", torch.hann_window(win_size))
        self._cfg = types.SimpleNamespace(n_fft=n_fft, win_size=win_size, hop_size=hop_size)
        self._frame_window = None       # (key, hann_window centred in an n_fft frame): what the kernel multiplies a frame by

    def _window(self):
        w = self.hann_window
        key = (w.data_ptr(), w._version, str(w.device))
        if self._frame_window is None or self._frame_window[0] != key:
            lp = (self.n_fft - self.win_size) // 2
            self._frame_window = (key, torch.nn.functional.pad(w, (lp, self.n_fft - self.win_size - lp)).contiguous())
        return self._frame_window[1]

    def forward(self, y):
        """y [B, L] -> log-mel [B, num_mels, F], F = 1 + (L - hop_size) // hop_size"""
        y = _lib.require_device_tensor(y, "MelSpectrogram input")
        if y.dim() != 2 or y.shape[0] < 1:
            raise ValueError(f"MelSpectrogram: expected audio [B, L], got {tuple(y.shape)}")
        pad = int((self.n_fft - self.hop_size) / 2)
        if y.shape[1] <= pad:
            raise ValueError(f"MelSpectrogram: {y.shape[1]} samples are too few for the reflection padding of {pad}")
        for name in ("mel_basis", "hann_window"):
            t = getattr(self, name)
            if t.device != y.device or t.dtype != torch.float32:
                raise RuntimeError(f"MelSpectrogram: {name} is {t.dtype} on {t.device}, the input float32 on {y.device}: move the module")
        return _mel._run(y, self._cfg, n_mel=self.num_mels, pad_mode=0, mag_eps=1e-9, log_clip=1e-5, basis=self.mel_basis.contiguous(),
                         window=self._window())["mel"]
