"""Drop-in side of models/vocoders/diffusion/diffusion_vocoder_inference.py: the DiffWave sampler (:13-73) and the list API (:76-131).

Each sampler step is N + 3 launches (amp_dw_sample_step); torch supplies memory, the stream and the Gaussian draws.  The range flag of
the f16x3 kernels is read once per sampler call, before the copy to the host; a call that left the operand range is repeated in exact
fp32 with the same noise."""
from __future__ import annotations

import numpy as np
import torch

from amphion_amd import _lib


def schedule(cfg, fast_inference=False):
    """T, c1, c2, sigma per inference step (diffusion_vocoder_inference.py:23-46,56-69), in float64 as the reference's numpy"""
    training = np.array(cfg.model.diffwave.noise_schedule)
    inference = np.array(cfg.model.diffwave.inference_noise_schedule) if fast_inference else training
    talpha_cum = np.cumprod(1 - training)
    beta = inference
    alpha = 1 - beta
    alpha_cum = np.cumprod(alpha)
    T = []
    for s in range(len(inference)):
        for t in range(len(training) - 1):
            if talpha_cum[t + 1] <= alpha_cum[s] <= talpha_cum[t]:
                twiddle = (talpha_cum[t] ** 0.5 - alpha_cum[s] ** 0.5) / (talpha_cum[t] ** 0.5 - talpha_cum[t + 1] ** 0.5)
                T.append(t + twiddle)
                break
    T = np.array(T, dtype=np.float32)
    if len(T) != len(inference):
        raise ValueError("the inference noise schedule does not map onto the training schedule (one index per step)")
    c1 = 1 / alpha ** 0.5
    c2 = beta / (1 - alpha_cum) ** 0.5
    sigma = np.zeros_like(beta)
    sigma[1:] = ((1.0 - alpha_cum[:-1]) / (1.0 - alpha_cum[1:]) * beta[1:]) ** 0.5
    return T, c1, c2, sigma


def _run(model, mels, cond, sched, noise_at):
    T, c1, c2, sigma = sched
    F = mels.shape[-1]
    audio = noise_at(0).clone()
    h, ws = model.handle(audio.device), model.workspace(audio.shape[0], F, audio.device)
    k = 1
    for n in range(len(T) - 1, -1, -1):
        z = None
        if n > 0:
            z = noise_at(k)
            k += 1
        model.sample_step(audio, T[n], c1[n], c2[n], sigma[n], z, cond, F, h, ws)
    return audio


def vocoder_inference(cfg, model, mels, f0s=None, device=None, fast_inference=False, *, noise=None):
    """mels [B, n_mel, F] -> CPU audio [B, F * hop].  ``noise``: the initial [B, L] tensor followed by one per step with n > 0, in
    order of use (default: ``torch.randn`` on the device, in the reference's call order and shapes)."""
    model.eval()
    with torch.no_grad():
        sched = schedule(cfg, fast_inference)
        mels = mels.to(device) if device is not None else mels
        mels = model._check_mel(mels.float() if isinstance(mels, torch.Tensor) else mels)
        B, _, F = mels.shape
        L = int(cfg.preprocess.hop_size) * F
        if L != model.hop * F:
            raise ValueError(f"DiffWave: hop_size {cfg.preprocess.hop_size} != upsample factors' {model.hop}")
        dev = mels.device
        drawn = []

        def noise_at(k):
            if noise is not None:
                z = _lib.require_device_tensor(noise[k].to(dev), "noise")
                if tuple(z.shape) != (B, L):
                    raise ValueError(f"noise[{k}] has shape {tuple(z.shape)}, expected {(B, L)}")
                return z
            while len(drawn) <= k:
                drawn.append(torch.randn(B, L, device=dev))
            return drawn[k]

        cond = model.condition(mels)
        audio = _run(model, mels, cond, sched, noise_at)
        try:
            _lib.range_check(dev)
        except _lib.AmpError as e:
            if e.status != _lib.AMP_ERR_RANGE:
                raise
            # exact fp32 with the same noise (the draws are kept)
            L_ = _lib.lib()
            h = model.handle(dev)
            _lib.check(L_.amp_dw_set_precision(h, _lib.AMP_PRECISION_F32))
            try:
                audio = _run(model, mels, model.condition(mels), sched, noise_at)
            finally:
                _lib.check(L_.amp_dw_set_precision(h, _lib.PRECISIONS[_lib.get_precision()]))
    return audio.detach().cpu()


def synthesis_audios(cfg, model, mels, f0s=None, batch_size=None, fast_inference=False):
    """list of [n_mel, T_i] mels -> list of [T_i * hop] audios (diffusion_vocoder_inference.py:76-131).  Each padded batch is ONE
    sampler call, so the random stream differs from the reference's per-item order."""
    from amphion_amd.utils.util import pad_mels_to_tensors

    device = next(model.parameters()).device
    audios = []
    mel_batches, mel_frames = pad_mels_to_tensors(mels, batch_size)
    for mel_batch, mel_frame in zip(mel_batches, mel_frames):
        audio = vocoder_inference(cfg, model, mel_batch, device=device, fast_inference=fast_inference)
        for i in range(mel_batch.shape[0]):
            audios.append(audio[i, : int(mel_frame[i]) * cfg.preprocess.hop_size])
    return audios
