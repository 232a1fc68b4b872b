"""Restatement of DiffWave (models/vocoders/diffusion/diffwave/diffwave.py) and of its sampler
(models/vocoders/diffusion/diffusion_vocoder_inference.py:13-73) in plain torch, in the dtype of the weights handed in (fp64 is the
yardstick of the GPU tests, fp32 measures the reference's own round-off), plus seeded synthetic weights and inputs.
tests/golden/make_golden_diffwave.py ties it to the real classes."""
from math import sqrt
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F


def make_cfg(C=64, N=30, cycle=10, n_mel=80, u=(16, 16), hop=None, factors=(1.0e-4, 0.05, 50), fast=(0.0001, 0.001, 0.01, 0.05, 0.2, 0.5)):
    """egs/vocoder/diffusion/diffwave/exp_config.json + config/diffwave.json, the fields the model and the sampler read"""
    return NS(preprocess=NS(n_mel=n_mel, hop_size=u[0] * u[1] if hop is None else hop),
              model=NS(generator="diffwave", diffwave=NS(residual_channels=C, residual_layers=N, dilation_cycle_length=cycle, upsample_factors=list(u),
                                                         noise_schedule_factors=list(factors), inference_noise_schedule=list(fast))))


SMALL = dict(C=32, N=4, cycle=3, n_mel=80, u=(4, 4))
WIDE = dict(C=64, N=10, cycle=10, n_mel=80, u=(16, 16))
RECIPE = dict(C=64, N=30, cycle=10, n_mel=80, u=(16, 16))
# gain of the drawn output_projection.weight per net: chosen on the fp64 restatement so that the predicted noise has rms >= 0.1 and
# at most 20 % of the sampler's final samples sit on the clamp (tests/test_oracle_diffwave.py asserts both)
OUT_GAIN = {"small": 1.0, "wide": 0.8, "recipe": 1.0}


def param_shapes(C, N, n_mel, u):
    """state_dict keys and shapes in registration order (diffwave.py:128-160; the embedding table is a non-persistent buffer)"""
    s = {"input_projection.weight": (C, 1, 1), "input_projection.bias": (C,),
         "diffusion_embedding.projection1.weight": (512, 128), "diffusion_embedding.projection1.bias": (512,),
         "diffusion_embedding.projection2.weight": (512, 512), "diffusion_embedding.projection2.bias": (512,),
         "spectrogram_upsampler.conv1.weight": (1, 1, 3, 2 * u[0]), "spectrogram_upsampler.conv1.bias": (1,),
         "spectrogram_upsampler.conv2.weight": (1, 1, 3, 2 * u[1]), "spectrogram_upsampler.conv2.bias": (1,)}
    for i in range(N):
        p = f"residual_layers.{i}."
        s[p + "dilated_conv.weight"] = (2 * C, C, 3)
        s[p + "dilated_conv.bias"] = (2 * C,)
        s[p + "diffusion_projection.weight"] = (C, 512)
        s[p + "diffusion_projection.bias"] = (C,)
        s[p + "conditioner_projection.weight"] = (2 * C, n_mel, 1)
        s[p + "conditioner_projection.bias"] = (2 * C,)
        s[p + "output_projection.weight"] = (2 * C, C, 1)
        s[p + "output_projection.bias"] = (2 * C,)
    s["skip_projection.weight"] = (C, C, 1)
    s["skip_projection.bias"] = (C,)
    s["output_projection.weight"] = (1, C, 1)
    s["output_projection.bias"] = (1,)
    return s


def synth_state_dict(C, N, n_mel, u, seed, out_gain=1.0):
    """Seeded weights: fan-in scaled normals, so that activations stay O(1) through N layers (the assertions of
    tests/test_oracle_diffwave.py pin that); output_projection.weight, zero in a fresh reference model, is drawn too."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in param_shapes(C, N, n_mel, u).items():
        if k.endswith(".bias"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
            continue
        fan_in = int(np.prod(shp[1:])) if len(shp) > 1 else shp[0]
        if k.startswith("spectrogram_upsampler"):
            fan_in = 6                                   # 3 mel taps x 2 time taps reach one output
        gain = 1.0
        if k == "output_projection.weight":
            gain = out_gain
        sd[k] = gain * torch.randn(shp, generator=g) / sqrt(fan_in)
    return sd


def synth_mel(B, n_mel, Fr, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n_mel, Fr, generator=g)


def embedding_table(max_steps):
    """diffwave.py:60-65, in fp32 as the reference builds it"""
    steps = torch.arange(max_steps).unsqueeze(1)
    dims = torch.arange(64).unsqueeze(0)
    table = steps * 10.0 ** (dims * 4.0 / 63.0)
    return torch.cat([torch.sin(table), torch.cos(table)], dim=1)


def silu(x):
    return x * torch.sigmoid(x)


def embed(sd, table, step):
    """diffwave.py:42-58: step int64 -> index, float -> lerp; returns [S, 512]"""
    dt = sd["diffusion_embedding.projection1.weight"].dtype
    table = table.to(dt)
    if step.dtype in (torch.int32, torch.int64):
        x = table[step]
    else:
        lo, hi = torch.floor(step).long(), torch.ceil(step).long()
        low, high = table[lo], table[hi]
        x = low + (high - low) * (step.to(dt) - lo.to(dt))[:, None]
    x = silu(F.linear(x, sd["diffusion_embedding.projection1.weight"], sd["diffusion_embedding.projection1.bias"]))
    return silu(F.linear(x, sd["diffusion_embedding.projection2.weight"], sd["diffusion_embedding.projection2.bias"]))


def dconst_table(sd, N, e):
    """every layer's diffusion_projection(e) (diffwave.py:113): [S, N, C]"""
    return torch.stack([F.linear(e, sd[f"residual_layers.{i}.diffusion_projection.weight"], sd[f"residual_layers.{i}.diffusion_projection.bias"])
                        for i in range(N)], dim=1)


def upsample(sd, u, mel):
    """diffwave.py:86-93"""
    x = mel.unsqueeze(1)
    for j in (0, 1):
        x = F.conv_transpose2d(x, sd[f"spectrogram_upsampler.conv{j + 1}.weight"], sd[f"spectrogram_upsampler.conv{j + 1}.bias"],
                               stride=[1, u[j]], padding=[1, u[j] // 2])
        x = F.leaky_relu(x, 0.4)
    return x.squeeze(1)


def layer(sd, i, d, x, dconst, cond, record=None):
    """diffwave.py:112-124; dconst [S, C] with S = 1 or B.  `record`: a dict that receives the staged operands and pre-activations"""
    p = f"residual_layers.{i}."
    y = x + dconst[:, :, None]
    a = F.conv1d(y, sd[p + "dilated_conv.weight"], sd[p + "dilated_conv.bias"], padding=d, dilation=d) \
        + F.conv1d(cond, sd[p + "conditioner_projection.weight"], sd[p + "conditioner_projection.bias"])
    gate, filt = torch.chunk(a, 2, dim=1)
    z = torch.sigmoid(gate) * torch.tanh(filt)
    r = F.conv1d(z, sd[p + "output_projection.weight"], sd[p + "output_projection.bias"])
    residual, skip = torch.chunk(r, 2, dim=1)
    if record is not None:
        record.update(y=y, a=a, z=z, r=r)
    return (x + residual) / sqrt(2.0), skip


def tail(sd, N, skip):
    """diffwave.py:175-178"""
    x = skip / sqrt(N)
    x = F.relu(F.conv1d(x, sd["skip_projection.weight"], sd["skip_projection.bias"]))
    return F.conv1d(x, sd["output_projection.weight"], sd["output_projection.bias"])


def forward(sd, hp, table, audio, step, mel=None, cond=None, stats=None):
    """DiffWave.forward (diffwave.py:162-179) -> [B, 1, L]; `stats`: a dict that receives max |staged operand|"""
    C, N, cycle, u = hp["C"], hp["N"], hp["cycle"], hp["u"]
    dt = sd["input_projection.weight"].dtype
    x = F.relu(F.conv1d(audio.to(dt).unsqueeze(1), sd["input_projection.weight"], sd["input_projection.bias"]))
    dc = dconst_table(sd, N, embed(sd, table, step))
    if cond is None:
        cond = upsample(sd, u, mel.to(dt))
    skip = None
    for i in range(N):
        rec = {} if stats is not None else None
        x, s = layer(sd, i, 2 ** (i % cycle), x, dc[:, i], cond, rec)
        skip = s if skip is None else s + skip
        if stats is not None:
            stats["staged"] = max(stats.get("staged", 0.0), rec["y"].abs().max().item(), rec["z"].abs().max().item())
    if stats is not None:
        stats["staged"] = max(stats["staged"], cond.abs().max().item())
    return tail(sd, N, skip)


def schedule(cfg, fast):
    """diffusion_vocoder_inference.py:23-46"""
    training = np.array(cfg.model.diffwave.noise_schedule)
    inference = np.array(cfg.model.diffwave.inference_noise_schedule) if fast else training
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
    return np.array(T, dtype=np.float32), alpha, beta, alpha_cum


def sample(sd, hp, table, cfg, mel, noise, fast, stats=None):
    """diffusion_vocoder_inference.py:48-73 with the draws injected: noise[0] is the initial audio, then one per step with n > 0"""
    T, alpha, beta, alpha_cum = schedule(cfg, fast)
    dt = sd["input_projection.weight"].dtype
    cond = upsample(sd, hp["u"], mel.to(dt))
    audio = noise[0].to(dt)
    k = 1
    for n in range(len(alpha) - 1, -1, -1):
        c1 = 1 / alpha[n] ** 0.5
        c2 = beta[n] / (1 - alpha_cum[n]) ** 0.5
        eps = forward(sd, hp, table, audio, torch.tensor([T[n]]), cond=cond, stats=stats).squeeze(1)
        if stats is not None:
            stats.setdefault("eps_rms", []).append(eps.pow(2).mean().sqrt().item())
        audio = c1 * (audio - c2 * eps)
        if n > 0:
            sigma = ((1.0 - alpha_cum[n - 1]) / (1.0 - alpha_cum[n]) * beta[n]) ** 0.5
            audio = audio + sigma * noise[k].to(dt)
            k += 1
        audio = torch.clamp(audio, -1.0, 1.0)
    return audio


def to_dtype(sd, dt):
    return {k: v.to(dt) for k, v in sd.items()}
