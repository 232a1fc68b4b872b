"""models/tts/fastspeech2/fs2.py on the HIP kernels: FastSpeech2 text -> mel, eval-mode inference (no targets in ``data``).

    Encoder / Decoder            FFT blocks (modules/transformer): 7 launches a block
    VariancePredictor            conv (k = 3, ReLU on store) -> amp_layer_norm_c -> conv (ReLU) -> amp_layer_norm_c_head      4 launches
    pitch / energy embedding     amp_bucketize_embed_add: scale, bucketize, gather and add in one launch, at EVERY column
    durations                    amp_fs2_durations (rounded durations, their running sum, the mel lengths), ONE host read of the mel
                                 lengths (it sizes the decoder batch), amp_expand_path for LengthRegulator
    mel_linear                   the pointwise GEMM
    PostNet                      five convs with BatchNorm folded in, tanh on store, the last one adding the mel        5 launches

The reference does not zero padded columns everywhere and its results depend on that: VariancePredictor has no mask between its convs,
the pitch embedding is added at padded phones too (the energy predictor's first conv reads it) and PostNet runs over ``mel_linear``'s bias
in padded frames.  So the predictors and PostNet run the PLAIN conv and LayerNorm over the full padded length here as well; only the FFT
blocks, whose ``masked_fill`` really zeroes, use the ragged forms.

An item whose predicted durations sum to zero makes the reference's decoder take a softmax over no key (NaN): refused with ValueError."""
from __future__ import annotations

import json
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle
from amphion_amd.models.vc.flow_matching_transformer.llama_nar import _pw
from amphion_amd.modules.hip_ops import (HipConv1d, bucketize_embed_add, expand_path, fs2_durations, layer_norm_c, layer_norm_c_head)
from amphion_amd.modules.transformer.Layers import PostNet
from amphion_amd.modules.transformer.Models import Decoder, Encoder, _get


def get_mask_from_lengths(lengths, max_len=None):
    """[B] lengths -> [B, max_len] bool, True = padded"""
    if max_len is None:
        max_len = int(torch.max(lengths).item())
    ids = torch.arange(0, int(max_len), device=lengths.device)[None, :]
    return ids >= lengths[:, None]


class Conv(nn.Module):
    """Convolution Module: the reference's wrapper, ``conv.weight`` / ``conv.bias``; channel-first here"""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, dilation=1, bias=True, w_init="linear"):
        super().__init__()
        if stride != 1:
            raise NotImplementedError("Conv: stride != 1 is not on the HIP path")
        self.conv = HipConv1d(in_channels, out_channels, kernel_size, padding=padding, dilation=dilation, weight_norm=False, bias=bias)

    def forward_cf(self, x, relu=False):
        return self.conv(x, slope_out=0.0 if relu else 1.0)


class VariancePredictor(nn.Module):
    """Duration, Pitch and Energy Predictor"""

    def __init__(self, cfg):
        super().__init__()
        vp = _get(_get(cfg, "model"), "variance_predictor")
        self.input_size = _get(_get(_get(cfg, "model"), "transformer"), "encoder_hidden")
        self.filter_size = _get(vp, "filter_size")
        self.kernel = _get(vp, "kernel_size")
        self.conv_output_size = self.filter_size
        self.dropout = _get(vp, "dropout")
        self.conv_layer = nn.Sequential(OrderedDict([
            ("conv1d_1", Conv(self.input_size, self.filter_size, kernel_size=self.kernel, padding=(self.kernel - 1) // 2)),
            ("relu_1", nn.ReLU()),
            ("layer_norm_1", nn.LayerNorm(self.filter_size)),
            ("dropout_1", nn.Dropout(self.dropout)),
            ("conv1d_2", Conv(self.filter_size, self.filter_size, kernel_size=self.kernel, padding=1)),
            ("relu_2", nn.ReLU()),
            ("layer_norm_2", nn.LayerNorm(self.filter_size)),
            ("dropout_2", nn.Dropout(self.dropout)),
        ]))
        self.linear_layer = nn.Linear(self.conv_output_size, 1)

    def forward_cf(self, x, lens):
        """x [B, C, T] over the full padded T (padded columns are inputs of the convs, as in the reference) -> [B, T], 0 beyond lens"""
        c = self.conv_layer
        h = c.conv1d_1.forward_cf(x, relu=True)
        h = layer_norm_c(h, c.layer_norm_1.weight.detach(), c.layer_norm_1.bias.detach(), eps=c.layer_norm_1.eps)
        h = c.conv1d_2.forward_cf(h, relu=True)
        if h.shape[2] != x.shape[2]:
            raise NotImplementedError(f"VariancePredictor: kernel_size {self.kernel} with conv1d_2's padding 1 changes the length")
        return layer_norm_c_head(h, c.layer_norm_2.weight, c.layer_norm_2.bias, self.linear_layer.weight, self._head_bias(), lens=lens,
                                 eps=c.layer_norm_2.eps)

    def _head_bias(self):
        """linear_layer.bias as a host float (a kernel argument), read from the device once per value"""
        b = self.linear_layer.bias
        sig = (b.data_ptr(), b._version)
        if getattr(self, "_b0_sig", None) != sig:
            self._b0, self._b0_sig = float(b.detach().item()), sig
        return self._b0

    def forward(self, encoder_output, mask):
        """encoder_output [B, T, C], mask [B, T] True = padded (or None) -> [B, T]"""
        if self.training:
            raise NotImplementedError("VariancePredictor: training mode is not on the HIP path: call .eval()")
        x = _lib.require_device_tensor(encoder_output, "VariancePredictor input").transpose(1, 2).contiguous()
        with _lib.on_device(x.device):
            return self.forward_cf(x, None if mask is None else (~mask).sum(1).to(torch.int32))


class LengthRegulator(nn.Module):
    """Length Regulator: ``amp_expand_path`` along the running sum of the truncated durations"""

    def forward_cf(self, x, cum, src_lens, mel_lens, max_len):
        return expand_path(x, cum, src_lens, mel_lens, int(max_len))[0]

    def forward(self, x, duration, max_len):
        """x [B, T, C], duration [B, T] (each truncated by int(), negatives count 0) -> ([B, max_len or the longest, C], mel_len int64 [B])"""
        x = _lib.require_device_tensor(x, "LengthRegulator input").transpose(1, 2).contiguous()
        n = duration.to(x.device).clamp(min=0).to(torch.int32)
        cum = n.cumsum(1).to(torch.int32).contiguous()
        mel_len = cum[:, -1].contiguous()
        Ty = int(mel_len.max().item()) if max_len is None else int(max_len)
        if Ty < 1:
            raise ValueError("LengthRegulator: every duration is zero")
        with _lib.on_device(x.device):
            out = self.forward_cf(x, cum, None, mel_len.clamp(max=Ty), Ty)
        return out.transpose(1, 2), mel_len.long()


def _read_stats(cfg, sub_dir):
    pre = _get(cfg, "preprocess")
    ds = _get(cfg, "dataset")[0]
    with open(os.path.join(_get(pre, "processed_dir"), ds, sub_dir, "statistics.json")) as f:
        stats = json.load(f)[ds + "_" + ds]
    mean, std = stats["voiced_positions"]["mean"], stats["voiced_positions"]["std"]
    return (stats["total_positions"]["min"] - mean) / std, (stats["total_positions"]["max"] - mean) / std


class VarianceAdaptor(nn.Module):
    """Variance Adaptor.  ``stats``: ``{"pitch": (min, max), "energy": (min, max)}``, the normalised extremes the reference computes from its two
    ``statistics.json`` files -- given, no file is read (the bins are parameters and arrive with the ``state_dict`` anyway)."""

    def __init__(self, cfg, *, stats=None):
        super().__init__()
        pre, model = _get(cfg, "preprocess"), _get(cfg, "model")
        self.duration_predictor = VariancePredictor(cfg)
        self.length_regulator = LengthRegulator()
        self.pitch_predictor = VariancePredictor(cfg)
        self.energy_predictor = VariancePredictor(cfg)
        self.pitch_feature_level = "frame_level" if _get(pre, "use_frame_pitch") else "phoneme_level"
        self.energy_feature_level = "frame_level" if _get(pre, "use_frame_energy") else "phoneme_level"
        ve = _get(model, "variance_embedding")
        n_bins = _get(ve, "n_bins")
        pq, eq = _get(ve, "pitch_quantization"), _get(ve, "energy_quantization")
        assert pq in ["linear", "log"] and eq in ["linear", "log"]
        if stats is None:
            self.energy_dir = _get(pre, "energy_dir") if self.energy_feature_level == "frame_level" else _get(pre, "phone_energy_dir")
            self.pitch_dir = _get(pre, "pitch_dir") if self.pitch_feature_level == "frame_level" else _get(pre, "phone_pitch_dir")
            energy_min, energy_max = _read_stats(cfg, self.energy_dir)
            pitch_min, pitch_max = _read_stats(cfg, self.pitch_dir)
        else:
            (pitch_min, pitch_max), (energy_min, energy_max) = stats["pitch"], stats["energy"]

        def bins(lo, hi, q):
            if q == "log":
                return torch.exp(torch.linspace(np.log(lo), np.log(hi), n_bins - 1))
            return torch.linspace(lo, hi, n_bins - 1)

        self.pitch_bins = nn.Parameter(bins(pitch_min, pitch_max, pq), requires_grad=False)
        self.energy_bins = nn.Parameter(bins(energy_min, energy_max, eq), requires_grad=False)
        hidden = _get(_get(model, "transformer"), "encoder_hidden")
        self.pitch_embedding = nn.Embedding(n_bins, hidden)
        self.energy_embedding = nn.Embedding(n_bins, hidden)

    def _embed(self, which, x, lens, control):
        pred = getattr(self, which + "_predictor").forward_cf(x, lens)
        y, scaled = bucketize_embed_add(x, pred, control, getattr(self, which + "_bins"), getattr(self, which + "_embedding").weight)
        return scaled, y

    def forward_cf(self, x, src_lens, p_control=1.0, e_control=1.0, d_control=1.0, durations=None):
        """x [B, C, Tx] -> (x [B, C, Ty], pitch, energy, log_d, d_rounded, mel_len int32 [B] on the device, Ty).  ``durations`` [B, Tx]:
        given, they take the place of the rounded prediction (everything else is unchanged)"""
        log_d = self.duration_predictor.forward_cf(x, src_lens)
        if self.pitch_feature_level == "phoneme_level":
            p_pred, x = self._embed("pitch", x, src_lens, p_control)
        if self.energy_feature_level == "phoneme_level":
            e_pred, x = self._embed("energy", x, src_lens, e_control)
        if durations is None:
            d_rounded, cum, mel_len = fs2_durations(log_d, d_control)
        else:
            d_rounded = durations.to(device=x.device, dtype=torch.float32)
            cum = d_rounded.clamp(min=0).to(torch.int32).cumsum(1).to(torch.int32).contiguous()
            mel_len = cum[:, -1].contiguous()
        host_len = mel_len.cpu()                                   # the one host read: it sizes the decoder batch
        if int(host_len.min()) < 1:
            raise ValueError(f"FastSpeech2: the predicted durations of item {int(host_len.argmin())} sum to zero frames: the decoder would take a "
                             "softmax over no key")
        Ty = int(host_len.max())
        x = self.length_regulator.forward_cf(x, cum, src_lens, mel_len, Ty)
        if self.pitch_feature_level == "frame_level":
            p_pred, x = self._embed("pitch", x, mel_len, p_control)
        if self.energy_feature_level == "frame_level":
            e_pred, x = self._embed("energy", x, mel_len, e_control)
        return x, p_pred, e_pred, log_d, d_rounded, mel_len, Ty


class FastSpeech2(nn.Module):
    """``FastSpeech2(cfg)`` as the reference; keyword-only ``stats`` (see VarianceAdaptor), ``n_speaker`` (the length of ``spk2id.json``, read
    from the file when None) and ``n_src_vocab`` build it without the dataset's files."""

    def __init__(self, cfg, *, stats=None, n_speaker=None, n_src_vocab=152) -> None:
        super().__init__()
        self.cfg = cfg
        model, pre = _get(cfg, "model"), _get(cfg, "preprocess")
        self.encoder = Encoder(model, n_src_vocab=n_src_vocab)
        self.variance_adaptor = VarianceAdaptor(cfg, stats=stats)
        self.decoder = Decoder(model)
        self.mel_linear = nn.Linear(_get(_get(model, "transformer"), "decoder_hidden"), _get(pre, "n_mel"))
        self.postnet = PostNet(n_mel_channels=_get(pre, "n_mel"))
        self.speaker_emb = None
        if _get(_get(cfg, "train"), "multi_speaker_training"):
            if n_speaker is None:
                with open(os.path.join(_get(pre, "processed_dir"), _get(cfg, "dataset")[0], "spk2id.json"), "r") as f:
                    n_speaker = len(json.load(f))
            self.speaker_emb = nn.Embedding(n_speaker, _get(_get(model, "transformer"), "encoder_hidden"))
        self._mel = _PwHandle()

    def forward(self, data, p_control=1.0, e_control=1.0, d_control=1.0, *, durations=None):
        """``data``: ``texts`` int64 [B, Tx], ``text_len`` [B], ``spk_id`` [B] (multi-speaker models).  Returns the reference's dict, batch-first.
        ``durations`` (keyword-only, [B, Tx]) replaces the rounded prediction: the decoder on known durations."""
        if self.training:
            raise NotImplementedError("FastSpeech2: training mode is not on the HIP path: call .eval()")
        for k in ("target_len", "pitch", "energy", "durations", "mel"):
            if k in data:
                raise NotImplementedError(f"FastSpeech2: '{k}' in data selects the training path (teacher forcing), which is not on the HIP path")
        texts = data["texts"]
        if not isinstance(texts, torch.Tensor) or not texts.is_cuda or texts.dim() != 2:
            raise RuntimeError("FastSpeech2: data['texts'] must be a [B, T] tensor on a ROCm device (the HIP path has no CPU fallback)")
        dev = texts.device
        src_lens = torch.as_tensor(data["text_len"]).to(dev)
        B, Tx = texts.shape
        if src_lens.shape != (B,) or int(src_lens.max()) != Tx or int(src_lens.min()) < 1:
            raise ValueError(f"FastSpeech2: text_len must hold {B} lengths in [1, {Tx}] whose largest is {Tx}, got {src_lens.tolist()}")
        with _lib.on_device(dev):
            src_masks = get_mask_from_lengths(src_lens, Tx)
            lens32 = src_lens.to(torch.int32).contiguous()
            x = self.encoder.forward_cf(texts.long(), (~src_masks).to(torch.uint8).contiguous(), lens32)
            if self.speaker_emb is not None:
                x = x + self.speaker_emb.weight[data["spk_id"].to(dev).long()][:, :, None]     # at padded phones too, as the reference
            x, p_pred, e_pred, log_d, d_rounded, mel_len, Ty = self.variance_adaptor.forward_cf(x, lens32, p_control, e_control, d_control,
                                                                                              durations)
            mel_lens = mel_len.long()
            mel_masks = get_mask_from_lengths(mel_lens, Ty)
            x = self.decoder.forward_cf(x, (~mel_masks).to(torch.uint8).contiguous(), mel_len)
            mel = _pw(self._mel, self.mel_linear, x)
            post = self.postnet.forward_cf(mel, res=mel)
        return {
            "output": mel.transpose(1, 2),
            "postnet_output": post.transpose(1, 2),
            "p_predictions": p_pred,
            "e_predictions": e_pred,
            "log_d_predictions": log_d,
            "d_rounded": d_rounded,
            "src_masks": src_masks,
            "mel_masks": mel_masks,
            "src_lens": src_lens,
            "mel_lens": mel_lens,
        }
