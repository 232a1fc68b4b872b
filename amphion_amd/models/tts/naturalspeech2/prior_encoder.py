"""models/tts/naturalspeech2/prior_encoder.py on the HIP kernels, inference only: phone encoder -> duration predictor -> length regulator ->
pitch predictor -> pitch embedding.

    durations     ``amp_fs2_durations`` at control 1 (``clamp(round(exp(x) - 1), min=0)``, their running sum, the frame counts), ONE host read of
                  the frame counts (it sizes everything downstream), ``amp_expand_path`` (zero beyond an item's frames)
    pitch         ``amp_bucketize_embed_add`` on ``exp(pitch_pred_log)``: bucketize, gather and add in one launch, at EVERY frame

As ``NaturalSpeech2.inference`` calls it, there is no phone mask and no frame mask: the predictors, the pitch embedding and everything behind
them run over the zero-padded frames of shorter items, so a batched item differs from the same item run alone, exactly as in the reference.
An item whose predicted durations sum to zero is refused with ValueError."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.modules.hip_ops import bucketize_embed_add, fs2_durations
from amphion_amd.modules.naturalpseech2.transformers import DurationPredictor, LengthRegulator, PitchPredictor, TransformerEncoder, _key_mask


class PriorEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.enc_emb_tokens = nn.Embedding(cfg.vocab_size, cfg.encoder.encoder_hidden, padding_idx=0)
        self.enc_emb_tokens.weight.data.normal_(mean=0.0, std=1e-5)
        self.encoder = TransformerEncoder(enc_emb_tokens=self.enc_emb_tokens, cfg=cfg.encoder)
        self.duration_predictor = DurationPredictor(cfg.duration_predictor)
        self.pitch_predictor = PitchPredictor(cfg.pitch_predictor)
        self.length_regulator = LengthRegulator()
        self.pitch_min, self.pitch_max, self.pitch_bins_num = cfg.pitch_min, cfg.pitch_max, cfg.pitch_bins_num
        pitch_bins = torch.exp(torch.linspace(np.log(self.pitch_min), np.log(self.pitch_max), self.pitch_bins_num - 1))
        self.register_buffer("pitch_bins", pitch_bins)
        self.pitch_embedding = nn.Embedding(self.pitch_bins_num, cfg.encoder.encoder_hidden)

    def forward_cf(self, phone_id, ref_emb, ref_key_mask):
        """phone_id [B, N]; ref_emb [B, d, T'] channel-first (padded frames as the prompt encoder leaves them); ref_key_mask [B, T'] uint8,
        1 = valid -> the reference's dict, ``prior_out`` as a [B, T, d] view of a channel-first tensor"""
        x = self.enc_emb_tokens(phone_id).transpose(1, 2).contiguous()
        cond_mean = torch.mean(ref_emb, dim=2, keepdim=True)                  # over the whole padded prompt, as the reference takes it
        x = self.encoder.forward_cf(x, None, cond_mean)
        log_d = self.duration_predictor.forward_cf(x, ref_emb, ref_key_mask)
        d_rounded, cum, mel_len = fs2_durations(log_d.contiguous(), 1.0)
        host_len = mel_len.cpu()                                              # the one host read
        if int(host_len.min()) < 1:
            raise ValueError(f"PriorEncoder: the predicted durations of item {int(host_len.argmin())} sum to zero frames")
        x = self.length_regulator.forward_cf(x, cum, mel_len, int(host_len.max()))
        pitch_log = self.pitch_predictor.forward_cf(x, ref_emb, ref_key_mask)
        pitch = pitch_log.exp()
        x, _ = bucketize_embed_add(x, pitch, 1.0, self.pitch_bins, self.pitch_embedding.weight)
        return {
            "dur_pred_round": d_rounded.long(),
            "dur_pred_log": log_d,
            "dur_pred": log_d.exp() - 1,
            "pitch_pred_log": pitch_log,
            "pitch_token": torch.bucketize(pitch, self.pitch_bins),
            "mel_len": mel_len.long(),
            "prior_out": x.transpose(1, 2),
        }

    def forward(self, phone_id, duration=None, pitch=None, phone_mask=None, mask=None, ref_emb=None, ref_mask=None, is_inference=False):
        """phone_id [B, N]; ref_emb [B, d, T']; ref_mask [B, T'], 0 = padded.  Inference only: no targets and no masks."""
        if self.training or not is_inference or duration is not None or pitch is not None or phone_mask is not None or mask is not None:
            raise NotImplementedError("PriorEncoder: only the inference path (eval mode, is_inference=True, no targets, no phone / frame mask) is on "
                                      "the HIP path")
        if ref_mask is None:
            raise ValueError("PriorEncoder: ref_mask is required (the reference negates it)")
        ref = _lib.require_device_tensor(ref_emb, "PriorEncoder prompt")
        with _lib.on_device(ref.device):
            return self.forward_cf(phone_id.to(ref.device), ref, _key_mask(ref_mask.to(ref.device)))
