"""FACodec drop-ins (models/codec/ns3_codec/facodec.py:121-1219) on the gfx950 kernels, eval mode only.  Same class names, constructor
arguments, submodule names and ``state_dict`` keys (weight-normed ``weight_g`` / ``weight_v`` or folded ``weight``).

    FACodecEncoder  first conv (1 -> ngf, k = 7)                     implicit-GEMM conv kernel (HipConv1d)
                    per EncoderBlock: 3 x ResidualUnit               amp_aa_unit_forward: ONE fused launch where the policy picks it
                                                                     (csrc/aa_unit_f16x3.hip, C % 32 == 0, C <= 128), else
                                                                     act1d -> conv -> act1d -> conv + residual inside the handle
                                      Activation1d -> strided conv   amp_antialias_snake, amp_sconv_forward(alpha = NULL)
                    Activation1d -> last conv (k = 3)                amp_antialias_snake, HipConv1d
    FACodecDecoder  quantize: prosody, content, residual groups      three launches of amp_fvq_encode_ex; the residual group starts from
                                                                     x - (q_p + q_c) and its stored sum is ``outs``
                    vq2emb                                           amp_fvq_decode_add per group (out-of-range index: AmpError)
                    timbre_encoder -> mean over time                 transformer.py (once per utterance, frame rate)
                    inference: timbre_norm, * gamma + beta           channel LayerNorm kernel, timbre_linear on the conv kernel
                               model: conv (k = 7), per DecoderBlock Activation1d -> amp_tconv_forward(alpha = NULL) -> 3 x ResidualUnit,
                               Activation1d -> conv (k = 7) with tanh on store

    FACodecEncoderV2   FACodecEncoder's block + mel_transform       get_prosody_feature: the mel front-end kernel, one launch (melspec.py)
    FACodecDecoderV2   quantize: the prosody group quantizes        melspec_linear on the pointwise GEMM, melspec_encoder (transformer.py),
                       melspec_encoder(melspec_linear(mel[:20]))     then the three amp_fvq_encode_ex launches of FACodecDecoder
                       inference: timbre_norm, * gamma + beta       ONE amp_layer_norm_c_style launch (style = timbre_linear on the conv kernel)
    FACodecRedecoder   forward / vq2emb: sums of nn.Embedding rows  amp_embed_sum_c, one launch per sum (out-of-range index: AmpError);
                       timbre_cond_prosody_enc                      the conditioned transformer (transformer.py, use_cln=True)
                       inference                                    as FACodecDecoderV2's

Every public forward ends with the op-level range check (``_lib.range_check``): an activation beyond the split-f16 operand range raises ``AmpError``
(AMP_ERR_RANGE) rather than returning a wrong tensor -- re-run under ``_lib.set_precision("f32")`` (AMP_PRECISION=f32), the exact-fp32 route.

The predictor heads (``f0_predictor``, ``phone_predictor``, ``res_f0_predictor``, ``res_phone_predictor``, ``content_f0_predictor``,
``prosody_phone_predictor``, ``x_timbre_predictor`` -- the last alone 63 M parameters) run only in the training branch
``forward(vq=False)``, which raises ``NotImplementedError``.  They are not built: ``load_state_dict`` accepts their keys and discards them,
and ``state_dict()`` omits them; ``FACodecDecoderV2`` treats them the same way."""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.codec import _check_channels, _StridedConv, _TransposedConv
from amphion_amd.models.codec.amphion_codec.vocos import _check_input, _check_tensors
from amphion_amd.models.vocoders.gan.generator._engine import ConvParams
from amphion_amd.modules.activation_functions.snake import SnakeBeta
from amphion_amd.modules.anti_aliasing.act import Activation1d
from amphion_amd.modules.hip_ops import HipConv1d, embed_sum_c, embed_sum_check, layer_norm_c, layer_norm_c_style

from .melspec import MelSpectrogram
from .quantize import ResidualVQ
from .transformer import AMP_PW_BIAS, ConvCache, TransformerEncoder, _PwHandle, pw_forward

PREDICTOR_PREFIXES = ("f0_predictor.", "phone_predictor.", "res_f0_predictor.", "res_phone_predictor.", "content_f0_predictor.",
                      "prosody_phone_predictor.", "x_timbre_predictor.")


def init_weights(m):
    """facodec.py:21-24.  Under weight-norm the reference's draw lands on the derived ``weight`` attribute and leaves g / v as they are."""
    if isinstance(m, ConvParams) and not m.transposed:
        if not m.has_weight_norm:
            nn.init.trunc_normal_(m.weight, std=0.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)


def WNConv1d(*args, **kwargs):
    return HipConv1d(*args, **kwargs)


def _aa(channels):
    return Activation1d(activation=SnakeBeta(channels, alpha_logscale=True))


class ResidualUnit(nn.Module):
    """facodec.py:121-133; ``block`` holds the parameters under the reference's keys, ``forward`` is ``amp_aa_unit_forward``."""

    def __init__(self, dim: int = 16, dilation: int = 1):
        super().__init__()
        pad = ((7 - 1) * dilation) // 2
        self.dim, self.dilation = dim, dilation
        self.block = nn.Sequential(_aa(dim), WNConv1d(dim, dim, 7, dilation=dilation, padding=pad), _aa(dim), WNConv1d(dim, dim, 1))
        self._cache = HandleCache("amp_aa_unit_destroy")

    def _handle(self, device):
        sig = param_sig(list(self.parameters()) + list(self.buffers()), str(device), _lib.get_precision())
        return self._cache.get(sig, self._build, device)

    def _build(self, device):
        a1, c1, a2, c2 = self.block
        beta1 = host_f32(a1.act.beta) if getattr(a1.act, "has_beta", False) else None
        beta2 = host_f32(a2.act.beta) if getattr(a2.act, "has_beta", False) else None
        t = [host_f32(a1.act.alpha), beta1, host_f32(c1.folded_weight()), host_f32(c1.bias), host_f32(a2.act.alpha), beta2,
             host_f32(c2.folded_weight()), host_f32(c2.bias)]
        fu, fd = host_f32(a1.upsample.filter).reshape(-1), host_f32(a1.downsample.lowpass.filter).reshape(-1)
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_aa_unit_create(self.dim, self.dilation, *[_p(v) for v in t], int(a1.act.alpha_logscale), _p(fu), _p(fd),
                                                     ctypes.byref(h)))
        return h

    def fused(self, device):
        return bool(_lib.lib().amp_aa_unit_fused(self._handle(device)))

    def run(self, x, out=None):
        B, C, T = x.shape
        dev = x.device
        L = _lib.lib()
        h = self._handle(dev)
        if out is None:
            out = torch.empty_like(x)
        need = L.amp_aa_unit_workspace_bytes(h, B, T)
        ws = torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None
        _lib.check(L.amp_aa_unit_forward(h, _p(x), B, T, _p(out), _p(ws), need, _lib.current_stream_ptr(dev)))
        return out

    def forward(self, x):
        x = _check_input(x, self.dim, "ResidualUnit")
        _check_tensors(self, x.device, "ResidualUnit")
        with _lib.on_device(x.device):
            return self.run(x)


class EncoderBlock(nn.Module):
    """facodec.py:136-154"""

    def __init__(self, dim: int = 16, stride: int = 1):
        super().__init__()
        self.block = nn.Sequential(ResidualUnit(dim // 2, dilation=1), ResidualUnit(dim // 2, dilation=3), ResidualUnit(dim // 2, dilation=9),
                                   _aa(dim // 2), _StridedConv(dim // 2, dim, stride, stride // 2 + stride % 2))

    def run(self, x):
        for unit in list(self.block)[:3]:
            x = unit.run(x)
        return self.block[4](self.block[3](x))

    def forward(self, x):
        x = _check_input(x, self.block[0].dim, "EncoderBlock")
        _check_tensors(self, x.device, "EncoderBlock")
        with _lib.on_device(x.device):
            return self.run(x)


class FACodecEncoder(nn.Module):
    def __init__(self, ngf=32, up_ratios=(2, 4, 5, 5), out_channels=1024):
        super().__init__()
        self.hop_length = np.prod(up_ratios)
        self.up_ratios = up_ratios
        d_model = ngf
        block = [WNConv1d(1, d_model, 7, padding=3)]
        for stride in up_ratios:
            d_model *= 2
            block += [EncoderBlock(d_model, stride=stride)]
        block += [_aa(d_model), WNConv1d(d_model, out_channels, 3, padding=1)]
        self.block = nn.Sequential(*block)
        self.enc_dim = d_model
        self.n_blocks = len(up_ratios)
        self.reset_parameters()

    def forward(self, x):
        """x [B, 1, T] waveform -> latent [B, out_channels, T']; any T the reference accepts (every strided conv must keep one frame)"""
        who = type(self).__name__
        x = _check_input(x, 1, who)
        dev = x.device
        _check_tensors(self, dev, who)
        with _lib.on_device(dev):
            h = self.block[0](x)
            for i in range(self.n_blocks):
                h = self.block[1 + i].run(h)
            h = self.block[2 + self.n_blocks](self.block[1 + self.n_blocks](h))
        _lib.range_check(dev)
        return h

    def inference(self, x):
        return self.forward(x)

    def reset_parameters(self):
        self.apply(init_weights)


class FACodecEncoderV2(FACodecEncoder):
    """facodec.py:772-845: FACodecEncoder's ``block`` and the mel transform of the prosody feature"""

    def __init__(self, ngf=32, up_ratios=(2, 4, 5, 5), out_channels=1024):
        super().__init__(ngf, up_ratios, out_channels)
        self.mel_transform = MelSpectrogram(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=200, win_size=800, fmin=0, fmax=8000)

    def get_prosody_feature(self, x):
        """x [B, 1, L] waveform -> the first 20 log-mel bands [B, 20, F], F = 1 + (L - 200) // 200"""
        x = _check_input(x, 1, "FACodecEncoderV2.get_prosody_feature")
        return self.mel_transform(x.squeeze(1))[:, :20, :]


class DecoderBlock(nn.Module):
    """facodec.py:220-239"""

    def __init__(self, input_dim: int = 16, output_dim: int = 8, stride: int = 1):
        super().__init__()
        self.input_dim = input_dim
        self.block = nn.Sequential(_aa(input_dim), _TransposedConv(input_dim, output_dim, stride, stride // 2 + stride % 2, stride % 2),
                                   ResidualUnit(output_dim, dilation=1), ResidualUnit(output_dim, dilation=3), ResidualUnit(output_dim, dilation=9))

    def run(self, x):
        x = self.block[1](self.block[0](x))
        for unit in list(self.block)[2:]:
            x = unit.run(x)
        return x

    def forward(self, x):
        x = _check_channels(x, self.input_dim, "DecoderBlock")
        _check_tensors(self, x.device, "DecoderBlock")
        with _lib.on_device(x.device):
            y = self.run(x)
        _lib.range_check(x.device)
        return y


def _decoder_model(in_channels, upsample_initial_channel, up_ratios):
    """conv (k = 7) -> one DecoderBlock per ratio -> Activation1d -> conv (k = 7), tanh on store (facodec.py:361-381,655-672,942-959)"""
    channels = upsample_initial_channel
    layers = [WNConv1d(in_channels, channels, 7, padding=3)]
    output_dim = channels
    for i, stride in enumerate(up_ratios):
        input_dim = channels // 2 ** i
        output_dim = channels // 2 ** (i + 1)
        layers += [DecoderBlock(input_dim, output_dim, stride)]
    layers += [_aa(output_dim), WNConv1d(output_dim, 1, 7, padding=3, tanh=True), nn.Tanh()]
    return nn.Sequential(*layers)              # nn.Tanh holds the reference's module index; the tanh itself is the last conv's store


class _TimbreDecoding(nn.Module):
    """What FACodecDecoder, FACodecDecoderV2 and FACodecRedecoder share past the quantizers: ``model``, ``timbre_linear`` / ``timbre_norm`` and
    the inference that runs them.  The subclass builds the submodules in the reference's order with ``_build_model`` / ``_build_timbre``."""

    def _build_model(self, in_channels, upsample_initial_channel, up_ratios):
        self.model = _decoder_model(in_channels, upsample_initial_channel, up_ratios)
        self.n_blocks = len(up_ratios)

    def _build_timbre(self, in_channels):
        self.timbre_linear = nn.Linear(in_channels, in_channels * 2)
        self.timbre_linear.bias.data[:in_channels] = 1
        self.timbre_linear.bias.data[in_channels:] = 0
        self.timbre_norm = nn.LayerNorm(in_channels, elementwise_affine=False)
        self._style = ConvCache()

    def _check_speaker(self, spk, B, dev, who):
        spk = _lib.require_device_tensor(spk, "speaker_embedding")
        if tuple(spk.shape) != (B, self.in_channels):
            raise ValueError(f"{who}: expected a speaker_embedding {(B, self.in_channels)}, got {tuple(spk.shape)}")
        if spk.device != dev:
            raise RuntimeError(f"{who}: the speaker_embedding is on {spk.device}, the input on {dev}")
        return spk

    def _timbre_style(self, spk):
        """timbre_linear(speaker_embedding) -> [B, 2 d, 1] = gamma | beta"""
        return self._style(self.timbre_linear.weight, self.timbre_linear.bias, spk.unsqueeze(2).contiguous())

    def _run_model(self, h):
        h = self.model[0](h)
        for i in range(self.n_blocks):
            h = self.model[1 + i].run(h)
        return self.model[2 + self.n_blocks](self.model[1 + self.n_blocks](h))

    def _inference_styled(self, x, speaker_embedding):
        """x [B, in_channels, T], speaker_embedding [B, in_channels] -> wave [B, 1, T * hop_length]; timbre_norm and the style in ONE launch"""
        who = type(self).__name__ + ".inference"
        x = _check_channels(x, self.in_channels, who)
        dev = x.device
        _check_tensors(self, dev, type(self).__name__)
        spk = self._check_speaker(speaker_embedding, x.shape[0], dev, who)
        with _lib.on_device(dev):
            h = self._run_model(layer_norm_c_style(x, self._timbre_style(spk), eps=self.timbre_norm.eps))
        _lib.range_check(dev)
        return h

    def reset_parameters(self):
        self.apply(init_weights)


class _FactorizedDecoder(_TimbreDecoding):
    """The constructor FACodecDecoder and FACodecDecoderV2 share (facodec.py:243-404,848-1010): the three quantizer groups, ``model``, the timbre
    path, and the predictor heads' keys accepted and discarded"""

    def __init__(self, in_channels=256, upsample_initial_channel=1536, ngf=32, up_ratios=(5, 5, 4, 2), vq_num_q_c=2, vq_num_q_p=1, vq_num_q_r=3,
                 vq_dim=1024, vq_commit_weight=0.005, vq_weight_init=False, vq_full_commit_loss=False, codebook_dim=8,
                 codebook_size_prosody=10, codebook_size_content=10, codebook_size_residual=10, quantizer_dropout=0.0, dropout_type="linear",
                 use_gr_content_f0=False, use_gr_prosody_phone=False, use_gr_residual_f0=False, use_gr_residual_phone=False,
                 use_gr_x_timbre=False, use_random_mask_residual=True, prob_random_mask_residual=0.75):
        super().__init__()
        self.hop_length = np.prod(up_ratios)
        self.ngf = ngf
        self.up_ratios = up_ratios
        self.in_channels = in_channels
        self.use_random_mask_residual = use_random_mask_residual
        self.prob_random_mask_residual = prob_random_mask_residual
        self.vq_num_q_p, self.vq_num_q_c, self.vq_num_q_r = vq_num_q_p, vq_num_q_c, vq_num_q_r
        self.codebook_size_prosody = codebook_size_prosody
        self.codebook_size_content = codebook_size_content
        self.codebook_size_residual = codebook_size_residual

        def group(n, size):
            return ResidualVQ(num_quantizers=n, dim=vq_dim, codebook_size=size, codebook_dim=codebook_dim, threshold_ema_dead_code=2,
                              commitment=vq_commit_weight, weight_init=vq_weight_init, full_commit_loss=vq_full_commit_loss,
                              quantizer_dropout=quantizer_dropout, dropout_type=dropout_type)

        self.quantizer = nn.ModuleList([group(vq_num_q_p, codebook_size_prosody), group(vq_num_q_c, codebook_size_content)])
        if self.vq_num_q_r > 0:
            self.quantizer.append(group(vq_num_q_r, codebook_size_residual))

        self._build_model(in_channels, upsample_initial_channel, up_ratios)
        self.timbre_encoder = TransformerEncoder(enc_emb_tokens=None, encoder_layer=4, encoder_hidden=256, encoder_head=4, conv_filter_size=1024,
                                                 conv_kernel_size=5, encoder_dropout=0.1, use_cln=False)
        self._build_timbre(in_channels)

        # the flags are kept; the heads they would build run in the training branch only (module docstring)
        self.use_gr_content_f0 = use_gr_content_f0
        self.use_gr_prosody_phone = use_gr_prosody_phone
        self.use_gr_residual_f0 = use_gr_residual_f0
        self.use_gr_residual_phone = use_gr_residual_phone
        self.use_gr_x_timbre = use_gr_x_timbre

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """the predictor heads' keys are accepted and discarded"""
        for k in [k for k in state_dict if k.startswith(prefix) and k[len(prefix):].startswith(PREDICTOR_PREFIXES)]:
            del state_dict[k]
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def _check_latent(self, x, who):
        x = _check_channels(x, self.quantizer[0].layers[0].dim, who)
        _check_tensors(self, x.device, who)
        return x

    def _quantize_groups(self, x_p, x, n_quantizers):
        """the prosody group quantizes x_p, the content group x, the residual group x - (q_p + q_c)"""
        q_p, c_p, _ = self.quantizer[0].encode(x_p, n_quantizers)
        q_c, c_c, _ = self.quantizer[1].encode(x, n_quantizers)
        qs, buf = [c_p, c_c], [q_p, q_c]
        outs = q_p + q_c
        if self.vq_num_q_r > 0:
            outs, c_r, all_r = self.quantizer[2].encode(x, n_quantizers, sub=outs)
            qs.append(c_r)
            buf.append(all_r.sum(0))
        qs = torch.cat(qs, dim=0)
        return outs, qs, torch.zeros(qs.shape[0], device=x.device), buf

    def _vq2emb(self, vq, use_residual):
        """vq [n_p + n_c + n_r, B, T] -> [B, vq_dim, T] (facodec.py:556-566,1179-1189)"""
        self.quantizer.eval()
        p, c = self.vq_num_q_p, self.vq_num_q_c
        out = self.quantizer[0].vq2emb(vq[0:p])
        out = self.quantizer[1].vq2emb(vq[p:p + c], add=out)
        if self.vq_num_q_r > 0 and use_residual:
            out = self.quantizer[2].vq2emb(vq[p + c:], add=out)
        return out

    def _speaker_embedding(self, x):
        return torch.mean(self.timbre_encoder.forward_cf(x.contiguous()), dim=2)


class FACodecDecoder(_FactorizedDecoder):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.register_buffer("_ln_one", torch.ones(self.in_channels), persistent=False)
        self.register_buffer("_ln_zero", torch.zeros(self.in_channels), persistent=False)
        self.reset_parameters()

    def quantize(self, x, n_quantizers=None):
        """facodec.py:408-445 -> (outs, qs [n_p + n_c + n_r, B, T], commit_loss = 0, quantized_buf).  ``n_quantizers`` caps each group."""
        x = self._check_latent(x, "FACodecDecoder.quantize")
        return self._quantize_groups(x, x, n_quantizers)

    def forward(self, x, vq=True, get_vq=False, eval_vq=True, speaker_embedding=None, n_quantizers=None, quantized=None):
        if get_vq:
            return [q.get_emb() for q in self.quantizer]
        if vq is not True:
            raise NotImplementedError("FACodecDecoder.forward(vq=False) is the training branch (predictor heads, random residual masking): not on "
                                      "the HIP path; use inference(x, speaker_embedding)")
        if eval_vq:
            self.quantizer.eval()
        outs, qs, commit_loss, quantized_buf = self.quantize(x, n_quantizers=n_quantizers)
        spk_embs = self._speaker_embedding(x)
        _lib.range_check(x.device)
        return outs, qs, commit_loss, quantized_buf, spk_embs

    def vq2emb(self, vq, use_residual_code=True):
        """vq [n_p + n_c + n_r, B, T] -> [B, vq_dim, T] (facodec.py:556-566)"""
        return self._vq2emb(vq, use_residual_code)

    def inference(self, x, speaker_embedding):
        """x [B, in_channels, T] (the quantized latent), speaker_embedding [B, in_channels] -> wave [B, 1, T * hop_length]"""
        x = _check_channels(x, self.in_channels, "FACodecDecoder.inference")
        dev = x.device
        _check_tensors(self, dev, "FACodecDecoder")
        spk = _lib.require_device_tensor(speaker_embedding, "speaker_embedding")
        if tuple(spk.shape) != (x.shape[0], self.in_channels):
            raise ValueError(f"FACodecDecoder.inference: expected a speaker_embedding {(x.shape[0], self.in_channels)}, got {tuple(spk.shape)}")
        with _lib.on_device(dev):
            gamma, beta = self._timbre_style(spk).chunk(2, 1)
            h = self._run_model(layer_norm_c(x, self._ln_one, self._ln_zero, eps=self.timbre_norm.eps) * gamma + beta)
        _lib.range_check(dev)
        return h


class FACodecDecoderV2(_FactorizedDecoder):
    """facodec.py:848-1219: FACodecDecoder whose prosody group quantizes an encoding of the mel prosody feature instead of the latent"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.melspec_linear = nn.Linear(20, 256)
        self.melspec_encoder = TransformerEncoder(enc_emb_tokens=None, encoder_layer=4, encoder_hidden=256, encoder_head=4, conv_filter_size=1024,
                                                  conv_kernel_size=5, encoder_dropout=0.1, use_cln=False, cfg=None)
        self._mel_in = _PwHandle()
        self.reset_parameters()

    def _check_prosody(self, x, prosody_feature, who):
        p = _lib.require_device_tensor(prosody_feature, "prosody_feature")
        if p.dim() != 3 or p.shape[1] != self.melspec_linear.in_features or p.shape[0] != x.shape[0]:
            raise ValueError(f"{who}: expected a prosody_feature [{x.shape[0]}, {self.melspec_linear.in_features}, T], got {tuple(p.shape)}")
        if p.shape[2] != x.shape[2]:
            raise ValueError(f"{who}: the prosody_feature has {p.shape[2]} frames, the latent {x.shape[2]}")
        if p.device != x.device:
            raise RuntimeError(f"{who}: the prosody_feature is on {p.device}, the latent on {x.device}")
        return p

    def _prosody_latent(self, prosody_feature):
        """prosody_feature [B, 20, T] -> melspec_encoder(melspec_linear(.)) [B, 256, T], what the prosody group quantizes"""
        B, _, T = prosody_feature.shape
        with _lib.on_device(prosody_feature.device):
            h = torch.empty((B, self.melspec_linear.out_features, T), dtype=torch.float32, device=prosody_feature.device)
            pw_forward(self._mel_in, self.melspec_linear, prosody_feature, AMP_PW_BIAS, h)
            return self.melspec_encoder.forward_cf(h)

    def quantize(self, x, prosody_feature, n_quantizers=None):
        """facodec.py:1027-1067 -> (outs, qs [n_p + n_c + n_r, B, T], commit_loss = 0, quantized_buf).  ``n_quantizers`` caps each group."""
        x = self._check_latent(x, "FACodecDecoderV2.quantize")
        p = self._check_prosody(x, prosody_feature, "FACodecDecoderV2.quantize")
        return self._quantize_groups(self._prosody_latent(p), x, n_quantizers)

    def forward(self, x, prosody_feature, vq=True, get_vq=False, eval_vq=True, speaker_embedding=None, n_quantizers=None, quantized=None):
        if get_vq:
            return [q.get_emb() for q in self.quantizer]
        if vq is not True:
            raise NotImplementedError("FACodecDecoderV2.forward(vq=False) is the training branch (predictor heads, random residual masking): not "
                                      "on the HIP path; use inference(x, speaker_embedding)")
        if self.training:
            raise NotImplementedError("FACodecDecoderV2: training mode is not on the HIP path: call .eval()")
        if eval_vq:
            self.quantizer.eval()
        outs, qs, commit_loss, quantized_buf = self.quantize(x, prosody_feature, n_quantizers=n_quantizers)
        spk_embs = self._speaker_embedding(x)
        _lib.range_check(x.device)
        return outs, qs, commit_loss, quantized_buf, spk_embs

    def vq2emb(self, vq, use_residual=True):
        """vq [n_p + n_c + n_r, B, T] -> [B, vq_dim, T] (facodec.py:1179-1189)"""
        return self._vq2emb(vq, use_residual)

    def inference(self, x, speaker_embedding):
        return self._inference_styled(x, speaker_embedding)


class FACodecRedecoder(_TimbreDecoding):
    """facodec.py:602-769: the decoder that re-synthesises from codes alone with another speaker's timbre.  Every group's codes go through
    ``nn.Embedding`` tables of width ``vq_dim``; the prosody stream passes the speaker-conditioned transformer."""

    def __init__(self, in_channels=256, upsample_initial_channel=1280, up_ratios=(5, 5, 4, 2), vq_num_q_c=2, vq_num_q_p=1, vq_num_q_r=3, vq_dim=256,
                 codebook_size_prosody=10, codebook_size_content=10, codebook_size_residual=10):
        super().__init__()
        if vq_dim != 256 or in_channels != 256:
            raise ValueError(f"FACodecRedecoder: the conditioned transformer's width is fixed at 256 (facodec.py:679-689); vq_dim={vq_dim}, "
                             f"in_channels={in_channels} cannot pass through it")
        if vq_num_q_p < 1 or vq_num_q_c < 1 or vq_num_q_r < 0 or max(vq_num_q_p, vq_num_q_c, vq_num_q_r) > 8:
            raise ValueError(f"FACodecRedecoder: {vq_num_q_p} / {vq_num_q_c} / {vq_num_q_r} levels (prosody and content 1..8, residual 0..8)")
        self.hop_length = np.prod(up_ratios)
        self.up_ratios = up_ratios
        self.in_channels = in_channels
        self.vq_num_q_p, self.vq_num_q_c, self.vq_num_q_r = vq_num_q_p, vq_num_q_c, vq_num_q_r
        self.vq_dim = vq_dim
        self.codebook_size_prosody = codebook_size_prosody
        self.codebook_size_content = codebook_size_content
        self.codebook_size_residual = codebook_size_residual

        def tables(n, size):
            embs = nn.ModuleList()
            for _ in range(n):
                emb = nn.Embedding(num_embeddings=2 ** size, embedding_dim=vq_dim)
                emb.weight.data.normal_(mean=0.0, std=1e-5)
                embs.append(emb)
            return embs

        self.prosody_embs = tables(vq_num_q_p, codebook_size_prosody)
        self.content_embs = tables(vq_num_q_c, codebook_size_content)
        self.residual_embs = tables(vq_num_q_r, codebook_size_residual)
        self._build_model(in_channels, upsample_initial_channel, up_ratios)
        self._build_timbre(in_channels)
        self.timbre_cond_prosody_enc = TransformerEncoder(enc_emb_tokens=None, encoder_layer=4, encoder_hidden=256, encoder_head=4,
                                                          conv_filter_size=1024, conv_kernel_size=5, encoder_dropout=0.1, use_cln=True, cfg=None)

    def _check_codes(self, vq, speaker_embedding, n, who):
        if not isinstance(vq, torch.Tensor) or vq.dim() != 3 or vq.shape[0] < n or vq.shape[1] < 1 or vq.shape[2] < 1:
            raise ValueError(f"{who}: expected codes [>= {n}, B, T], got {tuple(vq.shape) if isinstance(vq, torch.Tensor) else type(vq)}")
        if vq.dtype.is_floating_point or vq.dtype == torch.bool:
            raise TypeError(f"{who}: the codes must be integers, got {vq.dtype}")
        if not vq.is_cuda:
            raise RuntimeError(f"{who}: the codes must be a tensor on a ROCm device (there is no CPU fallback)")
        if self.training:
            raise NotImplementedError("FACodecRedecoder: training mode (dropout) is not on the HIP path: call .eval()")
        _check_tensors(self, vq.device, "FACodecRedecoder")
        return self._check_speaker(speaker_embedding, vq.shape[1], vq.device, who)

    @staticmethod
    def _sum(embs, codes, init=None):
        """one launch; the index check is the caller's, once behind all of a call's sums (``embed_sum_check``: it synchronises)"""
        return embed_sum_c(codes, [e.weight for e in embs], init, check=False)

    def _latent(self, vq, spk, use_residual):
        """forward's sum (facodec.py:698-722): x_p + (c_0 + c_1) [+ (r_0 + r_1 + r_2)], the groups summed on their own first"""
        p, c, r = self.vq_num_q_p, self.vq_num_q_c, self.vq_num_q_r
        x = self.timbre_cond_prosody_enc.forward_cf(self._sum(self.prosody_embs, vq[0:p]), spk)
        x = x + self._sum(self.content_embs, vq[p:p + c])
        if use_residual and r > 0:
            x = x + self._sum(self.residual_embs, vq[p + c:p + c + r])
        return x

    def forward(self, vq, speaker_embedding, use_residual_code=False):
        """vq [n_p + n_c (+ n_r), B, T], speaker_embedding [B, 256] -> wave [B, 1, T * hop_length]"""
        n = self.vq_num_q_p + self.vq_num_q_c + (self.vq_num_q_r if use_residual_code else 0)
        spk = self._check_codes(vq, speaker_embedding, n, "FACodecRedecoder.forward")
        dev = vq.device
        with _lib.on_device(dev):
            x = self._latent(vq, spk, use_residual_code)
            h = self._run_model(layer_norm_c_style(x, self._timbre_style(spk), eps=self.timbre_norm.eps))
        embed_sum_check(dev)
        _lib.range_check(dev)
        return h

    def vq2emb(self, vq, speaker_embedding, use_residual=True):
        """-> [B, 256, T] (facodec.py:734-759): the tables added ONE AFTER ANOTHER onto the transformed prosody stream.  The transformer runs
        inside the prosody loop, as the reference's does: once per prosody level"""
        p, c, r = self.vq_num_q_p, self.vq_num_q_c, self.vq_num_q_r if use_residual else 0
        spk = self._check_codes(vq, speaker_embedding, p + c + r, "FACodecRedecoder.vq2emb")
        dev = vq.device
        with _lib.on_device(dev):
            x_t = None
            for i in range(p):
                x_t = self.timbre_cond_prosody_enc.forward_cf(self._sum(self.prosody_embs[i:i + 1], vq[i:i + 1], x_t), spk)
            out = self._sum(list(self.content_embs) + list(self.residual_embs)[:r], vq[p:p + c + r], x_t)
        embed_sum_check(dev)
        _lib.range_check(dev)
        return out

    def inference(self, x, speaker_embedding):
        return self._inference_styled(x, speaker_embedding)
