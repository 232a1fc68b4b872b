"""VALL-E (models/tts/valle/valle.py: ``VALLE``), the codec-language-model TTS: text tokens plus an acoustic prompt -> the codes of every
quantizer level.  Eval mode, on the gfx950 kernels.  Same class name, constructor argument (``cfg``), ``state_dict`` keys and ``inference`` /
``continual`` signatures; ``torchmetrics`` is not imported (the accuracy metrics belong to training).

    AR stage     one prefill over [text S | prompt P] under the prefix-LM mask (``amp_prefix_attention``, prefix = S; text and audio positions
                 each from 0 with their own ``alpha``: ``amp_embed_pos``), every column's k and v into per-layer fp32 caches
                 [1, H*64, S + P + 16 S + 2]; then one decode step per token: ``amp_embed_pos`` at T = 1 -> L x ``step_cf``
                 (modules/transformer/transformer.py) -> LN + ``ar_predict_layer`` in one ``amp_pw_forward_vec_ln`` -> ``amp_ar_sample``
                 (temperature, top-k, the multinomial draw as an exponential race) and a greedy ``amp_mask_sample`` for the arg-max of the
                 stop test.  Two ids are read back per step.
    NAR stage    per quantizer level one full-attention forward over [text | audio] (``amp_cross_attention``), the adaptive norms as
                 ``amp_layer_norm_c`` with the stage's host-folded gamma | beta, the level's arg-max a greedy ``amp_mask_sample`` on the
                 predict layer's channel-first output, the running ``y_emb`` an ``amp_embed_sum_c`` with ``init``.

The reference recomputes the whole decoder over [text | audio] for every new token.  Under the prefix-LM mask a text column never depends on
audio and an audio column never on later audio, so the hidden states of earlier columns are what they were: decoding from the caches is the
same function.

Not on the HIP path (``NotImplementedError``): ``forward`` (training), ``add_prenet``, ``norm_first = False``, head dimensions other than 64."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from amphion_amd import _lib
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle
from amphion_amd.models.vc.flow_matching_transformer.llama_nar import _pw
from amphion_amd.modules.encoder import TokenEmbedding
from amphion_amd.modules.hip_ops import (ar_sample, embed_pos, embed_sum_c, embed_sum_check, kv_cache, mask_sample, pw_forward_vec, pw_forward_vec_ln)
from amphion_amd.modules.norms import AdaptiveLayerNorm, LayerNorm
from amphion_amd.modules.transformer.position_embedding import SinePositionalEmbedding
from amphion_amd.modules.transformer.transformer import TransformerEncoder, TransformerEncoderLayer


def _default_noise(device):
    return lambda shape: torch.empty(shape, dtype=torch.float32, device=device).exponential_()


class VALLE(nn.Module):
    def __init__(self, cfg, decoder_cls=TransformerEncoder, decoder_layer_cls=TransformerEncoderLayer):
        super().__init__()
        decoder_dim, nhead = cfg.decoder_dim, cfg.nhead
        nar_scale_factor, num_quantizers, num_decoder_layers = cfg.nar_scale_factor, cfg.num_quantizers, cfg.num_decoder_layers
        nar_decoder_dim, nar_nhead = int(decoder_dim * nar_scale_factor), int(nhead * nar_scale_factor)
        if cfg.add_prenet:
            raise NotImplementedError("VALLE: add_prenet=True is not on the HIP path (the conv / BatchNorm pre-nets of the text and audio embeddings)")
        if not cfg.norm_first:
            raise NotImplementedError("VALLE: norm_first=False (post-norm decoders) is not on the HIP path")
        if decoder_dim % nhead or decoder_dim // nhead != 64 or (num_quantizers > 1 and (nar_nhead < 1 or nar_decoder_dim != 64 * nar_nhead)):
            raise NotImplementedError(f"VALLE: head dimension {decoder_dim}/{nhead} (NAR {nar_decoder_dim}/{nar_nhead}) is not on the HIP path "
                                      "(64: the shipped configs)")
        self.ar_text_embedding = TokenEmbedding(decoder_dim, cfg.text_token_num)
        self.nar_text_embedding = TokenEmbedding(nar_decoder_dim, cfg.text_token_num)
        self.ar_audio_prepend_bos = cfg.prepend_bos
        self.ar_audio_embedding = TokenEmbedding(decoder_dim, cfg.audio_token_num + 1 + int(cfg.prepend_bos))
        self.audio_token_num = cfg.audio_token_num
        self.ar_text_prenet, self.ar_audio_prenet = nn.Identity(), nn.Identity()
        self.ar_text_position = SinePositionalEmbedding(decoder_dim, dropout=0.1, scale=False, alpha=True)
        self.ar_audio_position = SinePositionalEmbedding(decoder_dim, dropout=0.1, scale=False, alpha=True)
        self.ar_decoder = decoder_cls(decoder_layer_cls(decoder_dim, nhead, dim_feedforward=decoder_dim * 4, dropout=0.1, batch_first=True,
                                                        norm_first=cfg.norm_first),
                                      num_layers=num_decoder_layers, norm=LayerNorm(decoder_dim))
        self.ar_predict_layer = nn.Linear(decoder_dim, cfg.audio_token_num + 1, bias=False)
        self.num_heads, self.prefix_mode, self.num_quantizers = nhead, cfg.prefix_mode, num_quantizers
        self._ar_head = _PwHandle()
        assert num_quantizers >= 1
        if num_quantizers > 1:
            self.nar_audio_embeddings = nn.ModuleList([TokenEmbedding(nar_decoder_dim, cfg.audio_token_num + 1)]
                                                      + [TokenEmbedding(nar_decoder_dim, cfg.audio_token_num) for _ in range(num_quantizers - 1)])
            self.nar_text_prenet, self.nar_audio_prenet = nn.Identity(), nn.Identity()
            self.nar_text_position = SinePositionalEmbedding(nar_decoder_dim, dropout=0.0, scale=False, alpha=False)
            self.nar_audio_position = SinePositionalEmbedding(nar_decoder_dim, dropout=0.1, scale=False, alpha=False)
            self.nar_decoder = decoder_cls(decoder_layer_cls(nar_decoder_dim, nar_nhead, dim_feedforward=nar_decoder_dim * 4, dropout=0.1,
                                                             batch_first=True, norm_first=cfg.norm_first, adaptive_layer_norm=True),
                                           num_layers=int(num_decoder_layers * nar_scale_factor),
                                           norm=AdaptiveLayerNorm(nar_decoder_dim, norm=nn.LayerNorm(nar_decoder_dim)))
            self.nar_predict_layers = nn.ModuleList([nn.Linear(nar_decoder_dim, cfg.audio_token_num, bias=False) for _ in range(num_quantizers - 1)])
            self.nar_stage_embeddings = nn.ModuleList([TokenEmbedding(nar_decoder_dim, 1) for _ in range(num_quantizers - 1)])
            if cfg.share_embedding:
                for j in range(0, num_quantizers - 2):
                    self.nar_predict_layers[j].weight = self.nar_audio_embeddings[j + 2].weight
            self._nar_heads = [_PwHandle() for _ in range(num_quantizers - 1)]
        self.eval()

    def forward(self, *args, **kwargs):
        raise NotImplementedError("VALLE.forward is the training step (losses and accuracy metrics), which is not on the HIP path: use inference() / "
                                  "continual()")

    # ---- argument checks
    def _tokens(self, t, name):
        w = self.ar_predict_layer.weight
        if t.dtype.is_floating_point or t.numel() == 0:
            raise ValueError(f"VALLE: {name} must be a non-empty integer tensor")
        if not w.is_cuda:
            raise RuntimeError("VALLE: the kernels run on a ROCm (MI355X) device only; there is no CPU fallback (move the model and its input to 'cuda')")
        if t.device != w.device:
            raise RuntimeError(f"VALLE: {name} is on {t.device} but the parameters are on {w.device}")
        return t.to(torch.int64)

    def _eval_only(self):
        if self.training:
            raise NotImplementedError("VALLE: training mode is not on the HIP path (eval-only scope): call .eval()")

    @staticmethod
    def _embed(tokens, embedding, position, pos0=0):
        """position(embedding(tokens)) channel-first from position ``pos0``; a bad id is reported at the caller's ``embed_sum_check``"""
        w = embedding.weight
        pe = position.table(pos0 + tokens.shape[1], w.device)
        return embed_pos(tokens, w, pe, pos0, position.alpha, position.x_scale, check=False)

    # ---- the AR stage
    def _ar_generate(self, x_tokens, y, n_prompt, top_k, temperature, noise=None, step_logits=None, teacher=None, fused=True):
        """x_tokens [1, S]; y [1, P (+ bos)] -> y with the new tokens appended [1, P (+ bos) + n].  ``n_prompt`` = prompts.shape[1].
        ``fused=False``: the decode step from the launches that existed before ``amp_pw_forward_vec_ln`` (the norm at T = 1, the plain
        matrix-vector product, a separate ReLU) -- what tools/valle_bench.py measures the model's route against; not an option of ``inference``"""
        dev = x_tokens.device
        S, P0 = x_tokens.shape[1], y.shape[1]
        dec, H, C = self.ar_decoder, self.num_heads, self.ar_predict_layer.in_features
        V, EOS = self.ar_predict_layer.out_features, self.audio_token_num
        limit = 16 * S                                              # the reference's cap: more than x_lens.max() * 16 tokens beyond the prompt
        Lmax = S + P0 + limit + 2
        cap = P0 + limit + 2
        k = V if top_k <= 0 else min(max(int(top_k), 1), V)
        noise = _default_noise(dev) if noise is None else noise
        caches = [kv_cache(1, H, C // H, Lmax, dev) for _ in dec.layers]
        ident = (torch.ones((Lmax, C // H // 2), dtype=torch.float32, device=dev), torch.zeros((Lmax, C // H // 2), dtype=torch.float32, device=dev))
        ids = torch.zeros((1, cap), dtype=torch.int64, device=dev)
        ids[:, :P0] = y
        xy = torch.cat([self._embed(x_tokens, self.ar_text_embedding, self.ar_text_position),
                        self._embed(y, self.ar_audio_embedding, self.ar_audio_position)], dim=2)
        embed_sum_check(dev)                                        # a bad text / prompt id; the steps' ids are the sampler's, in [0, V)
        h = dec.forward_cf(xy, prefix=S, caches=caches, ident=ident, final_norm=False)[:, :, -1:].contiguous()
        head = self._ar_head.get(self.ar_predict_layer, dev)
        ng, nb = dec.norm.affine()
        n = P0                                                      # tokens in y so far
        while True:
            if fused:
                logits = pw_forward_vec_ln(head, V, h, ng, nb, dec.norm.eps)
            else:
                logits = pw_forward_vec(head, V, dec.norm.forward_cf(h))
            if step_logits is not None:
                step_logits.append(logits[0, :, 0].clone())
            q = noise((1, V)).to(device=dev, dtype=torch.float32)
            ar_sample(logits, q, ids, n, EOS, False, temperature, k, 1.0, 1.0)
            top, _ = mask_sample(logits, 1)
            if teacher is not None and n - P0 < len(teacher):
                ids[0, n] = int(teacher[n - P0])
            sample, top = torch.cat([ids[0, n:n + 1], top[0]]).tolist()          # the step's one host read: two ids
            if teacher is not None and n - P0 >= len(teacher):
                break
            if teacher is None and (top == EOS or sample == EOS or (n - n_prompt) > limit):
                if n_prompt == n:
                    raise SyntaxError("well trained model shouldn't reach here.")
                break
            n += 1
            x = self._embed(ids[:, n - 1:n], self.ar_audio_embedding, self.ar_audio_position, pos0=n - 1)
            h = dec.step_cf(x, S + n, caches, ident, fused)
        return ids[:, :n].clone()

    # ---- the NAR stage
    def _nar_levels(self, text, text_len, y0, prompts, prefix_len, codes, carry_prompt):
        """text [1, S']; y0 [1, T]: level 0 of prompt + generated frames; prompts [1, P, nq]; appends the arg-max codes [1, T - prefix_len] of
        levels 1 .. nq - 1 to ``codes``.  ``carry_prompt`` (prefix_mode 0): the prompt's own level is added beside each new level; otherwise
        every prompt level is summed in up front."""
        nq, dev = self.num_quantizers, text.device
        emb = self.nar_audio_embeddings
        T = y0.shape[1]
        x = self._embed(text, self.nar_text_embedding, self.nar_text_position)
        pos = self.nar_audio_position
        pos_w = pos.alpha.detach() * pos.table(T, dev)[:T]                      # the rows nar_audio_position adds, as one embedding table
        frames = torch.arange(T, device=dev)[None, None]
        y_emb = embed_sum_c(y0[None], [emb[0].weight], check=False)
        if not carry_prompt and prefix_len > 0:
            head = embed_sum_c(prompts.permute(2, 0, 1)[1:].contiguous(), [emb[j].weight for j in range(1, nq)],
                               init=y_emb[:, :, :prefix_len].contiguous(), check=False)
            y_emb = torch.cat([head, y_emb[:, :, prefix_len:]], dim=2)
        for i in range(nq - 1):
            stage = self.nar_stage_embeddings[i].weight
            y_pos = embed_sum_c(frames, [pos_w], init=y_emb * pos.x_scale if pos.x_scale != 1.0 else y_emb, check=False)
            xy = self.nar_decoder.forward_cf(torch.cat([x, y_pos], dim=2), stage)
            logits = _pw(self._nar_heads[i], self.nar_predict_layers[i], xy[:, :, text_len + prefix_len:].contiguous())
            samples, _ = mask_sample(logits, 1)
            codes.append(samples)
            if i < nq - 2:
                if carry_prompt:
                    new = torch.cat([prompts[:, :prefix_len, i + 1], samples], dim=1)
                    y_emb = embed_sum_c(new[None], [emb[i + 1].weight], init=y_emb, check=False)
                else:
                    tail = embed_sum_c(samples[None], [emb[i + 1].weight], init=y_emb[:, :, prefix_len:].contiguous(), check=False)
                    y_emb = torch.cat([y_emb[:, :, :prefix_len], tail], dim=2)
        embed_sum_check(dev)

    @torch.no_grad()
    def inference(self, x, x_lens, y, enroll_x_lens, top_k=-100, temperature=1.0, *, noise=None, step_logits=None, teacher=None):
        """x [1, S] text tokens, x_lens [1], y [1, T, nq] the acoustic prompt's codes, enroll_x_lens [1] (prefix_mode 2 / 4: the enrolled
        text's length) -> the predicted codes [1, n, nq], as the reference's ``inference`` (valle.py:445-608): the AR stage samples level 0
        until the arg-max or the sample is EOS or more than ``16 * x_lens.max()`` tokens are new, the NAR stage takes the arg-max of levels 1 ..
        ``noise``: a callable ``shape -> Exp(1) tensor`` on the device, one [1, V] row per step (default: ``exponential_()``).
        ``step_logits``: a list that receives every step's logits [V]; ``teacher``: level-0 tokens to force (the AR stage then runs exactly
        ``len(teacher) + 1`` steps)."""
        self._eval_only()
        assert x.ndim == 2, x.shape
        assert x_lens.ndim == 1, x_lens.shape
        assert y.ndim == 3, y.shape
        assert y.shape[0] == 1, y.shape
        assert torch.all(x_lens > 0)
        x, y = self._tokens(x, "x"), self._tokens(y, "y")
        if x.shape[0] != 1 or int(x_lens.max()) != x.shape[1]:
            raise ValueError(f"VALLE.inference: one unpadded sample at a time, as the reference (x {tuple(x.shape)}, x_lens.max() = {int(x_lens.max())})")
        if not temperature > 0:
            raise ValueError(f"VALLE.inference: temperature={temperature} must be strictly positive")
        text, text_len = x, int(x_lens.max())
        prompts, prefix_len = y, y.shape[1]
        bos = int(self.ar_audio_prepend_bos)
        y = prompts[..., 0]
        if bos:
            y = F.pad(y, (1, 0), value=self.audio_token_num + 1)
        with _lib.on_device(x.device):
            y = self._ar_generate(text, y, prompts.shape[1], int(top_k), float(temperature), noise, step_logits, teacher)
            codes = [y[:, prefix_len + bos:]]
            if self.num_quantizers == 1:
                return torch.stack(codes, dim=-1)
            if self.prefix_mode in [2, 4]:
                enrolled_len = int(enroll_x_lens.max().item())
                text = torch.cat([text[:, :1], text[:, enrolled_len - 1:]], dim=1)           # SOS + synthesis text + EOS
                text_len = text_len - (enrolled_len - 2)
                assert text.shape[0] == 1
            self._nar_levels(text, text_len, y[:, bos:], prompts, prefix_len, codes, self.prefix_mode == 0)
        assert len(codes) == self.num_quantizers
        return torch.stack(codes, dim=-1)

    @torch.no_grad()
    def continual(self, x, x_lens, y):
        """x [1, S], x_lens [1], y [1, T, 8] -> [1, T - prefix_len, 8] (valle.py:610-704): the first half of y (at most 225 frames) is the
        prompt, level 0 of the rest is kept and levels 1 .. 7 are predicted by the NAR stage alone"""
        self._eval_only()
        assert x.ndim == 2, x.shape
        assert x_lens.ndim == 1, x_lens.shape
        assert y.ndim == 3, y.shape
        assert y.shape[0] == 1, y.shape
        assert torch.all(x_lens > 0)
        assert self.num_quantizers == 8
        x, y = self._tokens(x, "x"), self._tokens(y, "y")
        if x.shape[0] != 1:
            raise ValueError(f"VALLE.continual: one sample at a time, as the reference (x {tuple(x.shape)})")
        text_len = int(x_lens.max())
        prefix_len = min(int(y.shape[1] * 0.5), 3 * 75)
        prompts = y[:, :prefix_len]
        codes = [y[:, prefix_len:, 0]]
        with _lib.on_device(x.device):
            self._nar_levels(x, text_len, y[..., 0], prompts, prefix_len, codes, self.prefix_mode == 0)
        assert len(codes) == 8
        return torch.stack(codes, dim=-1)
