"""Vevo's autoregressive transformer (models/vc/autoregressive_transformer/ar_model.py: ``AutoregressiveTransformer``), the stage between the
tokenizers and the flow-matching transformer: content or phone tokens plus a content-style prompt -> content-style tokens.  Eval mode, on the
gfx950 kernels.  Same class name, constructor arguments, special-token ids, ``state_dict`` keys (``model.model.*``, ``model.lm_head.weight``)
and ``forward`` / ``generate`` signatures; plain ``nn.Module``s hold the parameters (``transformers`` is not imported) and ``load_state_dict``
drops the ``*.rotary_emb.inv_freq`` buffers of older checkpoints.

    prefill (``forward``, and ``generate``'s prompt)   channel-first [B, C, T]: ``amp_pw_forward`` Linears (q | k | v and gate | up stacked, o_proj
                                                       and down_proj add the residual in their epilogue), ``amp_rms_norm_c_adaptive`` with the
                                                       weight's batch stride 0 as LlamaRMSNorm, ``amp_rope_attention_causal`` with the padding
                                                       mask as key mask, ``amp_swiglu``; ``generate`` then fills the KV caches with one
                                                       ``amp_kv_append`` per layer and takes the logits of the last column only
    decode step (one column)                           embed -> L x (norm, q | k | v ``amp_pw_forward_vec``, ``amp_kv_append``, ``amp_attention_decode``,
                                                       o_proj vec + residual, norm, gate | up vec, ``amp_swiglu``, down_proj vec + residual) ->
                                                       norm -> lm_head vec -> ``amp_ar_sample`` (HF's repetition penalty, EOS suppression,
                                                       temperature, top-k, top-p and the multinomial draw as an exponential race)

``generate`` reads the drawn token back once per step for the EOS test.  Not on the HIP path (``NotImplementedError``): the global style
encoder (no shipped config enables it), head dimensions other than 64 / 96, training mode, ``generate`` for more than one sample."""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from amphion_amd import _lib
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle
from amphion_amd.models.vc.flow_matching_transformer.llama_nar import (LlamaAttention, LlamaMLP, _drop_inv_freq, _gamma_one, _pw, _Stacked)
from amphion_amd.modules.hip_ops import (ar_sample, attention_decode, kv_append, kv_cache, pw_forward_vec, rope_attention, rope_tables, swiglu)

RMS_EPS = 1e-6        # LlamaConfig.rms_norm_eps' default, which the reference never overrides


class LlamaRMSNorm(nn.Module):
    """HF's LlamaRMSNorm: ``weight * x * rsqrt(mean(x^2) + eps)`` over the channel axis of [B, C, T]"""

    def __init__(self, hidden_size, eps=RMS_EPS):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward_cf(self, x):
        B, C, T = x.shape
        y = torch.empty_like(x)
        _lib.check(_lib.lib().amp_rms_norm_c_adaptive(_p(x), _p(self.weight), 0, B, C, T, float(self.variance_epsilon), _p(y),
                                                      _lib.current_stream_ptr(x.device)))
        return y


class LlamaDecoderLayer(nn.Module):
    def __init__(self, hidden_size, intermediate_size, num_heads):
        super().__init__()
        self.self_attn = LlamaAttention(hidden_size, num_heads)
        self.mlp = LlamaMLP(hidden_size, intermediate_size)
        self.input_layernorm = LlamaRMSNorm(hidden_size)
        self.post_attention_layernorm = LlamaRMSNorm(hidden_size)

    def _stacked(self):
        a, m = self.self_attn, self.mlp
        return _Stacked((a.q_proj, a.k_proj, a.v_proj)), _Stacked((m.gate_proj, m.up_proj))

    def prefill_cf(self, x, cos, sin, key_mask, cache=None):
        """x [B, C, T] -> the layer's output; ``cache`` (kcache, vcache): filled with the T columns at positions 0 .. T - 1"""
        a, m = self.self_attn, self.mlp
        C = a.hidden_size
        qkv_l, gu_l = self._stacked()
        qkv = _pw(a._qkv, qkv_l, self.input_layernorm.forward_cf(x))
        if cache is not None:
            kv_append(qkv[:, C:2 * C], qkv[:, 2 * C:], a.num_heads, cos, sin, 0, cache[0], cache[1])
        att = rope_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], a.num_heads, cos[:x.shape[2]], sin[:x.shape[2]], key_mask, causal=True)
        x = _pw(a._out, a.o_proj, att, res=x)
        return _pw(m._down, m.down_proj, swiglu(_pw(m._gu, gu_l, self.post_attention_layernorm.forward_cf(x))), res=x)

    def step_cf(self, x, cos, sin, L, cache):
        """x [B, C, 1], the column at position L - 1 -> the layer's output; the column's k / v are appended to the cache first"""
        a, m = self.self_attn, self.mlp
        C, dev = a.hidden_size, x.device
        qkv_l, gu_l = self._stacked()
        qkv = pw_forward_vec(a._qkv.get(qkv_l, dev), 3 * C, self.input_layernorm.forward_cf(x))
        kv_append(qkv[:, C:2 * C], qkv[:, 2 * C:], a.num_heads, cos, sin, L - 1, cache[0], cache[1])
        att = attention_decode(qkv[:, :C], a.num_heads, cos, sin, L, cache[0], cache[1])
        x = pw_forward_vec(a._out.get(a.o_proj, dev), C, att, gamma=_gamma_one(C, dev), res=x)
        gu = pw_forward_vec(m._gu.get(gu_l, dev), gu_l.out_features, self.post_attention_layernorm.forward_cf(x))
        return pw_forward_vec(m._down.get(m.down_proj, dev), C, swiglu(gu), gamma=_gamma_one(C, dev), res=x)


class LlamaModel(nn.Module):
    def __init__(self, vocab_size, hidden_size, intermediate_size, num_layers, num_heads, pad_token_id):
        super().__init__()
        self.embed_tokens = nn.Embedding(vocab_size, hidden_size, padding_idx=pad_token_id)
        self.layers = nn.ModuleList([LlamaDecoderLayer(hidden_size, intermediate_size, num_heads) for _ in range(num_layers)])
        self.norm = LlamaRMSNorm(hidden_size)


class LlamaForCausalLM(nn.Module):
    """the parameter tree of HF's class (``model.*``, ``lm_head.weight``) with its initialisation: normal(0, 0.02), a zero padding row"""

    def __init__(self, vocab_size, hidden_size, intermediate_size, num_layers, num_heads, pad_token_id):
        super().__init__()
        self.model = LlamaModel(vocab_size, hidden_size, intermediate_size, num_layers, num_heads, pad_token_id)
        self.lm_head = nn.Linear(hidden_size, vocab_size, bias=False)
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                m.weight.data.normal_(mean=0.0, std=0.02)
        self.model.embed_tokens.weight.data[pad_token_id].zero_()
        self._head = _PwHandle()


class CausalLMOutput(SimpleNamespace):
    """what ``forward`` returns: ``.logits`` [B, T, V] and ``.loss``"""


def _default_noise(device):
    return lambda shape: torch.empty(shape, dtype=torch.float32, device=device).exponential_()


class AutoregressiveTransformer(nn.Module):
    def __init__(self, input_vocab_size=1056, output_vocab_size=8192, hidden_size=1024, intermediate_size=4096, num_hidden_layers=12,
                 num_attention_heads=16, use_global_style_encoder=False, cfg=None):
        super().__init__()
        if cfg is not None:
            self.cfg = cfg
            input_vocab_size, output_vocab_size, hidden_size = cfg.input_vocab_size, cfg.output_vocab_size, cfg.hidden_size
            intermediate_size, num_hidden_layers, num_attention_heads = cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads
            use_global_style_encoder = cfg.use_global_style_encoder
        self.input_vocab_size, self.output_vocab_size, self.hidden_size = input_vocab_size, output_vocab_size, hidden_size
        self.intermediate_size, self.num_hidden_layers, self.num_attention_heads = intermediate_size, num_hidden_layers, num_attention_heads
        self.use_global_style_encoder = use_global_style_encoder
        if use_global_style_encoder:
            raise NotImplementedError("AutoregressiveTransformer: use_global_style_encoder=True is not on the HIP path (GlobalEncoder leans on "
                                      "HF internals and a random permutation; no shipped config enables it)")
        if hidden_size % num_attention_heads or hidden_size // num_attention_heads not in (64, 96):
            raise NotImplementedError(f"AutoregressiveTransformer: head dimension {hidden_size}/{num_attention_heads} is not on the HIP path "
                                      "(64 or 96: the shipped configs)")
        # five special tokens: pad, bos, eos for both input and output
        self.pad_token_id = input_vocab_size + output_vocab_size
        self.input_bos_token_id = self.pad_token_id + 1
        self.input_eos_token_id = self.pad_token_id + 2
        self.output_bos_token_id = self.pad_token_id + 3
        self.output_eos_token_id = self.pad_token_id + 4
        self.no_loss_label = -100
        vocab = input_vocab_size + output_vocab_size + 20        # 20 is for other special tokens during post-training
        self.config = SimpleNamespace(vocab_size=vocab, hidden_size=hidden_size, intermediate_size=intermediate_size,
                                      num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads, pad_token_id=self.pad_token_id,
                                      bos_token_id=self.output_bos_token_id, eos_token_id=self.output_eos_token_id, rms_norm_eps=RMS_EPS,
                                      rope_theta=10000.0, max_position_embeddings=2048)
        self.model = LlamaForCausalLM(vocab, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, self.pad_token_id)
        self._register_load_state_dict_pre_hook(_drop_inv_freq)

    # ---- the reference's padding, integer torch ops (ar_model.py:174-235)
    def padding_for_input(self, input_ids, input_mask, eos_id, bos_id, pad_id):
        input_ids = (input_ids + self.output_vocab_size) * input_mask
        input_ids = F.pad(input_ids, (0, 1), value=0) + eos_id * F.pad(1 - input_mask, (0, 1), value=1)
        input_mask = F.pad(input_mask, (1, 0), value=1)
        input_ids = input_ids * input_mask + pad_id * (1 - input_mask)
        input_ids = F.pad(input_ids, (1, 0), value=bos_id)
        input_mask = F.pad(input_mask, (1, 0), value=1)
        input_label = self.no_loss_label * torch.ones_like(input_ids)
        return input_ids.long(), input_mask.long(), input_label.long()

    def padding_for_output(self, output_ids, output_mask, eos_id, bos_id, pad_id):
        output_ids = output_ids * output_mask
        output_ids = F.pad(output_ids, (0, 1), value=0) + eos_id * F.pad(1 - output_mask, (0, 1), value=1)
        output_mask = F.pad(output_mask, (1, 0), value=1)
        output_ids = output_ids * output_mask + pad_id * (1 - output_mask)
        output_ids = F.pad(output_ids, (1, 0), value=bos_id)
        output_mask = F.pad(output_mask, (1, 0), value=1)
        output_label = output_ids * output_mask + self.no_loss_label * (1 - output_mask)
        return output_ids.long(), output_mask.long(), output_label.long()

    # ---- the launches
    def _ids(self, t, name):
        w = self.model.lm_head.weight
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.numel() == 0 or t.dtype.is_floating_point:
            raise ValueError(f"AutoregressiveTransformer: {name} must be a non-empty integer [B, T] tensor")
        if not w.is_cuda:
            raise RuntimeError("AutoregressiveTransformer: the kernels run on a ROCm (MI355X) device only; there is no CPU fallback (move the model "
                               "and its input to 'cuda')")
        if t.device != w.device:
            raise RuntimeError(f"AutoregressiveTransformer: {name} is on {t.device} but the parameters are on {w.device}")
        return t

    def _eval_only(self):
        if self.training:
            raise NotImplementedError("AutoregressiveTransformer: training mode is not on the HIP path (eval-only scope): call .eval()")

    def _prefill(self, ids, key_mask, caches=None, Lmax=None):
        """ids [B, T] -> the final norm's output [B, C, T]"""
        lm = self.model.model
        B, T = ids.shape
        cos, sin = rope_tables(Lmax or T, self.hidden_size // self.num_attention_heads, ids.device)
        x = lm.embed_tokens(ids).detach().transpose(1, 2).contiguous()
        for i, layer in enumerate(lm.layers):
            x = layer.prefill_cf(x, cos, sin, key_mask, None if caches is None else caches[i])
        return lm.norm.forward_cf(x)

    def _head_vec(self, h):
        """h [B, C, 1] -> logits [B, V, 1]"""
        head = self.model.lm_head
        return pw_forward_vec(self.model._head.get(head, h.device), head.out_features, h)

    @torch.no_grad()
    def forward(self, input_ids, input_mask, output_ids, output_mask, mels=None, mels_mask=None):
        """input_ids / input_mask [B, T1], output_ids / output_mask [B, T2] (masks: 1 = valid) -> ``.logits`` [B, T1 + T2 + 4, V], ``.loss``
        (HF's shifted cross-entropy over the output labels, in torch)"""
        self._eval_only()
        if mels is not None or mels_mask is not None:
            raise NotImplementedError("AutoregressiveTransformer: mels are the global style encoder's input, which is not on the HIP path")
        input_ids, output_ids = self._ids(input_ids, "input_ids"), self._ids(output_ids, "output_ids")
        input_mask, output_mask = self._ids(input_mask, "input_mask"), self._ids(output_mask, "output_mask")
        input_ids, input_mask, input_label = self.padding_for_input(input_ids, input_mask, self.input_eos_token_id, self.input_bos_token_id,
                                                                    self.pad_token_id)
        output_ids, output_mask, output_label = self.padding_for_output(output_ids, output_mask, self.output_eos_token_id,
                                                                        self.output_bos_token_id, self.pad_token_id)
        ids = torch.cat([input_ids, output_ids], dim=-1)
        mask = torch.cat([input_mask, output_mask], dim=-1)
        labels = torch.cat([input_label, output_label], dim=-1)
        with _lib.on_device(ids.device):
            h = self._prefill(ids, (mask != 0).to(torch.uint8))
            logits = _pw(self.model._head, self.model.lm_head, h).transpose(1, 2).contiguous()
        V = logits.shape[-1]
        loss = F.cross_entropy(logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=self.no_loss_label)
        return CausalLMOutput(logits=logits, loss=loss)

    @torch.no_grad()
    def generate(self, input_ids, prompt_mels=None, prompt_output_ids=None, max_length=2000, temperature=0.8, top_k=50, top_p=0.9,
                 repeat_penalty=1.0, min_new_tokens=50, *, noise=None, step_logits=None, teacher=None):
        """One sample: input_ids [1, T], prompt_output_ids [1, T'] -> the new content-style tokens [1, n], as the reference's ``generate``
        around HF's sampling loop: it stops on EOS or at ``max_length`` counted over prompt + new tokens, then strips BOS / EOS.
        ``noise``: a callable ``shape -> Exp(1) tensor`` on the device, one [1, V] row per step (default: ``exponential_()``).
        ``step_logits``: a list that receives every step's logits [V]; ``teacher``: tokens to force (for tests that compare steps)."""
        self._eval_only()
        if prompt_output_ids is None:
            raise ValueError("AutoregressiveTransformer.generate: prompt_output_ids is required without the global style encoder")
        for t in (input_ids, prompt_output_ids):
            if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] != 1:
                raise NotImplementedError("AutoregressiveTransformer.generate: one sample at a time, as the reference (B = 1)")
        input_ids, prompt_output_ids = self._ids(input_ids, "input_ids"), self._ids(prompt_output_ids, "prompt_output_ids")
        dev = input_ids.device
        input_ids, _, _ = self.padding_for_input(input_ids, torch.ones_like(input_ids), self.input_eos_token_id, self.input_bos_token_id,
                                                 self.pad_token_id)
        prompt, _, _ = self.padding_for_output(prompt_output_ids, torch.ones_like(prompt_output_ids), self.output_eos_token_id,
                                               self.output_bos_token_id, self.pad_token_id)
        prompt_ids = torch.cat([input_ids, prompt[:, :-1]], dim=-1)          # without the prompt's eos token
        n0, max_length = prompt_ids.shape[1], int(max_length)
        if n0 >= max_length:
            raise ValueError(f"AutoregressiveTransformer.generate: the prompt has {n0} tokens, max_length = {max_length} leaves none to generate")
        V, H, C = self.config.vocab_size, self.num_attention_heads, self.hidden_size
        top_k = V if not top_k else int(top_k)
        top_p = 1.0 if top_p is None else float(top_p)
        noise = _default_noise(dev) if noise is None else noise
        lm = self.model.model
        with _lib.on_device(dev):
            caches = [kv_cache(1, H, C // H, max_length, dev) for _ in lm.layers]
            cos, sin = rope_tables(max_length, C // H, dev)
            ids = torch.zeros((1, max_length), dtype=torch.int64, device=dev)
            ids[:, :n0] = prompt_ids
            h = self._prefill(prompt_ids, None, caches, max_length)[:, :, -1:].contiguous()
            n = n0
            while True:
                logits = self._head_vec(h)
                if step_logits is not None:
                    step_logits.append(logits[0, :, 0].clone())
                q = noise((1, V)).to(device=dev, dtype=torch.float32)
                ar_sample(logits, q, ids, n, self.output_eos_token_id, n - n0 < min_new_tokens, temperature, top_k, top_p, repeat_penalty)
                if teacher is not None:
                    ids[0, n] = int(teacher[n - n0])
                tok = int(ids[0, n])                                          # the step's one host read
                n += 1
                if tok == self.output_eos_token_id or n >= max_length:
                    break
                x = lm.embed_tokens(ids[:, n - 1:n]).detach().transpose(1, 2).contiguous()
                for layer, cache in zip(lm.layers, caches):
                    x = layer.step_cf(x, cos, sin, n, cache)
                h = lm.norm.forward_cf(x)
        gen_tokens = ids[:, n0:n].clone()
        if gen_tokens[:, 0] == self.output_bos_token_id:
            gen_tokens = gen_tokens[:, 1:]
        if gen_tokens[:, -1] == self.output_eos_token_id:
            gen_tokens = gen_tokens[:, :-1]
        return gen_tokens
