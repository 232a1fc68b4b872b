"""modules/transformer/Models.py on the HIP kernels, eval mode: the Encoder and Decoder of FastSpeech2 / JETS, stacks of FFT blocks behind
a sinusoidal position table.

The table is computed in float64 on the host as the reference does and kept as the ``position_enc`` parameter [1, max_seq_len + 1, C];
in eval mode a sequence longer than ``max_seq_len`` gets a table of its own length computed on the fly, in the Encoder and the Decoder
alike.  The embedding gather is ``amp_embed_sum_c`` (an index outside the vocabulary raises), the table is added by torch from a
transposed copy kept per device: two launches in front of the blocks' seven each.  ``n_src_vocab`` is a keyword (default 152, the
reference's ``len(symbols) + 1``): the text front end is not part of this package."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd.modules.hip_ops import embed_sum_c, embed_sum_check

from .Layers import FFTBlock
from .SubLayers import _eval_only, lens_of_mask

PAD = 0
UNK = 1
BOS = 2
EOS = 3

PAD_WORD = "<blank>"
UNK_WORD = "<unk>"
BOS_WORD = "<s>"
EOS_WORD = "</s>"


def _get(cfg, key):
    """``cfg[key]`` or ``cfg.key``: the reference subscripts ``cfg.model`` in Models.py and uses attributes everywhere else"""
    try:
        return cfg[key]
    except (TypeError, KeyError, IndexError):
        return getattr(cfg, key)


def get_sinusoid_encoding_table(n_position, d_hid, padding_idx=None):
    """Sinusoid position encoding table: float64 on the host, rounded to fp32 once"""
    pos = np.arange(n_position, dtype=np.float64)[:, None]
    hid = np.arange(d_hid)[None, :]
    table = pos / np.power(10000, 2 * (hid // 2) / d_hid)
    table[:, 0::2] = np.sin(table[:, 0::2])
    table[:, 1::2] = np.cos(table[:, 1::2])
    if padding_idx is not None:
        table[padding_idx] = 0.0
    return torch.FloatTensor(table)


class _PosTable:
    """the channel-first [C, T] slice of the position table on the input's device: the parameter's transposed copy (rebuilt when the parameter
    changes) or, beyond ``max_seq_len``, a table of the sequence's own length"""

    def __init__(self):
        self._sig, self._cf, self._long = None, None, {}

    def get(self, param, T, max_seq_len, d_model, device):
        if T > max_seq_len:
            key = (T, str(device))
            t = self._long.get(key)
            if t is None:
                if len(self._long) >= 16:
                    self._long.clear()
                t = self._long[key] = get_sinusoid_encoding_table(T, d_model).t().contiguous().to(device)
            return t
        sig = (param.data_ptr(), param._version, str(device))
        if sig != self._sig:
            self._cf, self._sig = param.detach()[0].t().contiguous().to(device), sig
        return self._cf[:, :T]


class Encoder(nn.Module):
    """Encoder"""

    def __init__(self, config, *, n_src_vocab=152):
        super().__init__()
        tr = _get(config, "transformer")
        n_position = _get(config, "max_seq_len") + 1
        d_model = _get(tr, "encoder_hidden")
        n_head = _get(tr, "encoder_head")
        d_k = d_v = d_model // n_head
        self.max_seq_len = _get(config, "max_seq_len")
        self.d_model = d_model
        self.src_word_emb = nn.Embedding(n_src_vocab, d_model, padding_idx=PAD)
        self.position_enc = nn.Parameter(get_sinusoid_encoding_table(n_position, d_model).unsqueeze(0), requires_grad=False)
        self.layer_stack = nn.ModuleList([FFTBlock(d_model, n_head, d_k, d_v, _get(tr, "conv_filter_size"), _get(tr, "conv_kernel_size"),
                                                   dropout=_get(tr, "encoder_dropout")) for _ in range(_get(tr, "encoder_layer"))])
        self._pos = _PosTable()

    def forward_cf(self, src_seq, key_mask, lens):
        """src_seq int64 [B, T] -> [B, C, T], zero beyond lens"""
        T = src_seq.shape[1]
        x = embed_sum_c(src_seq[None].contiguous(), [self.src_word_emb.weight], None, check=False)
        x = x + self._pos.get(self.position_enc, T, self.max_seq_len, self.d_model, x.device)
        for layer in self.layer_stack:
            x = layer.forward_cf(x, key_mask, lens)
        embed_sum_check(x.device)
        return x

    def forward(self, src_seq, mask, return_attns=False):
        """src_seq [B, T] token ids, mask [B, T] True = padded -> [B, T, C]"""
        _eval_only(self, "Encoder")
        with _lib.on_device(src_seq.device):
            return self.forward_cf(src_seq, (~mask).to(torch.uint8).contiguous(), lens_of_mask(mask)).transpose(1, 2)


class Decoder(nn.Module):
    """Decoder"""

    def __init__(self, config):
        super().__init__()
        tr = _get(config, "transformer")
        n_position = _get(config, "max_seq_len") + 1
        d_model = _get(tr, "decoder_hidden")
        n_head = _get(tr, "decoder_head")
        d_k = d_v = d_model // n_head
        self.max_seq_len = _get(config, "max_seq_len")
        self.d_model = d_model
        self.position_enc = nn.Parameter(get_sinusoid_encoding_table(n_position, d_model).unsqueeze(0), requires_grad=False)
        self.layer_stack = nn.ModuleList([FFTBlock(d_model, n_head, d_k, d_v, _get(tr, "conv_filter_size"), _get(tr, "conv_kernel_size"),
                                                   dropout=_get(tr, "decoder_dropout")) for _ in range(_get(tr, "decoder_layer"))])
        self._pos = _PosTable()

    def forward_cf(self, x, key_mask, lens):
        """x [B, C, T] (zero beyond lens) -> [B, C, T], zero beyond lens"""
        x = x + self._pos.get(self.position_enc, x.shape[2], self.max_seq_len, self.d_model, x.device)
        for layer in self.layer_stack:
            x = layer.forward_cf(x, key_mask, lens)
        return x

    def forward(self, enc_seq, mask, return_attns=False):
        """enc_seq [B, T, C], mask [B, T] True = padded -> ([B, T, C], mask)"""
        _eval_only(self, "Decoder")
        x = _lib.require_device_tensor(enc_seq, "Decoder input").transpose(1, 2).contiguous()
        with _lib.on_device(x.device):
            return self.forward_cf(x, (~mask).to(torch.uint8).contiguous(), lens_of_mask(mask)).transpose(1, 2), mask
