"""SLSTM drop-in (models/codec/speechtokenizer/modules/lstm.py:18-46) on the gfx950 kernels (csrc/lstm.hip), eval mode only.  ``lstm`` is an
``nn.LSTM`` that only HOLDS the parameters under torch's keys (``lstm.weight_ih_l0``, ``lstm.weight_hh_l0_reverse``, ..): it is never called.
The forward is ``amp_lstm_forward`` in the conv layout -- the reference's two permutes never exist, the skip is the last layer's store."""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32_array, param_sig
from amphion_amd._lib import ptr as _p
from amphion_amd.models.codec.amphion_codec.vocos import _check_input, _check_tensors


class SLSTM(nn.Module):
    def __init__(self, dimension: int, num_layers: int = 2, skip: bool = True, bidirectional: bool = False):
        super().__init__()
        self.bidirectional = bidirectional
        self.skip = skip
        self.dimension = dimension
        self.lstm = nn.LSTM(dimension, dimension, num_layers, bidirectional=bidirectional)
        self._cache = HandleCache("amp_lstm_destroy")

    def _handle(self, device):
        return self._cache.get(param_sig(self.lstm.parameters(), str(device), _lib.get_precision()), self._build, device)

    def _build(self, device):
        lstm = self.lstm
        ndir = 2 if self.bidirectional else 1

        def arr(kind):
            return host_f32_array([getattr(lstm, f"{kind}_l{layer}{'_reverse' if d else ''}") for layer in range(lstm.num_layers) for d in range(ndir)])

        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_lstm_create(lstm.input_size, lstm.hidden_size, lstm.num_layers, int(self.bidirectional), int(self.skip),
                                                  arr("weight_ih"), arr("weight_hh"), arr("bias_ih"), arr("bias_hh"), ctypes.byref(h)))
        return h

    def run(self, x):
        B, _, T = x.shape
        dev = x.device
        L = _lib.lib()
        h = self._handle(dev)
        y = torch.empty((B, L.amp_lstm_out_channels(h), T), dtype=torch.float32, device=dev)
        need = L.amp_lstm_workspace_bytes(h, B, T)
        ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
        _lib.check(L.amp_lstm_forward(h, _p(x), B, T, _p(y), _p(ws), need, _lib.current_stream_ptr(dev)))
        return y

    def forward(self, x):
        if self.training:
            raise NotImplementedError("SLSTM: training mode is not on the HIP path (the kernels have no backward): call .eval()")
        x = _check_input(x, self.dimension, "SLSTM")
        _check_tensors(self, x.device, "SLSTM")
        with _lib.on_device(x.device):
            return self.run(x)
