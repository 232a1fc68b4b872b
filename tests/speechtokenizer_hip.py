"""ctypes helpers of the SpeechTokenizer GPU tests: handles and calls of amp_elu_pad / amp_lstm_* / amp_evq_* on torch tensors."""
import ctypes

import torch

from amphion_amd import _lib
from amphion_amd._lib import ptr as _p

DEV = "cuda:0"


def _stream():
    return _lib.current_stream_ptr(torch.device(DEV))


def _arr(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def elu_pad(x, pl, pr, elu, alpha=1.0):
    B, C, T = x.shape
    y = torch.full((B, C, T + pl + pr), float("nan"), device=x.device)
    _lib.check(_lib.lib().amp_elu_pad(_p(x), B, C, T, pl, pr, int(elu), float(alpha), _p(y), _stream()))
    return y


class Lstm:
    """w_ih / w_hh / b_ih / b_hh: lists of host tensors in nn.LSTM's order (l0, l0_reverse, l1, ..)"""

    def __init__(self, In, H, layers, bidir, skip, w_ih, w_hh, b_ih, b_hh):
        keep = [[t.detach().float().contiguous() for t in ts] for ts in (w_ih, w_hh, b_ih, b_hh)]
        self.h = ctypes.c_void_p()
        self.H, self.ndir = H, 2 if bidir else 1
        _lib.check(_lib.lib().amp_lstm_create(In, H, layers, int(bidir), int(skip), *[_arr(k) for k in keep], ctypes.byref(self.h)))
        self._fin = _lib.finalizer(self, "amp_lstm_destroy", self.h)

    def _ws(self, B, T):
        need = _lib.lib().amp_lstm_workspace_bytes(self.h, B, T)
        # NaN-filled: step 0 must not read the state
        return torch.full((need // 4,), float("nan"), device=DEV), need

    def recur(self, layer, gx, skip=None):
        B, _, T = gx.shape
        y = torch.full((B, self.ndir * self.H, T), float("nan"), device=DEV)
        ws, _ = self._ws(B, T)
        _lib.check(_lib.lib().amp_lstm_recur(self.h, layer, _p(gx), B, T, _p(skip), _p(y), _p(ws), _stream()))
        return y

    def forward(self, x):
        B, _, T = x.shape
        y = torch.full((B, _lib.lib().amp_lstm_out_channels(self.h), T), float("nan"), device=DEV)
        ws, need = self._ws(B, T)
        _lib.check(_lib.lib().amp_lstm_forward(self.h, _p(x), B, T, _p(y), _p(ws), need, _stream()))
        return y


class Evq:
    def __init__(self, cbs):
        keep = [c.detach().float().contiguous() for c in cbs]
        self.K, self.D = keep[0].shape
        self.h = ctypes.c_void_p()
        _lib.check(_lib.lib().amp_evq_create(self.D, self.K, len(keep), _arr(keep), ctypes.byref(self.h)))
        self._fin = _lib.finalizer(self, "amp_evq_destroy", self.h)

    def encode(self, z, st, n_q):
        B, D, T = z.shape
        n = n_q - st
        codes = torch.full((n, B, T), -7, dtype=torch.int64, device=DEV)
        zq = torch.full((B, D, T), float("nan"), device=DEV)
        allq = torch.full((n, B, D, T), float("nan"), device=DEV)
        _lib.check(_lib.lib().amp_evq_encode(self.h, _p(z), B, T, st, n_q, _p(codes), _p(zq), _p(allq), _stream()))
        return codes, zq, allq

    def decode(self, codes, st):
        n, B, T = codes.shape
        out = torch.full((B, self.D, T), float("nan"), device=DEV)
        _lib.check(_lib.lib().amp_evq_decode(self.h, _p(codes.contiguous()), n, st, B, T, _p(out), _stream()))
        return out

    def check(self):
        return _lib.lib().amp_evq_check(self.h, _stream())
