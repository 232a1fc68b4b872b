"""EuclideanCodebook / VectorQuantization / ResidualVectorQuantization drop-ins
(models/codec/speechtokenizer/modules/quantization/core_vq.py:101-388) in eval mode on the exact-fp32 kernels of csrc/evq.hip.  Same constructor
arguments and ``state_dict`` keys: the codebooks' ``inited`` / ``cluster_size`` / ``embed`` / ``embed_avg`` buffers are kept (only ``embed`` is
read).  All levels of ``ResidualVectorQuantization.forward`` / ``.encode`` are ONE launch (``amp_evq_encode``), ``.decode`` one gather-sum launch
(``amp_evq_decode``, followed by ``amp_evq_check``: an index outside the codebook raises ``AmpError``).

Not on the HIP path (``NotImplementedError``): training mode (EMA updates, dead-code expiry, commitment loss), the k-means initialisation that
the reference runs at the first forward of a codebook whose ``inited`` is 0 -- load a checkpoint first -- and ``codebook_dim != dim``."""
from __future__ import annotations

import ctypes
import typing as tp

import torch
import torch.nn.functional as F
from torch import nn

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32_array, param_sig
from amphion_amd._lib import ptr as _p


def uniform_init(*shape: int):
    t = torch.empty(shape)
    nn.init.kaiming_uniform_(t)
    return t


def _no_training(module, who):
    if module.training:
        raise NotImplementedError(f"{who}: training mode is not on the HIP path (the quantizer kernels have no backward, EMA or k-means): "
                                  "call .eval()")


class EvqHandle:
    """The device copy of a stack of codebooks for ``amp_evq_*``, rebuilt when a codebook or the device changes"""

    def __init__(self):
        self._cache, self._inited = HandleCache("amp_evq_destroy"), None

    def check_inited(self, codebooks):
        """every codebook must hold trained rows; read once per state of the buffers, not per call: reading a device buffer synchronises"""
        sig = tuple((c.inited.data_ptr(), c.inited._version) for c in codebooks)
        if sig != self._inited:
            for c in codebooks:
                c.require_inited()
            self._inited = sig

    def get(self, codebooks, device):
        sig = param_sig([t for c in codebooks for t in (c.embed, c.inited)], str(device), len(codebooks))
        return self._cache.get(sig, self._build, codebooks, device)

    def _build(self, codebooks, device):
        K, D = codebooks[0].embed.shape
        if any(tuple(c.embed.shape) != (K, D) for c in codebooks):
            raise NotImplementedError("ResidualVectorQuantization: levels whose codebooks differ in shape are not on the HIP path")
        arr = host_f32_array([c.embed for c in codebooks])
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().amp_evq_create(D, K, len(codebooks), arr, ctypes.byref(h)))
        return h


def _check_latent(x, D, who):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f"{who}: expected a non-empty [B, {D}, T] tensor, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
    if x.shape[1] != D:
        raise ValueError(f"{who}: expected {D} channels, got {x.shape[1]}")
    return _lib.require_device_tensor(x, f"{who} input")


def evq_encode(handle, codebooks, x, st, n_q, want_sum=True, want_all=False):
    """x [B, D, T] -> (codes int64 [n_q - st, B, T], sum of the levels' rows [B, D, T] or None, every level's rows [n_q - st, B, D, T] or None)"""
    handle.check_inited(codebooks)
    D = codebooks[0].embed.shape[1]
    x = _check_latent(x, D, "quantizer")
    B, _, T = x.shape
    dev = x.device
    h = handle.get(codebooks, dev)
    n = n_q - st
    codes = torch.empty((n, B, T), dtype=torch.int64, device=dev)
    zq = torch.empty((B, D, T), dtype=torch.float32, device=dev) if want_sum else None
    allq = torch.empty((n, B, D, T), dtype=torch.float32, device=dev) if want_all else None
    with _lib.on_device(dev):
        _lib.check(_lib.lib().amp_evq_encode(h, _p(x), B, T, int(st), int(n_q), _p(codes), _p(zq), _p(allq), _lib.current_stream_ptr(dev)))
    return codes, zq, allq


def evq_decode(handle, codebooks, codes, st):
    """codes integers [n, B, T] on the device -> the sum of embed[st + i][codes[i]] [B, D, T]; an index outside a codebook raises ``AmpError``"""
    if not isinstance(codes, torch.Tensor) or codes.dim() != 3 or min(codes.shape) < 1:
        raise ValueError(f"decode: expected codes [n, B, T], got {tuple(codes.shape) if isinstance(codes, torch.Tensor) else type(codes)}")
    if codes.dtype.is_floating_point or codes.dtype == torch.bool:
        raise TypeError(f"decode: the codes must be integers, got {codes.dtype}")
    if not codes.is_cuda:
        raise RuntimeError("decode: the codes must be a tensor on a ROCm device (there is no CPU fallback)")
    n, B, T = codes.shape
    if st < 0 or st + n > len(codebooks):
        raise ValueError(f"decode: {n} levels from level {st} do not fit the {len(codebooks)} quantizers")
    handle.check_inited(codebooks)
    codes = codes.to(torch.int64).contiguous()
    dev = codes.device
    h = handle.get(codebooks, dev)
    out = torch.empty((B, codebooks[0].embed.shape[1], T), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        s = _lib.current_stream_ptr(dev)
        _lib.check(_lib.lib().amp_evq_decode(h, _p(codes), n, int(st), B, T, _p(out), s))
        _lib.check(_lib.lib().amp_evq_check(h, s))
    return out


class EuclideanCodebook(nn.Module):
    def __init__(self, dim: int, codebook_size: int, kmeans_init: int = False, kmeans_iters: int = 10, decay: float = 0.99,
                 epsilon: float = 1e-5, threshold_ema_dead_code: int = 2):
        super().__init__()
        self.decay = decay
        init_fn: tp.Union[tp.Callable[..., torch.Tensor], tp.Any] = uniform_init if not kmeans_init else torch.zeros
        embed = init_fn(codebook_size, dim)
        self.codebook_size = codebook_size
        self.kmeans_iters = kmeans_iters
        self.epsilon = epsilon
        self.threshold_ema_dead_code = threshold_ema_dead_code
        self.register_buffer("inited", torch.Tensor([not kmeans_init]))
        self.register_buffer("cluster_size", torch.zeros(codebook_size))
        self.register_buffer("embed", embed)
        self.register_buffer("embed_avg", embed.clone())
        self._handle = EvqHandle()

    def require_inited(self):
        if not bool(self.inited.item()):
            raise NotImplementedError("EuclideanCodebook: the k-means initialisation of a codebook whose `inited` buffer is 0 is not on the HIP "
                                      "path: load a checkpoint first")

    def encode(self, x):
        """x [..., D] -> indices [...]"""
        _no_training(self, "EuclideanCodebook")
        shape = x.shape
        z = x.reshape(1, -1, shape[-1]).transpose(1, 2).contiguous()
        codes, _, _ = evq_encode(self._handle, [self], z, 0, 1, want_sum=False)
        return codes.view(*shape[:-1])

    def decode(self, embed_ind):
        return F.embedding(embed_ind, self.embed)

    def dequantize(self, embed_ind):
        return self.decode(embed_ind)

    def forward(self, x):
        embed_ind = self.encode(x)
        return self.decode(embed_ind), embed_ind


class VectorQuantization(nn.Module):
    def __init__(self, dim: int, codebook_size: int, codebook_dim: tp.Optional[int] = None, decay: float = 0.99, epsilon: float = 1e-5,
                 kmeans_init: bool = True, kmeans_iters: int = 50, threshold_ema_dead_code: int = 2, commitment_weight: float = 1.0):
        super().__init__()
        _codebook_dim: int = codebook_dim if codebook_dim is not None else dim
        if _codebook_dim != dim:
            raise NotImplementedError("VectorQuantization: codebook_dim != dim (projections around the codebook) is not on the HIP path; "
                                      "SpeechTokenizer quantizes the latent itself")
        self.project_in = nn.Identity()
        self.project_out = nn.Identity()
        self.epsilon = epsilon
        self.commitment_weight = commitment_weight
        self._codebook = EuclideanCodebook(dim=_codebook_dim, codebook_size=codebook_size, kmeans_init=kmeans_init, kmeans_iters=kmeans_iters,
                                           decay=decay, epsilon=epsilon, threshold_ema_dead_code=threshold_ema_dead_code)
        self.codebook_size = codebook_size
        self._handle = EvqHandle()

    @property
    def codebook(self):
        return self._codebook.embed

    def encode(self, x):
        """x [B, D, T] -> indices [B, T]"""
        _no_training(self, "VectorQuantization")
        codes, _, _ = evq_encode(self._handle, [self._codebook], x, 0, 1, want_sum=False)
        return codes[0]

    def decode(self, embed_ind):
        """indices [B, T] -> [B, D, T]"""
        return evq_decode(self._handle, [self._codebook], embed_ind[None], 0)

    def forward(self, x):
        """-> (quantize [B, D, T], indices [B, T], loss [1] = 0)"""
        _no_training(self, "VectorQuantization")
        codes, zq, _ = evq_encode(self._handle, [self._codebook], x, 0, 1)
        return zq, codes[0], torch.zeros(1, device=x.device)


class ResidualVectorQuantization(nn.Module):
    def __init__(self, *, num_quantizers, **kwargs):
        super().__init__()
        self.layers = nn.ModuleList([VectorQuantization(**kwargs) for _ in range(num_quantizers)])
        self._handle = EvqHandle()

    def _codebooks(self):
        return [layer._codebook for layer in self.layers]

    def forward(self, x, n_q: tp.Optional[int] = None, layers: tp.Optional[list] = None):
        """-> (quantized_out [B, D, T], indices [n_q, B, T], losses [n_q, 1] = 0, the quantized of the levels in ``layers``)"""
        _no_training(self, "ResidualVectorQuantization")
        n_q = n_q or len(self.layers)
        codes, zq, allq = evq_encode(self._handle, self._codebooks(), x, 0, min(n_q, len(self.layers)), want_all=bool(layers))
        out_quantized = [allq[i] for i in range(codes.shape[0]) if layers and i in layers]
        return zq, codes, torch.zeros((codes.shape[0], 1), device=x.device), out_quantized

    def encode(self, x: torch.Tensor, n_q: tp.Optional[int] = None, st: tp.Optional[int] = None) -> torch.Tensor:
        """-> indices [n_q - st, B, T].  As in the reference, with st > 0 level st quantizes the WHOLE input (core_vq.py:370-378)."""
        _no_training(self, "ResidualVectorQuantization")
        n_q = n_q or len(self.layers)
        st = st or 0
        n_q = min(n_q, len(self.layers))
        if st >= n_q:
            raise ValueError(f"ResidualVectorQuantization.encode: st={st} leaves no level below n_q={n_q}")
        codes, _, _ = evq_encode(self._handle, self._codebooks(), x, st, n_q, want_sum=False)
        return codes

    def decode(self, q_indices: torch.Tensor, st: int = 0) -> torch.Tensor:
        return evq_decode(self._handle, self._codebooks(), q_indices, st)
