"""The one cache behind every "packed device copy of these parameters" of the drop-in modules, and the helpers that stage parameters for an
``amp_*_create`` call."""
from __future__ import annotations

import ctypes

import torch

from amphion_amd import _lib


class HandleCache:
    """One ``amp_*`` handle under the signature it was built for.  ``sig`` is None while the cache is empty, so a look-up is one tuple
    comparison: ``get``, or spelled out at a call site, ``c.handle if sig == c.sig else c.build(sig, builder, *args)``.

    The handle is destroyed once -- by ``release``, by a failed build, or when the cache is collected, which is when its owner is.  A copy
    or a pickle of the cache (so of any module that owns one) is a new, empty cache: two objects never share a handle."""

    __slots__ = ("destroy", "handle", "sig", "_fin", "__weakref__")

    def __init__(self, destroy):
        self.destroy = destroy          # name of the entry point that frees the handle ("amp_*_destroy")
        self.handle = self.sig = self._fin = None

    def __deepcopy__(self, memo):
        return HandleCache(self.destroy)

    def __reduce__(self):
        return HandleCache, (self.destroy,)

    def release(self):
        """Destroy the handle and forget it and its signature; does nothing on an empty cache"""
        fin, self.handle, self.sig, self._fin = self._fin, None, None, None
        if fin is not None:
            fin()

    def adopt(self, h):
        """Own ``h`` from here on, in place of whatever was held.  A builder that goes on after its create call (set_weight, finalize,
        set_option) adopts the handle first: if it then raises, ``build`` destroys it."""
        self.release()
        if h is not None:
            self.handle, self._fin = h, _lib.finalizer(self, self.destroy, h)
        return h

    def store(self, sig, h):
        """Hold ``h`` under ``sig``.  ``h`` may be None: "nothing to build for this signature" is cached like a handle."""
        if h is not self.handle:
            self.adopt(h)
        self.sig = sig
        return h

    def build(self, sig, builder, *args):
        """The miss: empty the cache FIRST, then ``store(sig, builder(*args))``.  If the builder raises, the cache stays empty -- the old
        signature can never return the destroyed handle -- and the exception propagates."""
        self.release()
        try:
            return self.store(sig, builder(*args))
        except BaseException:
            self.release()
            raise

    def get(self, sig, builder, *args):
        return self.handle if sig == self.sig else self.build(sig, builder, *args)


def param_sig(tensors, *extra):
    """(address, in-place version) of every tensor that is not None, then ``extra`` (the device, the precision, a count)"""
    return tuple((t.data_ptr(), t._version) for t in tensors if t is not None) + extra


def host_f32(t):
    """a contiguous fp32 host copy of ``t`` for an ``amp_*_create`` call; None stays None"""
    return None if t is None else t.detach().to("cpu", torch.float32).contiguous()


def host_f32_array(tensors):
    """a ``c_void_p`` array of the addresses of ``host_f32`` copies of ``tensors``; the array keeps the copies alive"""
    ts = [host_f32(t) for t in tensors]
    arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    arr.keep = ts
    return arr
