"""CPU-only: ``amphion_amd._handle.HandleCache`` driven by fake builders and a recorded destroy (no handle here is real: ``_lib._destroy`` is
replaced before any finalizer is made), and the modules that own one: a copy or a pickle of a used module carries the same ``state_dict``
and an empty cache."""
import copy
import ctypes
import gc
import os
import pickle
import sys
from types import SimpleNamespace as NS

import pytest
import torch

from amphion_amd import _lib
from amphion_amd._handle import HandleCache, host_f32, host_f32_array, param_sig

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import diffwave_ref  # noqa: E402


@pytest.fixture
def destroyed(monkeypatch):
    """the (entry point, address) pairs that would have gone to the library, in order"""
    log = []
    monkeypatch.setattr(_lib, "_destroy", lambda name, address: log.append((name, address)))
    return log


class Builder:
    """hands out the fake handles 0x1000, 0x2000, .. and counts its calls"""

    def __init__(self):
        self.calls = 0

    def __call__(self, *args):
        self.calls += 1
        return ctypes.c_void_p(0x1000 * self.calls)


def test_hit_returns_the_same_handle_without_building(destroyed):
    c, b = HandleCache("amp_x_destroy"), Builder()
    h = c.get((1, "cuda:0"), b)
    assert h.value == 0x1000 and b.calls == 1
    assert c.get((1, "cuda:0"), b) is h and c.handle is h and b.calls == 1
    assert destroyed == []


def test_changed_signature_destroys_the_old_handle_once_before_the_rebuild(destroyed):
    c, seen = HandleCache("amp_x_destroy"), []

    def build():
        seen.append((list(destroyed), c.handle, c.sig))      # what the builder finds
        return ctypes.c_void_p(0x1000 * len(seen))

    c.get((1,), build)
    h2 = c.get((2,), build)
    assert seen[1] == ([("amp_x_destroy", 0x1000)], None, None)
    assert h2.value == 0x2000 and c.sig == (2,) and destroyed == [("amp_x_destroy", 0x1000)]


def test_failed_build_leaves_the_cache_empty_and_the_old_signature_rebuilds(destroyed):
    """the stale-handle regression: release, failed rebuild, then the OLD signature again must not return the destroyed handle"""
    c, b = HandleCache("amp_x_destroy"), Builder()

    def refuse():
        raise _lib.AmpError(_lib.AMP_ERR_UNSUPPORTED, "refused")

    old = c.get((1, "f16x3"), b)
    with pytest.raises(_lib.AmpError):
        c.get((1, "f32"), refuse)
    assert c.handle is None and c.sig is None and destroyed == [("amp_x_destroy", 0x1000)]
    again = c.get((1, "f16x3"), b)
    assert b.calls == 2 and again is not old and again.value == 0x2000
    assert destroyed == [("amp_x_destroy", 0x1000)]


def test_two_phase_build_that_fails_destroys_the_half_built_handle_once(destroyed):
    c = HandleCache("amp_x_destroy")

    def create_then_fail():
        c.adopt(ctypes.c_void_p(0x5000))
        raise _lib.AmpError(_lib.AMP_ERR_INVALID, "set_weight refused")

    with pytest.raises(_lib.AmpError):
        c.get((1,), create_then_fail)
    assert c.handle is None and c.sig is None and destroyed == [("amp_x_destroy", 0x5000)]
    c.release()
    del c
    gc.collect()
    assert destroyed == [("amp_x_destroy", 0x5000)]


def test_two_phase_build_that_succeeds_keeps_the_adopted_handle(destroyed):
    c = HandleCache("amp_x_destroy")

    def create_then_finish():
        return c.adopt(ctypes.c_void_p(0x5000))

    h = c.get((1,), create_then_finish)
    assert c.get((1,), create_then_finish) is h and destroyed == []
    c.release()
    assert destroyed == [("amp_x_destroy", 0x5000)]


def test_release_twice_destroys_once(destroyed):
    c = HandleCache("amp_x_destroy")
    c.store((1,), ctypes.c_void_p(0x7000))
    c.release()
    c.release()
    assert c.handle is None and c.sig is None and destroyed == [("amp_x_destroy", 0x7000)]


def test_none_is_cached_like_a_handle(destroyed):
    """``HipConv1d._ensure_gated``: "outside the gated kernel" is remembered under its signature"""
    c, calls = HandleCache("amp_x_destroy"), []
    for _ in range(2):
        assert c.get((1,), lambda: calls.append(1)) is None
    assert len(calls) == 1 and c.sig == (1,)
    c.release()
    assert destroyed == []


def test_dropping_the_owner_destroys_once(destroyed):
    class Owner:
        def __init__(self):
            self._cache = HandleCache("amp_x_destroy")

    o = Owner()
    o._cache.store((1,), ctypes.c_void_p(0x9000))
    del o
    gc.collect()
    assert destroyed == [("amp_x_destroy", 0x9000)]


@pytest.mark.parametrize("clone", [copy.deepcopy, lambda c: pickle.loads(pickle.dumps(c))], ids=["deepcopy", "pickle"])
def test_copies_are_empty_and_share_nothing(destroyed, clone):
    c = HandleCache("amp_x_destroy")
    h = c.store((1,), ctypes.c_void_p(0xA000))
    d = clone(c)
    assert type(d) is HandleCache and d.destroy == "amp_x_destroy" and d.handle is None and d.sig is None
    d.store((1,), ctypes.c_void_p(0xB000))
    d.release()
    assert destroyed == [("amp_x_destroy", 0xB000)] and c.handle is h and c.sig == (1,)
    c.release()
    assert destroyed == [("amp_x_destroy", 0xB000), ("amp_x_destroy", 0xA000)] and d.handle is None


def test_staging_helpers():
    w = torch.arange(6, dtype=torch.float64).reshape(2, 3).t()       # not contiguous, not fp32
    b = torch.ones(3, requires_grad=True)
    assert host_f32(None) is None
    h = host_f32(w)
    assert h.dtype == torch.float32 and h.is_contiguous() and torch.equal(h, w.float()) and not host_f32(b).requires_grad
    assert param_sig([w, None, b], "cuda:0", 2) == ((w.data_ptr(), w._version), (b.data_ptr(), b._version), "cuda:0", 2)
    before = param_sig([b])
    with torch.no_grad():
        b.add_(1)
    assert param_sig([b]) != before
    arr = host_f32_array([w, b])
    assert len(arr) == 2 and [t.data_ptr() for t in arr.keep] == list(arr) and torch.equal(arr.keep[0], w.float())


# ---- the owners: a used module copies and pickles, and the copy starts empty --------------------------------------------------------
def _hifigan():
    from amphion_amd.models.vocoders.gan.generator.hifigan import HiFiGAN

    hp = dict(resblock="1", upsample_rates=[4, 4], upsample_kernel_sizes=[8, 8], upsample_initial_channel=32,
              resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 3], [1, 3]])
    return HiFiGAN(NS(preprocess=NS(n_mel=8, hop_size=16), model=NS(hifigan=NS(**hp))))


def _owners():
    from amphion_amd.models.codec.amphion_codec.codec import ResidualUnit, _StridedConv, _TransposedConv
    from amphion_amd.models.codec.coco.rep_coco_model import DownsampleConv1d
    from amphion_amd.models.codec.speechtokenizer.modules.lstm import SLSTM
    from amphion_amd.models.vocoders.diffusion.diffwave.diffwave import DiffWave
    from amphion_amd.modules.hip_ops import HipConv1d

    return {
        "HipConv1d": (lambda: HipConv1d(4, 6, 3, padding=1), "_cache", "amp_conv_destroy"),
        "ResidualUnit": (lambda: ResidualUnit(8, dilation=3), "_cache", "amp_codec_unit_destroy"),
        "_StridedConv": (lambda: _StridedConv(4, 8, 2, 1), "_cache", "amp_sconv_destroy"),
        "_TransposedConv": (lambda: _TransposedConv(8, 4, 2, 1), "_cache", "amp_tconv_destroy"),
        "SLSTM": (lambda: SLSTM(8, num_layers=1), "_cache", "amp_lstm_destroy"),
        "DownsampleConv1d": (lambda: DownsampleConv1d(4, 4), "_cache", "amp_dsconv_destroy"),
        "DiffWave": (lambda: DiffWave(diffwave_ref.make_cfg(**diffwave_ref.SMALL)), "_cache", "amp_dw_destroy"),
        "HiFiGAN": (_hifigan, "_amp_cache", "amp_gen_destroy"),
    }


@pytest.mark.parametrize("clone", [copy.deepcopy, lambda m: pickle.loads(pickle.dumps(m))], ids=["deepcopy", "pickle"])
@pytest.mark.parametrize("name", ["HipConv1d", "ResidualUnit", "_StridedConv", "_TransposedConv", "SLSTM", "DownsampleConv1d", "DiffWave", "HiFiGAN"])
def test_used_module_copies_and_pickles_with_an_empty_cache(destroyed, name, clone):
    make, attr, destroy = _owners()[name]
    m = make()
    cache = getattr(m, attr)
    h = cache.store(("as if built",), ctypes.c_void_p(0xC000))
    m2 = clone(m)
    c2 = getattr(m2, attr)
    assert c2 is not cache and c2.handle is None and c2.sig is None and c2.destroy == cache.destroy
    assert cache.handle is h and destroyed == []
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) and sd[k].data_ptr() != sd2[k].data_ptr() for k in sd)
    if name == "HiFiGAN":
        assert m._amp_handle is h and m2._amp_handle is None
    del m2, c2
    gc.collect()
    assert destroyed == []
    del m, cache
    gc.collect()
    assert destroyed == [(destroy, 0xC000)]


def test_hipconv1d_ensure_hit_and_stale_path_without_a_device(destroyed):
    """the per-launch look-up of ``HipConv1d._ensure`` (spelled out there): a hit does not build; a parameter change releases the
    handle BEFORE the rebuild, so that a refused rebuild leaves nothing to return"""
    from amphion_amd.modules.hip_ops import HipConv1d

    def refuse(device):
        raise _lib.AmpError(_lib.AMP_ERR_UNSUPPORTED, "refused")

    m = HipConv1d(4, 6, 3, padding=1)
    m._build = refuse
    dev = torch.device("cuda", 0)
    h = m._cache.store(m._param_sig() + (dev,), ctypes.c_void_p(0xD000))
    assert m._ensure(dev) is h and m._ensure(torch.device("cuda", 0)) is h
    with torch.no_grad():
        m.bias.add_(1.0)
    with pytest.raises(_lib.AmpError):
        m._ensure(dev)
    assert m._cache.handle is None and m._cache.sig is None and destroyed == [("amp_conv_destroy", 0xD000)]
