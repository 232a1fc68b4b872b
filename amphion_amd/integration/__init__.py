"""Run the reference's own entry points on the MI355X kernels without editing them.

    PYTHONPATH=<repo>/amphion_amd/integration:<repo>:<Amphion checkout> \
        python <Amphion>/bins/vocoder/inference.py ...

``sitecustomize.py`` in this directory calls ``install()``, which registers a ``sys.meta_path`` finder for
``models.vocoders.vocoder_inference`` and for ``models.codec.codec_inference`` (which carries its own copy of the
same three registries, codec_inference.py:39-75): right after a reference module body has executed, its
``_vocoders`` / ``_vocoder_forward_funcs`` / ``_vocoder_infer_funcs`` entries for the GAN generators built here are
replaced (the dicts are read at call time, vocoder_inference.py:245,346,507).  ``models`` is a regular package, so
it cannot be shadowed -- it is patched.
"""
import importlib.abc
import importlib.util
import os
import sys

TARGETS = ("models.vocoders.vocoder_inference", "models.codec.codec_inference")
TARGET = TARGETS[0]
# generator modules whose CLASSES other models import directly instead of going through the registries:
# models/tts/vits/vits.py:20 (HiFiGAN_vits as Generator), models/tts/jets/jets.py:23,454-458 (HiFiGAN with
# n_mel = attention_dim as the JETS waveform decoder).  Their class attributes are replaced right after the module
# body ran, so a later `from models.vocoders.gan.generator.hifigan import HiFiGAN` binds the MI355X class
# (inference only: these classes have no backward).
CLASS_TARGETS = {
    "models.vocoders.gan.generator.hifigan": ("HiFiGAN", "HiFiGAN_vits"),
    "models.vocoders.gan.generator.bigvgan": ("BigVGAN",),
    "models.vocoders.gan.generator.melgan": ("MelGAN",),
    "models.vocoders.gan.generator.nsfhifigan": ("NSFHiFiGAN",),
    "models.vocoders.gan.generator.apnet": ("APNet",),
}


# Vocos (models/codec/amphion_codec/vocos.py:824-881), the vocoder of Vevo / VevoSing (models/vc/vevo/vevo_utils.py:117-118,
# models/svc/vevosing/vevosing_utils.py:96) and of the MaskGCT codec decoder (models/codec/amphion_codec/codec.py:372-382).
# CodecEncoder / CodecDecoder (models/codec/amphion_codec/codec.py:100-428) are what maskgct_utils.build_acoustic_codec constructs
# (models/tts/maskgct/maskgct_utils.py:66-72): the prompt's wave -> codes and the codes -> latent -> wave path of MaskGCT / DebaTTS / Metis.
# They have their own one-shot finder: _Finder leaves sys.meta_path once the registries and the generator modules are patched,
# whether or not a codec package is ever imported.
CODEC_CLASS_TARGETS = {
    "models.codec.amphion_codec.vocos": ("Vocos",),
    "models.codec.amphion_codec.codec": ("CodecEncoder", "CodecDecoder"),
}


# DiffWave is opt-in: AMP_HOOK_DIFFWAVE=1 in the environment (read once, by the first install()) or install(diffwave=True) make
# install_into_reference overwrite the three `diffwave` registry entries too; without it they stay the reference's.
_DIFFWAVE = None


def _patch_classes(module, fullname, targets=CLASS_TARGETS):
    import importlib

    ours = importlib.import_module("amphion_amd." + fullname)
    for name in targets[fullname]:
        if hasattr(module, name) and hasattr(ours, name):
            setattr(module, "_reference_" + name, getattr(module, name))     # the original stays reachable
            setattr(module, name, getattr(ours, name))
    module.__amphion_amd_patched__ = True


class _PatchLoader(importlib.abc.Loader):
    def __init__(self, inner):
        self._inner = inner

    def create_module(self, spec):
        return self._inner.create_module(spec)

    def exec_module(self, module):
        self._inner.exec_module(module)
        if module.__name__ in CLASS_TARGETS:
            _patch_classes(module, module.__name__)
            return
        from amphion_amd.models.vocoders.vocoder_inference import install_into_reference

        install_into_reference(module, diffwave=bool(_DIFFWAVE))
        module.__amphion_amd_patched__ = True
        for other in TARGETS:       # a target imported while this finder was busy resolving another one
            m = sys.modules.get(other)
            if m is not None and hasattr(m, "_vocoders") and not getattr(m, "__amphion_amd_patched__", False):
                install_into_reference(m, diffwave=bool(_DIFFWAVE))
                m.__amphion_amd_patched__ = True


class _Finder(importlib.abc.MetaPathFinder):
    def __init__(self):
        self._pending = set(TARGETS) | set(CLASS_TARGETS)
        self._busy = False

    def find_spec(self, fullname, path, target=None):
        if self._busy or fullname not in self._pending:
            return None
        self._pending.discard(fullname)       # one shot per target
        self._busy = True                     # find_spec below walks sys.meta_path again
        try:
            spec = importlib.util.find_spec(fullname)
        finally:
            self._busy = False
        if not self._pending:
            sys.meta_path.remove(self)
        if spec is None or spec.loader is None:
            return None
        spec.loader = _PatchLoader(spec.loader)
        return spec


class _ClassPatchLoader(importlib.abc.Loader):
    def __init__(self, inner):
        self._inner = inner

    def create_module(self, spec):
        return self._inner.create_module(spec)

    def exec_module(self, module):
        self._inner.exec_module(module)
        _patch_classes(module, module.__name__, CODEC_CLASS_TARGETS)


class _OneShotClassFinder(importlib.abc.MetaPathFinder):
    """One shot per module of its pending set; leaves sys.meta_path when all of them are patched."""

    def __init__(self, pending):
        self._pending = set(pending)
        self._busy = False

    def find_spec(self, fullname, path, target=None):
        if self._busy or fullname not in self._pending:
            return None
        self._pending.discard(fullname)
        self._busy = True
        try:
            spec = importlib.util.find_spec(fullname)
        finally:
            self._busy = False
        if not self._pending:
            sys.meta_path.remove(self)
        if spec is None or spec.loader is None:
            return None
        spec.loader = _ClassPatchLoader(spec.loader)
        return spec


class _CodecFinder(_OneShotClassFinder):
    """Vocos: gone from sys.meta_path once models.codec.amphion_codec.vocos is patched, whether or not the codec itself is ever imported"""


class _CodecModelFinder(_OneShotClassFinder):
    """CodecEncoder / CodecDecoder (models.codec.amphion_codec.codec)"""


_CODEC_FINDERS = {"models.codec.amphion_codec.vocos": _CodecFinder, "models.codec.amphion_codec.codec": _CodecModelFinder}


def _install_codec():
    pending = {}
    for t in CODEC_CLASS_TARGETS:
        m = sys.modules.get(t)
        if m is None:
            pending.setdefault(_CODEC_FINDERS[t], []).append(t)
        elif not getattr(m, "__amphion_amd_patched__", False):
            _patch_classes(m, t, CODEC_CLASS_TARGETS)
    for cls, targets in pending.items():
        if not any(type(f) is cls for f in sys.meta_path):
            sys.meta_path.insert(0, cls(targets))


def install(diffwave=None):
    global _DIFFWAVE
    if diffwave is not None:
        _DIFFWAVE = bool(diffwave)
    elif _DIFFWAVE is None:
        _DIFFWAVE = os.environ.get("AMP_HOOK_DIFFWAVE", "") == "1"
    _install_codec()
    from_loaded = [t for t in TARGETS if t in sys.modules]
    if from_loaded:
        from amphion_amd.models.vocoders.vocoder_inference import install_into_reference

        for t in from_loaded:
            install_into_reference(sys.modules[t], diffwave=_DIFFWAVE)
            sys.modules[t].__amphion_amd_patched__ = True
    cls_loaded = [t for t in CLASS_TARGETS if t in sys.modules]
    for t in cls_loaded:
        if not getattr(sys.modules[t], "__amphion_amd_patched__", False):
            _patch_classes(sys.modules[t], t)
    if (len(from_loaded) < len(TARGETS) or len(cls_loaded) < len(CLASS_TARGETS)) and not any(isinstance(f, _Finder) for f in sys.meta_path):
        f = _Finder()
        f._pending -= set(from_loaded) | set(cls_loaded)
        sys.meta_path.insert(0, f)
