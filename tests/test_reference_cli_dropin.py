"""The registry hook (amphion_amd/integration) must make the reference's own modules resolve `hifigan` & co. to the MI355X
generators.  The reference tree is not part of this repository, so the hook is exercised on a stand-in package `models.*` written
into a temporary directory: the module paths, registry dicts and class names the hook patches, nothing else.  The reference
collator is pinned by its golden output (tests/golden/make_golden_collator.py).  The loop the reference CLI runs
(VocoderInference.inference, vocoder_inference.py:334-374) is exercised through its mirror `inference_batches` on the 16 real clips
of BASELINE configs[0]: tests/test_gpu_c1_clips.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the parts of the reference package the hook touches: the three registries of vocoder_inference.py:39-75 (entries of other
# vocoders stay the reference's own) and the generator modules whose classes other models import directly
STANDIN = {
    "models/__init__.py": "",
    "models/vocoders/__init__.py": "",
    "models/vocoders/gan/__init__.py": "",
    "models/vocoders/gan/generator/__init__.py": "",
    "models/vocoders/gan/generator/hifigan.py": "class HiFiGAN:\n    pass\n\n\nclass HiFiGAN_vits:\n    pass\n",
    "models/vocoders/gan/generator/bigvgan.py": "class BigVGAN:\n    pass\n",
    "models/vocoders/gan/generator/melgan.py": "class MelGAN:\n    pass\n",
    "models/vocoders/gan/generator/nsfhifigan.py": "class NSFHiFiGAN:\n    pass\n",
    "models/vocoders/gan/generator/apnet.py": "class APNet:\n    pass\n",
    "models/vocoders/diffwave/__init__.py": "",
    "models/vocoders/diffwave/diffwave.py": "class DiffWave:\n    pass\n",
    "models/vocoders/vocoder_inference.py": (
        "from models.vocoders.diffwave.diffwave import DiffWave\n"
        "from models.vocoders.gan.generator import apnet, bigvgan, hifigan, melgan, nsfhifigan\n\n"
        "_vocoders = {'diffwave': DiffWave, 'nsfhifigan': nsfhifigan.NSFHiFiGAN, 'bigvgan': bigvgan.BigVGAN, 'hifigan': hifigan.HiFiGAN,\n"
        "             'melgan': melgan.MelGAN, 'apnet': apnet.APNet}\n"
        "_vocoder_forward_funcs = {name: None for name in _vocoders}\n"
        "_vocoder_infer_funcs = {name: None for name in _vocoders}\n"),
}


@pytest.fixture
def ref(tmp_path):
    """a stand-in reference tree: its root directory"""
    for rel, text in STANDIN.items():
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
    return str(tmp_path)


def test_hook_patches_reference_registries(ref):
    code = (
        "import models.vocoders.vocoder_inference as m;"
        "import amphion_amd.models.vocoders.gan.generator.hifigan as h, amphion_amd.models.vocoders.gan.generator.bigvgan as b;"
        "assert m._vocoders['hifigan'] is h.HiFiGAN and m._vocoders['bigvgan'] is b.BigVGAN;"
        "assert m._vocoder_forward_funcs['hifigan'].__module__.startswith('amphion_amd');"
        "assert m._vocoder_infer_funcs['bigvgan'].__module__.startswith('amphion_amd');"
        "assert m._vocoders['melgan'].__module__.startswith('amphion_amd');"
            "assert m._vocoders['apnet'].__module__.startswith('amphion_amd');"
            "assert m._vocoders['diffwave'].__module__.startswith('models.');"
        "print('PATCHED', m.__amphion_amd_patched__)"
    )
    env = dict(os.environ)
    env["WORK_DIR"] = ref
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "amphion_amd", "integration"), os.path.join(ROOT, "tests", "shims"), ROOT, ref])
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ref, timeout=300)
    assert "PATCHED True" in r.stdout, r.stdout + r.stderr


def test_hook_patches_generator_classes_for_direct_importers(ref):
    # models/tts/vits/vits.py:20 and models/tts/jets/jets.py:23 import the generator CLASSES, not the registries
    code = (
        "from models.vocoders.gan.generator.hifigan import HiFiGAN, HiFiGAN_vits;"
        "import models.vocoders.gan.generator.hifigan as rh, models.vocoders.gan.generator.bigvgan as rb;"
        "assert HiFiGAN.__module__.startswith('amphion_amd') and HiFiGAN_vits.__module__.startswith('amphion_amd');"
        "assert rb.BigVGAN.__module__.startswith('amphion_amd');"
        "assert rh._reference_HiFiGAN.__module__ == 'models.vocoders.gan.generator.hifigan';"
        "import models.vocoders.vocoder_inference as m;"
        "assert m._vocoders['hifigan'] is HiFiGAN;"
        "print('CLASSES PATCHED')"
    )
    env = dict(os.environ)
    env["WORK_DIR"] = ref
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "amphion_amd", "integration"), os.path.join(ROOT, "tests", "shims"), ROOT, ref])
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ref, timeout=300)
    assert "CLASSES PATCHED" in r.stdout, r.stdout + r.stderr


def test_hook_patches_codec_registries_too(ref):
    # models/codec/codec_inference.py:39-75 holds its own copy of the three registries
    code = (
        "import amphion_amd.integration as ig;"
        "import types, sys;"
        "m = types.ModuleType('models.codec.codec_inference');"
        "m._vocoders = {'hifigan': None, 'diffwave': 'ref'}; m._vocoder_forward_funcs = {}; m._vocoder_infer_funcs = {};"
        "sys.modules['models.codec.codec_inference'] = m;"
        "ig.install();"
        "assert m._vocoders['hifigan'].__module__.startswith('amphion_amd') and m._vocoders['diffwave'] == 'ref';"
        "assert m._vocoder_infer_funcs['bigvgan'].__module__.startswith('amphion_amd');"
        "assert any(isinstance(f, ig._Finder) for f in sys.meta_path);"          # still waiting for the vocoder module
        "import models.vocoders.vocoder_inference as v;"
        "assert v.__amphion_amd_patched__ and not any(isinstance(f, ig._Finder) for f in sys.meta_path);"
        "print('BOTH PATCHED')"
    )
    env = dict(os.environ)
    env["WORK_DIR"] = ref
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests", "shims"), ROOT, ref])
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ref, timeout=300)
    assert "BOTH PATCHED" in r.stdout, r.stdout + r.stderr


def test_collator_matches_reference():
    # models/vocoders/vocoder_dataset.py:229-264 (golden output on a ragged batch) against the mirror, on the same batch
    from amphion_amd.models.vocoders.vocoder_dataset import VocoderCollator as Ours, batch_to_generator_input

    G = np.load(os.path.join(ROOT, "tests", "golden", "golden_collator.npz"))
    lens = [int(n) for n in G["lens"]]
    batch = [{"target_len": n, "mel": G[f"in_{i}_mel"], "frame_pitch": G[f"in_{i}_frame_pitch"], "audio": G[f"in_{i}_audio"]}
             for i, n in enumerate(lens)]
    a = {str(k): torch.from_numpy(G[f"out_{k}"]) for k in G["keys"]}
    b = Ours(None)(batch)
    assert list(a) == list(b), (list(a), list(b))
    assert all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)
    mel, ln = batch_to_generator_input(b)
    assert mel.shape == (4, 4, 9) and ln == lens and torch.equal(mel[1, :, :3], torch.from_numpy(batch[1]["mel"]))
