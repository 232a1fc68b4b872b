"""Vocos on the CPU: the fp64 restatement (tests/vocos_ref.py) against the golden outputs of the real reference class
(tests/golden/make_golden_vocos.py), the drop-in's state_dict keys, and the integration hook for models.codec.amphion_codec.vocos."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import vocos_ref as V  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_vocos_ref_matches_the_reference_class():
    z = np.load(os.path.join(GOLDEN, "golden_vocos.npz"))
    for tag in ("a", "b"):
        hp = V.small_hp(int(z[f"{tag}_n_fft"]), int(z[f"{tag}_hop"]))
        sd = V.synth_vocos_state_dict(hp, int(z[f"{tag}_seed"]))
        y = V.vocos_forward(sd, hp, torch.from_numpy(z[f"{tag}_x"]))
        ref = torch.from_numpy(z[f"{tag}_y"]).double()
        assert y.shape == ref.shape
        assert (y - ref).abs().max().item() <= 2e-5


def test_dropin_keys_at_the_three_configs():
    """the drop-in at the recipe, MaskGCT-decoder and class-default sizes (built on the meta device: no weights allocated) has the
    keys and shapes of vocos_param_shapes, which the golden keys tie to the reference class"""
    from types import SimpleNamespace as NS

    from amphion_amd.models.codec.amphion_codec.vocos import Vocos

    for hp in (V.recipe_hp(), V.maskgct_decoder_hp(), V.class_default_hp()):
        with torch.device("meta"):
            m = Vocos(cfg=NS(**hp))
        got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        assert got == [(k, tuple(v)) for k, v in V.vocos_param_shapes(hp).items()], hp


def test_dropin_state_dict_keys_match_the_reference():
    from amphion_amd.models.codec.amphion_codec.vocos import Vocos

    with open(os.path.join(GOLDEN, "keys_vocos.json")) as f:
        keys = [(k, tuple(s)) for k, s in json.load(f)]
    m = Vocos(**V.small_hp())                        # constructible without a GPU
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == keys
    assert [(k, tuple(v)) for k, v in V.vocos_param_shapes(V.small_hp()).items()] == keys
    # the cfg form (Vocos(cfg=cfg.model.vocos)) and the codec decoder's keyword call
    from types import SimpleNamespace as NS

    m2 = Vocos(cfg=NS(**V.class_default_hp()))
    assert m2.head.out.out_features == 802 and len(m2.backbone.convnext) == 8
    m3 = Vocos(input_channels=256, dim=512, intermediate_dim=4096, num_layers=2, adanorm_num_embeddings=None)
    assert m3.backbone.convnext[0].pwconv1.weight.shape == (4096, 512)


def test_unsupported_forms_raise():
    from amphion_amd.models.codec.amphion_codec.vocos import Vocos

    with pytest.raises(NotImplementedError):
        Vocos(**dict(V.small_hp(), padding="center"))
    with pytest.raises(NotImplementedError):
        Vocos(**V.small_hp(), adanorm_num_embeddings=4)


_STANDIN = '''
class Vocos:
    pass
'''


def test_hook_patches_the_codec_vocos_class(tmp_path):
    pkg = tmp_path / "models" / "codec" / "amphion_codec"
    pkg.mkdir(parents=True)
    for d in (tmp_path / "models", tmp_path / "models" / "codec", pkg):
        (d / "__init__.py").write_text("")
    (pkg / "vocos.py").write_text(_STANDIN)
    code = (
        "import amphion_amd.integration as ig, sys;"
        "ig.install();"
        "assert any(isinstance(f, ig._CodecFinder) for f in sys.meta_path);"
        "from models.codec.amphion_codec.vocos import Vocos;"
        "import models.codec.amphion_codec.vocos as rv;"
        "assert Vocos.__module__ == 'amphion_amd.models.codec.amphion_codec.vocos', Vocos.__module__;"
        "assert rv._reference_Vocos.__module__ == 'models.codec.amphion_codec.vocos';"
        "assert not any(isinstance(f, ig._CodecFinder) for f in sys.meta_path);"
        "print('VOCOS PATCHED')"
    )
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, str(tmp_path)])
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert "VOCOS PATCHED" in r.stdout, r.stdout + r.stderr
