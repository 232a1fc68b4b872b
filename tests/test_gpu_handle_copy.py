"""A deep copy of a module that has run gets its own device handle: the copy computes the same bits, and changing a parameter of the copy
changes the copy's output and leaves the original's bit for bit.  One representative of each kind of owner of a ``HandleCache``
(amphion_amd/_handle.py), at the smallest configuration its own GPU test uses."""
import copy
import os
import sys
from types import SimpleNamespace as NS

import pytest
import torch

from oracle import synth
from oracle import vocoder_oracle as vo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import codec_ref  # noqa: E402
import diffwave_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _hipconv1d():
    from amphion_amd.modules.hip_ops import HipConv1d

    return HipConv1d(32, 48, 3, padding=1), (_randn(2, 32, 100, seed=1),), lambda m: m.bias


def _residual_unit():
    from amphion_amd.models.codec.amphion_codec.codec import ResidualUnit

    return ResidualUnit(32, dilation=3), (_randn(2, 32, 65, seed=2),), lambda m: m.block[3].bias


def _residual_vq():
    from amphion_amd.models.codec.amphion_codec.quantize import ResidualVQ

    hp = codec_ref.small_fvq_hp()
    m = ResidualVQ(input_dim=hp["D"], num_quantizers=hp["N"], codebook_size=hp["K"], codebook_dim=hp["d"], quantizer_type="fvq",
                   use_l2_normlize=hp["l2"])
    return m, (_randn(2, hp["D"], 65, seed=3),), lambda m: m.quantizers[0].out_project.bias


def _slstm():
    from amphion_amd.models.codec.speechtokenizer.modules.lstm import SLSTM

    return SLSTM(20, num_layers=2), (_randn(2, 20, 33, seed=4),), lambda m: m.lstm.bias_ih_l0


def _diffwave():
    from amphion_amd.models.vocoders.diffusion.diffwave.diffwave import DiffWave

    hp = diffwave_ref.SMALL
    m = DiffWave(diffwave_ref.make_cfg(**hp))
    with torch.no_grad():
        m.output_projection.weight.normal_(0.0, 0.1, generator=torch.Generator().manual_seed(5))     # the constructor zeroes it
    F = 6
    args = (_randn(1, F * hp["u"][0] * hp["u"][1], seed=6), torch.tensor([3], device=DEV), _randn(1, hp["n_mel"], F, seed=7))
    return m, args, lambda m: m.output_projection.bias


def _hifigan():
    from amphion_amd.models.vocoders.gan.generator.hifigan import HiFiGAN

    hp = vo.hifigan_v1_hp()
    m = HiFiGAN(NS(preprocess=NS(n_mel=80, hop_size=256), model=NS(hifigan=NS(**hp))))
    m.load_state_dict(synth.synth_state_dict(synth.hifigan_param_shapes(80, hp), 1234))
    return m, (synth.synth_mel(1, 80, 40, seed=8).to(DEV),), lambda m: m.conv_post.bias


def _first(y):
    return y[0] if isinstance(y, (tuple, list)) else y


@pytest.mark.parametrize("case", [_hipconv1d, _residual_unit, _residual_vq, _slstm, _diffwave, _hifigan], ids=lambda f: f.__name__.strip("_"))
def test_deepcopy_after_a_forward_owns_its_handle(case):
    torch.manual_seed(0)
    m, args, param = case()
    m = m.to(DEV).eval()
    with torch.no_grad():
        y = _first(m(*args)).clone()
        m2 = copy.deepcopy(m)
        y2 = _first(m2(*args)).clone()
        assert torch.isfinite(y).all() and float(y.abs().max()) > 0 and torch.equal(y2, y)
        param(m2).add_(0.25)
        y_again, y2_changed = _first(m(*args)).clone(), _first(m2(*args)).clone()
    torch.cuda.synchronize()
    assert torch.equal(y_again, y)
    assert not torch.equal(y2_changed, y)
