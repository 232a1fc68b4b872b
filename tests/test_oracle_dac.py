"""CPU: the torch restatement of tests/dac_ref.py reproduces what the real reference classes computed (tests/golden/golden_dac.npz, written by
tests/golden/make_golden_dac.py), the key lists of the restatement and of the drop-in modules are the reference's, and the drop-ins refuse what
they must before any launch."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import codec_ref as C  # noqa: E402
import dac_ref as D  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [("small", 1), ("small", 7), ("small", 33), ("even", 33)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_dac.npz"))


def keys(name):
    with open(os.path.join(GOLDEN, f"keys_{name}.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)]


def hp_of(name):
    return D.small_decoder_hp() if name == "small" else D.even_decoder_hp()


@pytest.mark.parametrize("name,T", CASES)
def test_decoder_draw_does_not_saturate(gold, name, T):
    """on the fp64 reference alone, before anything is compared: a saturated tanh would hide every error in front of it"""
    hp = hp_of(name)
    sd = D.synth_decoder_state_dict(hp, int(gold[f"{name}_seed"]))
    y = D.decoder_forward(sd, hp, torch.from_numpy(gold[f"{name}_x_{T}"]), torch.float64)
    share = float((y.abs() > 0.99).double().mean())
    print(f"{name} T={T}: saturated share {share:.4f}, rms {float(y.pow(2).mean().sqrt()):.3f}")
    assert share <= 0.01


@pytest.mark.parametrize("name,T", CASES)
def test_decoder_restatement_matches_reference(gold, name, T):
    hp = hp_of(name)
    sd = D.synth_decoder_state_dict(hp, int(gold[f"{name}_seed"]))
    y = D.decoder_forward(sd, hp, torch.from_numpy(gold[f"{name}_x_{T}"]), torch.float64)
    ref = torch.from_numpy(gold[f"{name}_y_{T}"]).double()
    assert y.shape == ref.shape
    t = T
    for s in hp["rates"]:                                  # T_out = T s for even s, T s - 1 for odd s (no output_padding)
        t = D.tconv_out_len(t, s, D.block_padding(s), 0)
    assert y.shape[2] == t
    rel = float((y - ref).abs().max() / ref.abs().max())
    print(f"{name} T={T}: wave {tuple(y.shape)}, max rel err {rel:.2e}")
    assert rel <= 1e-5


def test_output_padding_block_matches_reference(gold):
    sd = D.synth_block_state_dict(64, 32, 3, int(gold["ab_seed"]))
    P = {k: v.double() for k, v in sd.items()}
    y = D.decoder_block_forward(P, "block.", torch.from_numpy(gold["ab_x"]).double(), 3, output_padding=1)
    ref = torch.from_numpy(gold["ab_y"]).double()
    assert y.shape == ref.shape and y.shape[2] == 33 * 3
    assert float((y - ref).abs().max() / ref.abs().max()) <= 1e-5


def test_encoder_restatement_matches_reference(gold):
    hp = D.small_dac_encoder_hp()
    sd = D.synth_dac_encoder_state_dict(hp, int(gold["enc_seed"]))
    chp = dict(d_model=hp["d_model"], up_ratios=hp["strides"], out_channels=hp["d_latent"])
    z = C.encoder_forward(sd, chp, torch.from_numpy(gold["enc_x"]), torch.float64)
    ref = torch.from_numpy(gold["enc_z"]).double()
    assert z.shape == ref.shape and float((z - ref).abs().max() / ref.abs().max()) <= 1e-5


def test_key_lists_match_reference():
    assert [(k, tuple(v)) for k, v in D.decoder_param_shapes(D.small_decoder_hp()).items()] == keys("dac_decoder")
    assert [(k, tuple(v)) for k, v in D.dac_encoder_param_shapes(D.small_dac_encoder_hp()).items()] == keys("dac_encoder")


def test_drop_in_modules_have_reference_keys():
    import torch.nn as nn
    from amphion_amd.models.codec.amphion_codec.codec import DecoderBlock as AmphionBlock
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import Decoder, DecoderBlock, Encoder
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import dac_layers, dac_model

    hp, ehp = D.small_decoder_hp(), D.small_dac_encoder_hp()
    dec, enc = Decoder(**hp), Encoder(**ehp)
    assert [(k, tuple(v.shape)) for k, v in dec.state_dict().items()] == keys("dac_decoder")
    assert [(k, tuple(v.shape)) for k, v in enc.state_dict().items()] == keys("dac_encoder")
    assert isinstance(dec.model[-1], nn.Tanh) and len(dec.model) == 1 + len(hp["rates"]) + 3 and dec.model[-2].tanh      # the reference's indices
    assert enc.enc_dim == ehp["d_model"] * 2 ** len(ehp["strides"])
    for name in ("Snake1d", "snake", "WNConv1d", "WNConvTranspose1d"):
        assert hasattr(dac_layers, name)
    for name in ("ResidualUnit", "EncoderBlock", "Encoder", "DecoderBlock", "Decoder"):
        assert hasattr(dac_model, name)
    # both forms of the block: the same keys, output_padding 0 (DualCodec) or stride % 2 (Amphion)
    b0, b1 = DecoderBlock(64, 32, 3), AmphionBlock(64, 32, 3)
    shapes = [(k, tuple(v)) for k, v in D.decoder_block_shapes(64, 32, 3).items()]
    assert [(k, tuple(v.shape)) for k, v in b0.state_dict().items()] == shapes == [(k, tuple(v.shape)) for k, v in b1.state_dict().items()]
    assert (b0.block[1].output_padding, b1.block[1].output_padding) == (0, 1) and b0.block[1].padding == b1.block[1].padding == 2
    assert b0.block[1].out_len(33) == 98 and b1.block[1].out_len(33) == 99
    t = dac_layers.WNConvTranspose1d(64, 32, kernel_size=8, stride=4, padding=2)
    assert tuple(t.weight_g.shape) == (64, 1, 1) and tuple(t.weight_v.shape) == (64, 32, 8)      # the norm is over the INPUT channels
    with pytest.raises(NotImplementedError):
        dac_layers.WNConvTranspose1d(64, 32, kernel_size=7, stride=4)


def test_folded_weights_load_and_come_back_folded():
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import Decoder

    hp = D.small_decoder_hp()
    sd = D.synth_decoder_state_dict(hp, 5)
    dec = Decoder(**hp)
    dec.load_state_dict(sd)
    back = dec.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    w = dec.model[1].block[1].folded_weight()                  # g * v / ||v|| per INPUT channel
    assert torch.allclose(w, C.folded(sd, "model.1.block.1."), rtol=1e-6, atol=0)
    fsd = D.fold_state_dict(sd)
    dec.load_state_dict(fsd)
    assert set(dec.state_dict()) == set(fsd) and torch.equal(dec.state_dict()["model.1.block.1.weight"], fsd["model.1.block.1.weight"])
    dec.load_state_dict(sd)                                    # and back to the weight-normed form
    assert list(dec.state_dict()) == list(sd)


def test_refusals_before_any_launch():
    """a wrong channel count is a ValueError and a host tensor a RuntimeError, both raised before the device is looked at"""
    from amphion_amd.models.codec.amphion_codec.codec import CodecDecoder
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import Decoder, DecoderBlock, Encoder

    dec, blk, enc = Decoder(**D.even_decoder_hp()).eval(), DecoderBlock(64, 32, 4).eval(), Encoder(**D.small_dac_encoder_hp()).eval()
    for call in (lambda: dec(torch.zeros(1, 65, 4)), lambda: dec(torch.zeros(64, 4)), lambda: blk(torch.zeros(1, 32, 4)),
                 lambda: enc(torch.zeros(1, 2, 64))):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: dec(torch.zeros(1, 64, 4)), lambda: blk(torch.zeros(1, 64, 4)), lambda: enc(torch.zeros(1, 1, 64))):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(NotImplementedError):                   # the convolutional CodecDecoder stays refused: its wiring is a follow-up
        CodecDecoder(quantizer_type="fvq", use_vocos=False)


def test_library_has_the_tconv_entry_points():
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 146
    for name in ("amp_tconv_create", "amp_tconv_out_len", "amp_tconv_fused", "amp_set_tconv_fusion", "amp_tconv_workspace_bytes",
                 "amp_tconv_forward", "amp_tconv_destroy"):
        assert hasattr(L, name)
    assert L.amp_tconv_out_len(None, 5) == 0 and L.amp_tconv_fused(None) == -1 and L.amp_tconv_workspace_bytes(None, 1, 1) == 0
    with pytest.raises(_lib.AmpError):
        _lib.check(L.amp_set_tconv_fusion(2))
    _lib.check(L.amp_set_tconv_fusion(-1))
