"""CPU checks of the FACodec feature: the fp32 restatement of tests/facodec_ref.py against the golden outputs of the real reference classes
(tests/golden/make_golden_facodec.py), the state_dict key lists, the new ABI, and that the fp64 reference alone decides the quantizer tests'
frames for the seeds the GPU tests use."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import codec_ref as C  # noqa: E402
import facodec_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_facodec.npz"))


@pytest.fixture(scope="module")
def dec_sd(gold):
    return R.synth_decoder_state_dict(R.small_decoder_hp(), int(gold["dec_seed"]))


def close(a, b, rel=2e-5):
    """the restatement in fp32 against the reference's fp32: two fp32 evaluations in different operation orders"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return a.shape == b.shape and float((a - b).abs().max()) <= rel * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("T", [230, 240])
def test_encoder_restatement_matches_the_reference(gold, T):
    hp = R.small_encoder_hp()
    sd = R.synth_encoder_state_dict(hp, int(gold["enc_seed"]))
    z = R.encoder_forward(sd, hp, torch.from_numpy(gold[f"x_{T}"]), torch.float32)
    assert close(z, gold[f"z_{T}"])
    z64 = R.encoder_forward(sd, hp, torch.from_numpy(gold[f"x_{T}"]), torch.float64)
    assert close(z64, gold[f"z_{T}"])


def test_quantizer_restatement_matches_the_reference(gold, dec_sd):
    hp = R.small_decoder_hp()
    z = torch.from_numpy(gold["z_240"])
    r64, r32, tau, decided = R.margin_rule(dec_sd, hp, z)
    qs = torch.from_numpy(gold["fwd_qs"])
    assert qs.shape == r64["qs"].shape == (6, 2, 40)
    assert bool((qs == r64["qs"])[decided].all())
    assert 1.0 - float(decided.all(0).double().mean()) <= 0.02
    follow = R.quantize(dec_sd, hp, z, torch.float32, codes=qs)
    assert close(follow["outs"], gold["fwd_outs"])
    for i in range(3):
        assert close(follow["quantized_buf"][i], gold[f"fwd_buf{i}"])
    assert float(np.abs(gold["fwd_commit"]).sum()) == 0.0 and gold["fwd_commit"].shape == (6,)
    assert close(R.vq2emb(dec_sd, hp, qs, torch.float32), gold["fwd_emb"])
    assert close(R.vq2emb(dec_sd, hp, qs, torch.float32, use_residual_code=False), gold["fwd_emb_nores"])
    assert close(gold["fwd_emb"], gold["fwd_outs"])


def test_timbre_restatement_matches_the_reference(gold, dec_sd):
    z = torch.from_numpy(gold["z_240"])
    spk = R.speaker_embedding(dec_sd, z, torch.float32)
    assert close(spk, gold["fwd_spk"])
    # the quirk: row pe[b] goes to every frame of item b, so item 1 alone (at index 0) embeds differently
    alone = R.speaker_embedding(dec_sd, z[1:2], torch.float64)
    assert float((alone[0] - torch.from_numpy(gold["fwd_spk"][1]).double()).abs().max()) > 1e-3


@pytest.mark.parametrize("n", [1, 7, 33])
def test_decoder_restatement_matches_the_reference(gold, dec_sd, n):
    hp = R.small_decoder_hp()
    w = R.decoder_inference(dec_sd, hp, torch.from_numpy(gold[f"dec_x_{n}"]), torch.from_numpy(gold["dec_spk"]), torch.float32)
    assert close(w, gold[f"dec_wav_{n}"])
    assert float((np.abs(gold[f"dec_wav_{n}"]) > 0.99).mean()) < 0.2          # the tanh is not saturated: the comparison sees the decoder


@pytest.mark.parametrize("T", [1, 63, 65])
def test_fp64_reference_decides_the_quantizer_frames(dec_sd, T):
    hp = R.small_decoder_hp()
    r64, _, tau, decided = R.margin_rule(dec_sd, hp, C.synth_latent(2, hp["vq_dim"], T, R.QUANT_SEEDS[T]))
    undecided = 1.0 - float(decided.all(0).double().mean())
    assert undecided <= 0.02, (T, tau, undecided)
    # the residual group inherits the other two groups' decisions
    assert not bool((decided[3:] & ~(decided[0] & decided[2])[None]).any())


def test_state_dict_keys():
    """drop-in keys + the discarded predictor prefixes == the reference's keys, in the reference's order"""
    from amphion_amd.models.codec.ns3_codec import FACodecDecoder, FACodecEncoder

    with open(os.path.join(GOLDEN, "keys_facodec_encoder.json")) as f:
        ref_e = json.load(f)
    with open(os.path.join(GOLDEN, "keys_facodec_decoder.json")) as f:
        ref_d = json.load(f)
    assert list(FACodecEncoder(**R.small_encoder_hp()).state_dict()) == ref_e == list(R.encoder_param_shapes(R.small_encoder_hp()))
    dec = FACodecDecoder(**R.small_decoder_hp())
    ours = list(dec.state_dict())
    kept = [k for k in ref_d if not k.startswith(R.PREDICTOR_PREFIXES)]
    assert ours == kept == list(R.decoder_param_shapes(R.small_decoder_hp()))
    assert len(kept) < len(ref_d) and all(k.startswith(("f0_predictor.", "phone_predictor.")) for k in ref_d if k not in kept)
    # predictor keys are accepted and discarded; the folded form loads; the shapes agree
    sd = R.synth_decoder_state_dict(R.small_decoder_hp(), 1)
    sd["phone_predictor.heads.0.bias"] = torch.zeros(5003)
    dec.load_state_dict(sd)
    assert list(dec.state_dict()) == kept
    dec.load_state_dict(R.fold(sd))
    assert all(tuple(v.shape) == tuple(R.fold(sd)[k].shape) for k, v in dec.state_dict().items())
    with pytest.raises(NotImplementedError):
        dec(torch.zeros(1, 256, 4), vq=False)


def test_abi_version_and_symbols():
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 148
    for name in ("amp_aa_unit_create", "amp_aa_unit_fused", "amp_set_aa_unit_fusion", "amp_aa_unit_workspace_bytes", "amp_aa_unit_forward",
                 "amp_aa_unit_destroy"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    assert L.amp_set_aa_unit_fusion(3) < 0 and L.amp_set_aa_unit_fusion(-1) == 0
    assert L.amp_aa_unit_fused(None) == -1 and L.amp_aa_unit_workspace_bytes(None, 1, 1) == 0


def test_unit_bound_is_positive_and_scales():
    """the derived bound: positive everywhere, and it grows with the input (it is built from operand magnitudes, not fitted)"""
    sd64 = {k: v.double() for k, v in R.synth_unit_state_dict(32, 1).items()}
    x = C.synth_latent(1, 32, 20, 2).double()
    _, t1 = R.unit_bound(sd64, x, 3)
    _, t2 = R.unit_bound(sd64, 4 * x, 3)
    assert bool((t1 > 0).all()) and float(t2.mean()) > 2 * float(t1.mean())
