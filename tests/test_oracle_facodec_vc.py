"""CPU checks of FACodec's voice-conversion classes: the fp32 restatement of tests/facodec_vc_ref.py against the golden outputs of the real
reference classes (tests/golden/make_golden_facodec_vc.py), the state_dict key lists, the new ABI, and that the fp64 reference alone decides the
frames of the GPU quantizer tests for the seeds they use."""
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
import facodec_vc_ref as V  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def close(a, b, rel=2e-5):
    """the restatement in fp32 against the reference's fp32: two fp32 evaluations in different operation orders (tests/test_oracle_facodec.py)"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return a.shape == b.shape and float((a - b).abs().max()) <= rel * max(1.0, float(b.abs().max()))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_facodec_vc.npz"))


@pytest.fixture(scope="module")
def dec_sd(gold):
    return V.synth_decoder_v2_state_dict(R.small_decoder_hp(), int(gold["dec_seed"]))


@pytest.fixture(scope="module")
def red_sd(gold):
    return V.synth_redecoder_state_dict(V.small_redecoder_hp(), int(gold["red_seed"]))


def g(gold, k):
    return torch.from_numpy(gold[k])


def test_style_layer_norm_is_the_reference_expression():
    """against torch's own modules: LayerNorm without affine, a Linear on the condition's mean, gamma * norm + beta"""
    t = torch.Generator().manual_seed(5)
    x, cond = torch.randn(2, 9, 16, generator=t, dtype=torch.float64), torch.randn(2, 9, 16, generator=t, dtype=torch.float64)
    lin = torch.nn.Linear(16, 32).double()
    style = lin(cond.mean(dim=1, keepdim=True))
    want = style[..., :16] * torch.nn.LayerNorm(16, elementwise_affine=False)(x) + style[..., 16:]
    got = V.style_layer_norm(x, cond.mean(dim=1, keepdim=True), lin.weight, lin.bias)
    assert torch.allclose(got, want, rtol=0, atol=1e-14)


def test_encoder_and_prosody_feature_restatement(gold):
    hp = R.small_encoder_hp()
    sd = V.synth_encoder_v2_state_dict(hp, int(gold["enc_seed"]))
    block = {k: v for k, v in sd.items() if k.startswith("block.")}
    assert close(R.encoder_forward(block, hp, g(gold, "x_230"), torch.float32), gold["z_230"])
    for L in (600, 1000, 1601):
        pf = gold[f"pf_{L}"]
        assert pf.shape == (2, 20, 1 + (L - 200) // 200)
        for dt in (torch.float32, torch.float64):
            # a log: compared absolutely, at the front end's documented 1e-4
            assert float((V.prosody_feature(g(gold, f"wave_{L}"), dt).double() - torch.from_numpy(pf).double()).abs().max()) <= 1e-4
    mb, hw = V.mel_buffers()
    assert torch.equal(sd["mel_transform.mel_basis"], mb) and torch.equal(sd["mel_transform.hann_window"], hw)


def test_decoder_v2_restatement_matches_the_reference(gold, dec_sd):
    hp = R.small_decoder_hp()
    x, pf = g(gold, "fwd_x"), g(gold, "fwd_pf")
    xp64 = V.prosody_latent(dec_sd, pf, torch.float64)
    r64, r32, tau, decided = V.margin_rule3(dec_sd, hp, xp64, x)
    qs = g(gold, "fwd_qs")
    assert qs.shape == r64["qs"].shape == (6, 2, 33)
    assert bool((qs == r64["qs"])[decided].all())
    assert 1.0 - float(decided.all(0).double().mean()) <= 0.1
    follow = V.quantize3(dec_sd, hp, V.prosody_latent(dec_sd, pf, torch.float32), x, torch.float32, codes=qs)
    assert close(follow["outs"], gold["fwd_outs"]) and close(follow["quantized_buf"][0], gold["fwd_buf0"])
    assert float(np.abs(gold["fwd_commit"]).sum()) == 0.0 and gold["fwd_commit"].shape == (6,)
    assert close(V.vq2emb_v2(dec_sd, hp, qs, torch.float32, use_residual=False), gold["fwd_emb_nores"])
    assert close(R.speaker_embedding(dec_sd, x, torch.float32), gold["fwd_spk"])
    # the prosody group really quantizes the mel encoding: the latent in its place gives other codes
    assert not torch.equal(R.quantize(dec_sd, hp, x)["qs"][0], qs[0])


@pytest.mark.parametrize("n", [1, 7, 33])
def test_wave_restatements_match_the_reference(gold, dec_sd, red_sd, n):
    dhp, rhp = R.small_decoder_hp(), V.small_redecoder_hp()
    x, spk, vq = g(gold, f"x_{n}"), g(gold, "spk"), g(gold, f"vq_{n}")
    # waves at 1e-4, the relative tolerance every wave test of the decoder uses: the restatement and the real class are two fp32 walks through
    # 2 x 3 anti-aliased units in different operation orders, and at 33 frames EACH is 2.1e-5 from fp64 for this seed
    assert close(V.styled_inference(dec_sd, dhp, x, spk, torch.float32), gold[f"v2_wav_{n}"], 1e-4)
    assert close(V.styled_inference(red_sd, rhp, x, spk, torch.float32), gold[f"red_inf_wav_{n}"], 1e-4)
    for res in (False, True):
        assert close(V.redecoder_forward(red_sd, rhp, vq, spk, torch.float32, res), gold[f"red_fwd_wav_{n}_{int(res)}"], 1e-4)
        if f"red_emb_{n}_{int(res)}" in gold:
            assert close(V.redecoder_vq2emb(red_sd, rhp, vq, spk, torch.float32, res), gold[f"red_emb_{n}_{int(res)}"])
    assert float((np.abs(gold[f"red_fwd_wav_{n}_1"]) > 0.99).mean()) < 0.2           # the tanh is not saturated
    # the codes cover both ends of every table, and the speaker matters
    sizes = [5, 6, 6, 5, 5, 5]
    assert all(int(vq[i].min()) == 0 and int(vq[i].max()) == 2 ** s - 1 for i, s in enumerate(sizes))
    other = V.redecoder_vq2emb(red_sd, rhp, vq, -spk, torch.float64)
    assert float((other - V.redecoder_vq2emb(red_sd, rhp, vq, spk, torch.float64)).abs().max()) > 1e-2


def test_redecoder_summation_orders_differ(gold, red_sd):
    """forward groups the content and residual tables before adding them, vq2emb adds one table after another: the same codes, another
    rounding.  In fp64 the two agree to rounding, in fp32 they are not the same bits -- why amp_embed_sum_c is called both ways"""
    rhp = V.small_redecoder_hp()
    vq, spk = g(gold, "vq_33"), g(gold, "spk")
    a = V.redecoder_latent(red_sd, rhp, vq, spk, torch.float32, True)
    b = V.redecoder_vq2emb(red_sd, rhp, vq, spk, torch.float32, True)
    assert not torch.equal(a, b) and float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


@pytest.mark.parametrize("T", [1, 63, 65])
def test_fp64_reference_decides_the_quantizer_frames(dec_sd, T):
    hp = R.small_decoder_hp()
    sx, sp = V.QUANT_SEEDS[T]
    x, pf = C.synth_latent(2, hp["vq_dim"], T, sx), V.synth_prosody_feature(2, T, sp)
    r64, _, tau, decided = V.margin_rule3(dec_sd, hp, V.prosody_latent(dec_sd, pf), x)
    undecided = 1.0 - float(decided.all(0).double().mean())
    assert undecided <= 0.02, (T, tau, undecided)
    assert not bool((decided[3:] & ~(decided[0] & decided[2])[None]).any())


def test_state_dict_keys():
    """drop-in keys + the discarded predictor prefixes == the reference's keys, in the reference's order"""
    from amphion_amd.models.codec.ns3_codec import FACodecDecoderV2, FACodecEncoderV2, FACodecRedecoder

    def ref(name):
        with open(os.path.join(GOLDEN, f"keys_facodec_{name}.json")) as f:
            return json.load(f)

    ehp, dhp, rhp = R.small_encoder_hp(), R.small_decoder_hp(), V.small_redecoder_hp()
    assert list(FACodecEncoderV2(**ehp).state_dict()) == ref("encoder_v2") == list(V.encoder_v2_param_shapes(ehp))
    red = FACodecRedecoder(**rhp)
    assert list(red.state_dict()) == ref("redecoder") == list(V.redecoder_param_shapes(rhp))
    assert all(tuple(v.shape) == V.redecoder_param_shapes(rhp)[k] for k, v in red.state_dict().items())
    dec = FACodecDecoderV2(**dhp)
    ref_d = ref("decoder_v2")
    kept = [k for k in ref_d if not k.startswith(R.PREDICTOR_PREFIXES)]
    assert list(dec.state_dict()) == kept == list(V.decoder_v2_param_shapes(dhp))
    assert len(kept) < len(ref_d) and all(k.startswith(("f0_predictor.", "phone_predictor.")) for k in ref_d if k not in kept)
    sd = V.synth_decoder_v2_state_dict(dhp, 1)
    sd["phone_predictor.heads.0.bias"] = torch.zeros(5003)
    dec.load_state_dict(sd)
    assert list(dec.state_dict()) == kept
    dec.load_state_dict(R.fold(sd))
    # the style Linears start as the reference's: scale 1, shift 0
    b = red.timbre_cond_prosody_enc.last_ln.style.bias
    assert torch.equal(b[:256], torch.ones(256)) and torch.equal(b[256:], torch.zeros(256))


def test_host_side_refusals():
    from amphion_amd.models.codec.ns3_codec import FACodecDecoderV2, FACodecRedecoder, MelSpectrogram
    from amphion_amd.models.codec.ns3_codec.transformer import TransformerEncoder

    with pytest.raises(ValueError):
        FACodecRedecoder(vq_dim=128)
    with pytest.raises(ValueError):
        FACodecRedecoder(in_channels=128)
    with pytest.raises(NotImplementedError):
        MelSpectrogram(1024, 80, 16000, 200, 800, 0, 8000, center=True)
    dec = FACodecDecoderV2(**R.small_decoder_hp())
    with pytest.raises(NotImplementedError):
        dec(torch.zeros(1, 256, 4), torch.zeros(1, 20, 4), vq=False)
    with pytest.raises(NotImplementedError):
        TransformerEncoder(use_cln=True).eval()(torch.zeros(1, 4, 256), key_padding_mask=torch.ones(1, 4), condition=torch.zeros(1, 4, 256))
    with pytest.raises(ValueError):
        TransformerEncoder(use_cln=True).eval()(torch.zeros(1, 4, 256))
    with pytest.raises(RuntimeError):
        MelSpectrogram(1024, 80, 16000, 200, 800, 0, 8000)(torch.zeros(1, 1000))            # a host tensor: no CPU fallback


def test_abi_version_and_symbols():
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 151
    for name in ("amp_layer_norm_c_style", "amp_embed_sum_c", "amp_embed_sum_check"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    with open(os.path.join(ROOT, "include", "amphion_hip.h")) as f:
        header = f.read()
    assert all(f"int {name}(" in header for name in ("amp_layer_norm_c_style", "amp_embed_sum_c", "amp_embed_sum_check"))
    # judged on the host before a device is touched
    assert L.amp_layer_norm_c_style(None, None, None, 1, 1, 1, 1e-5, None, None) == _lib.AMP_ERR_INVALID
    assert L.amp_embed_sum_c(None, 1, None, None, 1, None, 1, 1, None, None, None) == _lib.AMP_ERR_INVALID
    assert L.amp_embed_sum_check(None, None) == _lib.AMP_ERR_INVALID
