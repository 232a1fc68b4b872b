"""CPU: the torch restatement of tests/dualcodec_ref.py reproduces what the real reference classes computed (tests/golden/golden_dualcodec.npz,
written by tests/golden/make_golden_dualcodec.py: codes equal, tensors to 1e-5 of their largest magnitude), the key lists of the restatement and of
the drop-in modules are the reference's, the fp64 reference alone decides (margin rule of codec_ref) at least 98 % of the frames of every quantizer
case the GPU tests use, and the library and the drop-ins refuse what they must before any launch."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import codec_ref as C  # noqa: E402
import dualcodec_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NETS = [("causal", True), ("centred", False)]
CASES = [(tag, causal, T) for tag, causal in NETS for T in R.MODEL_LENGTHS]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_dualcodec.npz"))


def keys(name):
    with open(os.path.join(GOLDEN, f"keys_{name}.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)]


def rel(a, ref):
    ref = torch.as_tensor(ref).double()
    assert tuple(a.shape) == tuple(ref.shape), (tuple(a.shape), tuple(ref.shape))
    return float((a.double() - ref).abs().max() / ref.abs().max())


_ENC = {}


def encoded(causal, T):
    """the fp64 restatement of one golden case, computed once"""
    if (causal, T) not in _ENC:
        hp = R.small_hp(causal)
        sd = R.synth_dualcodec_state_dict(hp, R.MODEL_SEED)
        wave, feats = R.model_inputs(hp, T)
        _ENC[(causal, T)] = (hp, sd, wave, feats, R.encode(sd, hp, wave, feats))
    return _ENC[(causal, T)]


@pytest.mark.parametrize("tag,causal,T", CASES)
def test_restatement_matches_reference(gold, tag, causal, T):
    hp, sd, wave, feats, e = encoded(causal, T)
    p = f"{tag}_{T}_"
    assert int(gold["seed"]) == R.MODEL_SEED
    s = R.semantic_quantize(sd, hp, feats)
    assert rel(s["h"], gold[p + "cn_enc"]) <= 1e-5
    assert torch.equal(e["semantic_codes"], torch.from_numpy(gold[p + "sem_codes"]))
    assert torch.equal(e["acoustic_codes"], torch.from_numpy(gold[p + "ac_codes"]))
    assert e["semantic_codes"].shape == (2, 1, T) and e["acoustic_codes"].shape == (2, hp["n_codebooks"], T)
    assert rel(e["r"]["latents"], gold[p + "latents"]) <= 1e-5
    qsd = R.quantizer_sd(sd, "dac.quantizer.quantizers.")
    loss = float(R.rvq_losses(qsd, e["r"]))
    assert abs(loss - gold[p + "losses"][0]) <= 1e-5 * loss and abs(loss - gold[p + "losses"][1]) <= 1e-5 * loss
    if p + "z" in gold.files:
        assert rel(e["z"], gold[p + "z"]) <= 1e-5 and rel(e["r"]["z_q_1"], gold[p + "first"]) <= 1e-5
    two = R.encode(sd, hp, wave, feats, num_quantizers=2)
    assert torch.equal(two["acoustic_codes"], e["acoustic_codes"][:, :1])
    assert R.encode(sd, hp, wave, feats, num_quantizers=1)["acoustic_codes"] is None
    y = R.decode_from_codes(sd, hp, e["semantic_codes"], e["acoustic_codes"])
    assert rel(y, gold[p + "wave"]) <= 1e-5
    assert rel(R.decode_from_codes(sd, hp, e["semantic_codes"], None), gold[p + "wave_sem"]) <= 1e-5
    print(f"{tag} T={T}: wave {tuple(y.shape)}, saturated share {float((y.abs() > 0.99).double().mean()):.4f}")


@pytest.mark.parametrize("tag,causal", NETS)
def test_block_restatement_matches_reference(gold, tag, causal):
    bsd = {k: v.double() for k, v in R.synth_convnext_block(64, "", R.MODEL_SEED + 50, gamma=True).items()}
    x = C.synth_latent(2, 64, 33, R.MODEL_SEED + 51).double()
    assert rel(R.convnext_block(bsd, "", x, causal), gold[f"{tag}_blk_y"]) <= 1e-5
    # the causal block never looks ahead: frame t is unchanged when later frames are
    if causal:
        x2 = x.clone()
        x2[..., 20:] = 0.0
        assert torch.equal(R.convnext_block(bsd, "", x2, True)[..., :20], R.convnext_block(bsd, "", x, True)[..., :20])


def test_quantizer_and_preparation_restatements_match_reference(gold):
    qhp = dict(D=64, d=8, K=64, N=3, l2=True)
    qsd = R.quantizer_sd(R.synth_rvq_state_dict(qhp, R.MODEL_SEED + 60), "quantizers.")
    z = C.synth_latent(2, 64, 33, R.MODEL_SEED + 61)
    r = R.rvq_forward(qsd, qhp, z, n=2)
    assert torch.equal(r["codes"].transpose(0, 1), torch.from_numpy(gold["rvq_codes"]))
    assert rel(r["zq"], gold["rvq_zq"]) <= 1e-5 and rel(r["latents"], gold["rvq_latents"]) <= 1e-5 and rel(r["z_q_1"], gold["rvq_first"]) <= 1e-5
    loss = float(R.rvq_losses(qsd, r))
    assert abs(loss - gold["rvq_losses"][0]) <= 1e-5 * loss and abs(loss - gold["rvq_losses"][1]) <= 1e-5 * loss
    assert rel(C.vq2emb(qsd, qhp, r["codes"], n=2), gold["rvq_from_codes"]) <= 1e-5
    hidden, mean, std = R.synth_hidden(2, 9, 64, R.MODEL_SEED + 70)
    prep = R.prepare_semantic_features(hidden, mean, std, 2)
    assert prep.shape == (2, 64, 4) and rel(prep, gold["prep"]) <= 1e-5


def test_key_lists_match_reference():
    hp = R.small_hp(True)
    assert [(k, tuple(v)) for k, v in R.dualcodec_param_shapes(hp).items()] == keys("dualcodec")
    assert [(k, tuple(v)) for k, v in R.rvq_param_shapes(R.acoustic_q_hp(hp)).items()] == keys("dac_rvq")


def test_drop_in_modules_have_reference_keys():
    from amphion_amd.models.codec.dualcodec.dualcodec import model_codec as M

    for causal in (True, False):
        hp = R.small_hp(causal)
        m = M.DualCodec(**hp)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == keys("dualcodec")
        assert [(k, tuple(v.shape)) for k, v in m.dac.quantizer.state_dict().items()] == keys("dac_rvq")
        assert isinstance(m.dac, M.DAC) and isinstance(m.semantic_vq, M.ResidualVectorQuantize) and isinstance(m.convnext_encoder[1], M.ConvNeXtBlock)
        assert all(b.is_causal == causal and b.gamma is None and b.dwconv.padding == ((0,) if causal else (3,)) for b in list(m.convnext_encoder)[1:])
        assert m.dac.hop_length == 6 and m.dac.latent_dim == 1024 and m.semantic_downsample_factor == 2
    blk = M.ConvNeXtBlock(64, 2048, layer_scale_init_value=0.5, is_causal=True)
    assert [(k, tuple(v.shape)) for k, v in blk.state_dict().items()] == [(k, tuple(v)) for k, v in R.convnext_block_shapes(64, "", gamma=True).items()]
    assert M.DAC(encoder_dim=8, encoder_rates=[2, 3], decoder_dim=64, decoder_rates=[3, 2]).latent_dim == 32     # encoder_dim * 2 ** len(rates)
    for name in ("DualCodec", "DAC", "ResidualVectorQuantize", "VectorQuantize", "ConvNeXtBlock", "prepare_semantic_features", "AttrDict"):
        assert hasattr(M, name)


def test_folded_weights_load_and_come_back_folded():
    import dac_ref as D
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import DualCodec

    hp = R.small_hp(True)
    sd = R.synth_dualcodec_state_dict(hp, 5)
    m = DualCodec(**hp)
    m.load_state_dict(sd)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    fsd = D.fold_state_dict(sd)
    m.load_state_dict(fsd)
    assert set(m.state_dict()) == set(fsd)
    assert torch.equal(m.state_dict()["semantic_vq.quantizers.0.in_proj.weight"], fsd["semantic_vq.quantizers.0.in_proj.weight"])
    m.load_state_dict(sd)
    assert list(m.state_dict()) == list(sd)


@pytest.mark.parametrize("name", list(R.FVQ_OP_CASES))
@pytest.mark.parametrize("T", R.FVQ_OP_LENGTHS)
def test_op_cases_are_decided_by_fp64_alone(name, T):
    """the cap is a condition on the cases, not a tolerance: with and without the subtracted tensor"""
    qhp, sd, z, sub = R.fvq_op_inputs(name, T)
    qsd = R.quantizer_sd(sd, "quantizers.")
    for tag, zin in (("plain", z[..., :T].contiguous()), ("sub", z[..., :T] - sub)):
        r64, _, tau, decided = C.margin_rule(qsd, qhp, zin)
        undecided = 1.0 - float(decided[-1].double().mean())
        print(f"{name} T={T} {tag}: tau {tau:.3e}, smallest fp64 margin {float(r64['margin'].min()):.3e}, undecided {undecided:.4f}")
        assert undecided <= 0.02


@pytest.mark.parametrize("tag,causal,T", CASES)
def test_model_cases_are_decided_by_fp64_alone(tag, causal, T):
    hp, sd, wave, feats, e = encoded(causal, T)
    s = R.semantic_quantize(sd, hp, feats)
    for name, prefix, qhp, z in (("semantic", "semantic_vq.quantizers.", R.semantic_q_hp(hp), s["h"]),
                                 ("acoustic", "dac.quantizer.quantizers.", R.acoustic_q_hp(hp), e["z_enc"][..., :T] - e["semantic"])):
        r64, _, tau, decided = C.margin_rule(R.quantizer_sd(sd, prefix), qhp, z.float())
        undecided = 1.0 - float(decided[-1].double().mean())
        print(f"{tag} T={T} {name}: tau {tau:.3e}, smallest fp64 margin {float(r64['margin'].min()):.3e}, undecided {undecided:.4f}")
        assert undecided <= 0.02


def test_library_has_the_entry_points_and_refuses_on_the_host():
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 147
    for name in ("amp_dwconv_layer_norm_c_causal", "amp_fvq_encode_ex", "amp_fvq_decode_add", "amp_semantic_prepare"):
        assert hasattr(L, name)
    fake = ctypes.c_void_p(4096)                               # never dereferenced: each call below is refused before any launch
    assert L.amp_fvq_encode_ex(None, fake, 8, None, 1, 8, 1, fake, None, None, None, None) == _lib.AMP_ERR_INVALID
    assert L.amp_fvq_decode_add(None, fake, 1, 1, 8, None, fake, None) == _lib.AMP_ERR_INVALID
    assert L.amp_semantic_prepare(fake, None, None, 1, 3, 1024, 4, fake, None) == _lib.AMP_ERR_INVALID          # T < factor
    assert b"shorter than one pooling window" in L.amp_last_error()
    assert L.amp_semantic_prepare(fake, None, None, 1, 8, 1024, 0, fake, None) == _lib.AMP_ERR_INVALID
    assert L.amp_semantic_prepare(None, None, None, 1, 8, 1024, 2, fake, None) == _lib.AMP_ERR_INVALID
    assert L.amp_semantic_prepare(fake, None, None, 1, 8, 1024, 2, fake.value, None) == _lib.AMP_ERR_INVALID    # out aliases hidden
    for K, dil, C_ in ((3, 1, 64), (7, 2, 64), (7, 1, 1025), (5, 1, 64)):
        assert L.amp_dwconv_layer_norm_c_causal(fake, fake, fake, K, dil, fake, fake, None, 1, C_, 8, 1e-6, 0, ctypes.c_void_p(8192), None) \
            == _lib.AMP_ERR_INVALID, (K, dil, C_)
    assert L.amp_dwconv_layer_norm_c_causal(fake, fake, fake, 7, 1, fake, fake, None, 1, 64, 8, 1e-6, 0, fake, None) == _lib.AMP_ERR_INVALID   # y aliases x


def test_refusals_before_any_launch():
    from amphion_amd.models.codec.dualcodec.dualcodec import model_codec as M

    with pytest.raises(NotImplementedError):
        M.ResidualVectorQuantize(64, n_codebooks=2, codebook_dim=[8, 4])
    assert M.ResidualVectorQuantize(64, n_codebooks=2, codebook_dim=[8, 8]).codebook_dim == [8, 8]
    with pytest.raises(NotImplementedError):
        M.DAC(encoder_dim=8, encoder_rates=[2], decoder_dim=16, decoder_rates=[2], distill=True)
    with pytest.raises(NotImplementedError):
        M.ConvNeXtBlock(64, 2048, adanorm_num_embeddings=4)
    with pytest.raises(AssertionError):
        M.DualCodec(**dict(R.small_hp(True), decode_semantic_for_codec=False))          # convnext_dim must then be 1024
    hp = R.small_hp(True)
    m = M.DualCodec(**hp)
    wave, feats = R.model_inputs(hp, 9)
    codes = torch.zeros(2, 1, 9, dtype=torch.int64)
    assert m.training
    for call in (lambda: m.encode(wave, semantic_repr=feats), lambda: m.semantic_quantize(feats), lambda: m.decode_from_codes(codes, None),
                 lambda: m(wave, semantic_repr=feats), lambda: m.dac.encode(wave), lambda: m.dac.quantizer(torch.zeros(1, 1024, 4)),
                 lambda: m.semantic_vq.quantizers[0](torch.zeros(1, 64, 4))):
        with pytest.raises(NotImplementedError):
            call()
    m.eval()
    for call in (lambda: m.encode(wave, semantic_repr=feats[:, :-1]), lambda: m.semantic_quantize(feats[0]),
                 lambda: m.dac.quantizer(torch.zeros(1, 64, 4)), lambda: m.dac.quantizer.from_codes(torch.zeros(2, 4, 9, dtype=torch.int64)),
                 lambda: M.prepare_semantic_features(torch.zeros(1, 3, 1024), factor=4), lambda: m.encode(wave)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        m.decode_from_codes(codes.float(), None)
    for call in (lambda: m.encode(wave, semantic_repr=feats), lambda: m.decode_from_codes(codes, None), lambda: m.convnext_encoder[1](torch.zeros(1, 64, 4)),
                 lambda: M.prepare_semantic_features(torch.zeros(1, 8, 1024))):
        with pytest.raises(RuntimeError):
            call()                                                                      # host tensors: no CPU fallback


def test_package_imports_no_optional_third_party_module():
    pkg = os.path.join(ROOT, "amphion_amd", "models", "codec", "dualcodec")
    pat = re.compile(r"^\s*(import|from)\s+(easydict|audiotools|einops)\b", re.M)
    for root, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(".py"):
                assert not pat.search(open(os.path.join(root, fn)).read()), fn
