"""CPU checks of the SpeechTokenizer feature: the restatement of tests/speechtokenizer_ref.py against the golden outputs of the real reference
classes (tests/golden/make_golden_speechtokenizer.py), the state_dict key list, the new ABI and its host-side refusals, the drop-ins' refusals,
and that the fp64 reference alone decides the quantizer tests' frames for the inputs the GPU tests use."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import speechtokenizer_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SAMPLES = (1, 47, 48, 49, 480)
QUANT_SHAPES = ((8, 5, 4), (32, 64, 8), (1024, 1024, 8))
QUANT_T = (1, 31, 33, 65)
INVALID, HIP, UNSUPPORTED = -1, -3, -4


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_speechtokenizer.npz"))


@pytest.fixture(scope="module")
def sd(gold):
    return R.synth_state_dict(R.small_hp(), int(gold["seed"]))


def close(a, b, rel=2e-5):
    """the restatement against the reference's fp32: two evaluations in different operation orders, within the fp32 class's own rounding"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return a.shape == b.shape and float((a - b).abs().max()) <= rel * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("n", SAMPLES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_matches_the_reference(gold, sd, n, dtype):
    hp = R.small_hp()
    x = torch.from_numpy(gold[f"x_{n}"])
    frames = -(-n // R.hop(hp))
    r = R.model_forward(sd, hp, x, dtype)
    codes = torch.from_numpy(gold[f"codes_{n}"]).long()
    assert tuple(codes.shape) == (hp["n_q"], 2, frames)
    assert torch.equal(r["codes"], codes)
    assert close(r["e"], gold[f"z_{n}"])
    assert close(r["o"], gold[f"fwd_o_{n}"]) and gold[f"fwd_o_{n}"].shape == (2, 1, frames * R.hop(hp))
    assert close(r["feature"], gold[f"fwd_feat_{n}"]) and gold[f"fwd_feat_{n}"].shape == (2, frames, hp["semantic_dimension"])
    assert close(R.model_decode(sd, hp, codes, dtype), gold[f"dec_{n}"])
    assert close(gold[f"dec_{n}"], gold[f"fwd_o_{n}"])
    assert gold[f"fwd_commit_{n}"].shape == () and float(gold[f"fwd_commit_{n}"]) == 0.0


def test_encode_quirk_and_partial_levels(gold, sd):
    """encode(st = 1) starts level 1 from the WHOLE latent: its codes are not rows 1.. of the full walk"""
    hp = R.small_hp()
    z = torch.from_numpy(gold["z_480"])
    cbs = R.codebooks_of(sd, hp)
    st1 = torch.from_numpy(gold["codes_st1_480"]).long()
    assert tuple(st1.shape) == (3, 2, 10)
    assert torch.equal(R.evq_forward(cbs, z, torch.float64, 1, 4)["codes"], st1)
    assert not torch.equal(st1, torch.from_numpy(gold["codes_480"]).long()[1:])
    nq2 = torch.from_numpy(gold["codes_nq2_480"]).long()
    assert torch.equal(nq2, torch.from_numpy(gold["codes_480"]).long()[:2])
    assert close(R.model_decode(sd, hp, st1, torch.float64, st=1), gold["dec_st1_480"])


def test_state_dict_keys(sd):
    from amphion_amd.models.codec.speechtokenizer import SpeechTokenizer

    with open(os.path.join(GOLDEN, "keys_speechtokenizer.json")) as f:
        ref = json.load(f)
    hp = R.small_hp()
    m = SpeechTokenizer(hp)
    assert list(m.state_dict()) == ref == list(R.param_shapes(hp))
    assert all(tuple(v.shape) == tuple(R.param_shapes(hp)[k]) for k, v in m.state_dict().items())
    m.load_state_dict(sd)
    back = m.state_dict()
    assert list(back) == ref and all(torch.equal(back[k], sd[k]) for k in ref)
    for k in ("inited", "cluster_size", "embed", "embed_avg"):
        assert f"quantizer.vq.layers.3._codebook.{k}" in back
    assert "encoder.model.13.lstm.weight_hh_l1_reverse" in back and "decoder.model.1.lstm.weight_ih_l0" in back
    # the recipe's keys are the same names at other shapes
    assert len(R.param_shapes(R.recipe_hp())) == len(ref) + 4 * 4


def test_drop_in_refusals():
    from amphion_amd.models.codec.speechtokenizer import SpeechTokenizer
    from amphion_amd.models.codec.speechtokenizer.modules import SConv1d, SEANetDecoder, SEANetEncoder, SEANetResnetBlock, SLSTM
    from amphion_amd.models.codec.speechtokenizer.modules.quantization import ResidualVectorQuantizer, VectorQuantization

    with pytest.raises(NotImplementedError):
        SEANetEncoder(activation="Snake")
    with pytest.raises(NotImplementedError):
        SEANetDecoder(norm="time_group_norm")
    with pytest.raises(NotImplementedError):
        SEANetEncoder(causal=True)
    with pytest.raises(NotImplementedError):
        SConv1d(4, 4, 3, pad_mode="constant")
    with pytest.raises(NotImplementedError):
        SEANetResnetBlock(8, norm="layer_norm")
    with pytest.raises(NotImplementedError):
        VectorQuantization(8, 16, codebook_dim=4)
    m = SpeechTokenizer(R.small_hp())
    assert m.training
    x = torch.zeros(1, 1, 48)
    for call in (lambda: m.encoder(x), lambda: m.decoder(torch.zeros(1, 32, 1)), lambda: m.quantizer(torch.zeros(1, 32, 1)),
                 lambda: SLSTM(8).train()(torch.zeros(1, 8, 2)), lambda: m.encode(x), lambda: m(x)):
        with pytest.raises(NotImplementedError):
            call()
    # a codebook that still waits for its k-means initialisation
    q = ResidualVectorQuantizer(dimension=8, n_q=2, bins=4).eval()
    assert float(q.vq.layers[0]._codebook.inited) == 0.0
    with pytest.raises(NotImplementedError):
        q.encode(torch.zeros(1, 8, 3))
    with pytest.raises(ValueError, match="asks for level 1"):
        q(torch.zeros(1, 8, 3), n_q=1, layers=[1])
    with pytest.raises(ValueError, match="no residual argument"):
        SConv1d(4, 8, 4, stride=2, norm="weight_norm").run(torch.zeros(1, 4, 8), res=torch.zeros(1, 8, 4))
    # a host tensor is refused by name, not run on the CPU
    m.eval()
    with pytest.raises(RuntimeError):
        m.encoder(x)


def test_abi_version_and_symbols():
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 149
    for name in ("amp_elu_pad", "amp_lstm_create", "amp_lstm_workspace_bytes", "amp_lstm_out_channels", "amp_lstm_forward", "amp_lstm_recur",
                 "amp_lstm_destroy", "amp_evq_create", "amp_evq_encode", "amp_evq_decode", "amp_evq_check", "amp_evq_destroy"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    # NULL handles: -1 or 0, like amp_aa_unit_*
    assert L.amp_lstm_out_channels(None) == -1 and L.amp_lstm_workspace_bytes(None, 1, 1) == 0
    assert L.amp_lstm_forward(None, None, 1, 1, None, None, 0, None) == INVALID
    assert L.amp_lstm_recur(None, 0, None, 1, 1, None, None, None, None) == INVALID
    assert L.amp_evq_encode(None, None, 1, 1, 0, 1, None, None, None, None) == INVALID
    assert L.amp_evq_decode(None, None, 1, 0, 1, 1, None, None) == INVALID
    assert L.amp_evq_check(None, None) == INVALID
    L.amp_lstm_destroy(None)
    L.amp_evq_destroy(None)


def _lstm_create(In, H, layers, bidir, skip, null_at=None):
    from amphion_amd import _lib

    ndir = 2 if bidir else 1
    n = max(layers, 1) * ndir
    Hc, Ic = max(1, min(H, 8)), max(1, min(In, 8))          # refusals come before any weight is read
    keep = [np.zeros((4 * Hc, max(Ic, ndir * Hc)), np.float32) for _ in range(n)]
    arr = lambda: (ctypes.c_void_p * n)(*[None if i == null_at else k.ctypes.data for i, k in enumerate(keep)])  # noqa: E731
    h = ctypes.c_void_p()
    rc = _lib.lib().amp_lstm_create(In, H, layers, int(bidir), int(skip), arr(), arr(), arr(), arr(), ctypes.byref(h))
    return rc, h


def test_lstm_create_refusals_need_no_device():
    from amphion_amd import _lib

    L = _lib.lib()
    for args, want in (((8, 1025, 1, 0, 0), UNSUPPORTED), ((2049, 8, 1, 0, 0), UNSUPPORTED), ((8, 8, 5, 0, 0), UNSUPPORTED),
                       ((0, 8, 1, 0, 0), INVALID), ((8, 0, 1, 0, 0), INVALID), ((8, 8, 0, 0, 0), INVALID), ((4, 8, 1, 1, 1), INVALID)):
        rc, _ = _lstm_create(*args)
        assert rc == want, (args, rc, L.amp_last_error())
        assert b"amp_lstm_create" in L.amp_last_error()
    rc, _ = _lstm_create(8, 8, 2, 1, 1, null_at=3)
    assert rc == INVALID
    h = ctypes.c_void_p()
    assert L.amp_lstm_create(8, 8, 1, 0, 0, None, None, None, None, ctypes.byref(h)) == INVALID
    # inside the coverage the host has no objection: the only possible failure is the absent device
    rc, h = _lstm_create(8, 8, 2, 1, 1)
    assert rc in (0, HIP), L.amp_last_error()
    if rc == 0:
        L.amp_lstm_destroy(h)
    else:
        assert b"no HIP device" in L.amp_last_error()


def test_evq_create_refusals_need_no_device():
    from amphion_amd import _lib

    L = _lib.lib()

    def create(D, K, N, null_at=None, value=0.0):
        n = max(N, 1)
        keep = [np.full((max(1, min(K, 4)) * max(1, min(D, 4)),), value, np.float32) for _ in range(n)]
        arr = (ctypes.c_void_p * n)(*[None if i == null_at else k.ctypes.data for i, k in enumerate(keep)])
        h = ctypes.c_void_p()
        return L.amp_evq_create(D, K, N, arr, ctypes.byref(h)), h

    for args, want in (((1025, 4, 1), UNSUPPORTED), ((4, 4097, 1), UNSUPPORTED), ((4, 4, 33), UNSUPPORTED), ((0, 4, 1), INVALID),
                       ((4, 0, 1), INVALID), ((4, 4, 0), INVALID)):
        rc, _ = create(*args)
        assert rc == want, (args, rc, L.amp_last_error())
        assert b"amp_evq_create" in L.amp_last_error()
    assert create(4, 4, 2, null_at=1)[0] == INVALID
    assert create(4, 4, 1, value=float("inf"))[0] == INVALID
    h = ctypes.c_void_p()
    assert L.amp_evq_create(4, 4, 1, None, ctypes.byref(h)) == INVALID
    rc, h = create(4, 4, 2)
    assert rc in (0, HIP), L.amp_last_error()
    if rc == 0:
        L.amp_evq_destroy(h)
    else:
        assert b"no HIP device" in L.amp_last_error()


def test_elu_pad_refusals_need_no_device():
    """every refusal is decided before the launch: the pointers are never followed"""
    from amphion_amd import _lib

    L = _lib.lib()
    x, y = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    for args, want in (((x, 1, 1, 4, -1, 0, 1, 1.0, y, None), INVALID), ((x, 1, 1, 4, 0, -2, 0, 1.0, y, None), INVALID),
                       ((x, 0, 1, 4, 0, 0, 1, 1.0, y, None), INVALID), ((x, 1, 0, 4, 0, 0, 1, 1.0, y, None), INVALID),
                       ((x, 1, 1, 0, 1, 1, 1, 1.0, y, None), INVALID), ((None, 1, 1, 4, 0, 0, 1, 1.0, y, None), INVALID),
                       ((x, 1, 1, 4, 0, 0, 1, 1.0, None, None), INVALID), ((x, 1, 1, 4, 1, 1, 1, 1.0, x, None), INVALID),
                       ((x, 1, 1, 2 ** 30, 1, 0, 1, 1.0, y, None), UNSUPPORTED), ((x, 2 ** 15, 2 ** 15, 2 ** 20, 0, 0, 1, 1.0, y, None), UNSUPPORTED)):
        assert L.amp_elu_pad(*args) == want, (args[1:8], L.amp_last_error())
        assert b"amp_elu_pad" in L.amp_last_error()


@pytest.mark.parametrize("D,K,N", QUANT_SHAPES)
def test_fp64_reference_decides_the_quantizer_frames(D, K, N):
    """the condition of the GPU quantizer tests: at most 5 % of the frames undecided at the last level, for the inputs they use"""
    for s in (1.0, 0.05):
        for T in QUANT_T:
            if s != 1.0 and T != 33:
                continue
            cbs, z = R.quantizer_case(D, K, N, T, s)
            r64, _, tau, decided = R.margin_rule(cbs, z)
            undecided = 1.0 - float(decided[-1].double().mean())
            print(f"evq D={D} K={K} N={N} T={T} s={s}: tau = {tau:.3g}, undecided at the last level = {100 * undecided:.2f} %")
            assert undecided <= 0.05, (D, K, N, T, s, tau, undecided)
            assert not bool((decided[1:] & ~decided[:-1]).any())          # a frame is decided at a level only if every level up to it is


def test_plain_encode_is_the_reference_encode(gold, sd):
    """the yardstick the measurement tool times runs the reference's ops only, and gives the reference's codes"""
    hp = R.small_hp()
    cbs = R.codebooks_of(sd, hp)
    z = torch.from_numpy(gold["z_480"])
    assert torch.equal(R.rvq_encode_plain(cbs, z), torch.from_numpy(gold["codes_480"]).long())
    assert torch.equal(R.rvq_encode_plain(cbs, z, 1, 4), torch.from_numpy(gold["codes_st1_480"]).long())


def test_stack_keys_with_true_skip():
    """two residual layers per ratio and true_skip: the drop-ins' keys are the restatement's (no shortcut convs)"""
    from amphion_amd.models.codec.speechtokenizer.modules import SEANetDecoder, SEANetEncoder

    hp = R.stack_hp()
    kw = dict(dimension=16, n_filters=8, n_residual_layers=2, ratios=[3, 2], lstm=1, true_skip=True, dilation_base=2)
    for which, cls in (("encoder", SEANetEncoder), ("decoder", SEANetDecoder)):
        sd = R.synth_stack_state_dict(hp, which, 3)
        m = cls(**kw)
        assert list(m.state_dict()) == list(sd) and not any("shortcut" in k for k in sd)
        m.load_state_dict(sd)


def test_pad_rule_of_the_restatement():
    """pad1d's small-input rule, spelled out: T = 1 with pads (1, 1) is [0, a, 0]; T = 2 with pads (3, 10) reflects the zero extension"""
    a = torch.tensor([[[5.0]]])
    assert R.pad1d_reflect(a, 1, 1).flatten().tolist() == [0.0, 5.0, 0.0]
    b = torch.tensor([[[1.0, 2.0]]])
    out = R.pad1d_reflect(b, 3, 10).flatten().tolist()
    assert len(out) == 15 and out[:5] == [0.0, 0.0, 2.0, 1.0, 2.0] and out[5:12] == [0.0] * 7
    assert R.sconv_pads(47, 8, 4, 1) == (2, 2 + 1) and R.sconv_pads(1, 7, 1, 1) == (3, 3)
