"""CPU checks of the semantic tokenizers: the restatement of tests/tokenizer_ref.py against the golden outputs of the real reference classes
(tests/golden/make_golden_tokenizers.py), the three state_dict key lists, the new ABI and its host-side refusals, the drop-ins' refusals, and
that the fp64 reference alone decides the quantizer frames of the inputs the GPU tests use."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import speechtokenizer_ref as S  # noqa: E402
import tokenizer_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
INVALID, HIP, UNSUPPORTED = -1, -3, -4
UNDECIDED_CAP = 0.02


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_tokenizers.npz"))


@pytest.fixture(scope="module")
def nets(gold):
    return R.golden_models(int(gold["seed"]))


def close(a, b, rel=2e-5):
    """the restatement against the reference's fp32: two evaluations in different operation orders, within the fp32 class's own rounding"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return a.shape == b.shape and float((a - b).abs().max()) <= rel * max(1.0, float(b.abs().max()))


def codes_of(gold, key):
    return torch.from_numpy(gold[key]).long()


@pytest.mark.parametrize("T", R.GOLDEN_LENGTHS)
def test_repcodec_restatement_matches_the_reference(gold, nets, T):
    x = R.golden_inputs(T)["rep"]
    for K in (64, 8192):
        hp, sd = nets[f"rep{K}"]
        r = R.repcodec_forward(sd, hp, x, torch.float64)
        codes = codes_of(gold, f"rep{K}_codes_{T}")
        assert tuple(codes.shape) == (2, T) and torch.equal(r["codes"][0], codes)
        assert close(r["z"], gold[f"rep_z_{T}"])
        if K == 64:
            assert close(r["x_rec"], gold[f"rep_rec_{T}"]) and gold[f"rep_rec_{T}"].shape == (2, T, 64)


@pytest.mark.parametrize("T", R.GOLDEN_LENGTHS)
def test_coco_restatement_matches_the_reference(gold, nets, T):
    hp, sd = nets["coco"]
    x = R.golden_inputs(T)
    r = R.coco_forward(sd, hp, dict(whisper=x["whisper"], chroma=x["chroma"]), torch.float64)
    Tq = ((T - 1) // 2 + 1 - 1) // 2 + 1
    codes = codes_of(gold, f"coco_codes_{T}")
    assert tuple(codes.shape) == (2, Tq) and torch.equal(r["codes"][0], codes)
    assert close(r["z"], gold[f"coco_z_{T}"]) and close(r["zq"].transpose(1, 2), gold[f"coco_zq_{T}"])
    assert close(r["whisper"], gold[f"coco_whisper_{T}"]) and gold[f"coco_whisper_{T}"].shape == (2, T, 64)
    assert close(r["chroma"], gold[f"coco_chroma_{T}"]) and gold[f"coco_chroma_{T}"].shape == (2, T, 24)
    # where the up-sampled length 4 T' falls short of T the last frame is repeated; where it is longer it is cropped
    assert r["dec"].shape[2] == Tq and r["up"].shape[2] == T


@pytest.mark.parametrize("T", R.GOLDEN_LENGTHS)
def test_vevo_restatement_matches_the_reference(gold, nets, T):
    hp, sd = nets["vevo"]
    x = R.golden_inputs(T)["vevo"]
    r = R.vevo_forward(sd, hp, x, torch.float64)
    codes = codes_of(gold, f"vevo_codes_{T}")
    assert tuple(codes.shape) == (1, 2, T) and torch.equal(r["codes"], codes)
    assert close(r["z"], gold[f"vevo_z_{T}"])
    assert close(r["y"], gold[f"vevo_y_{T}"])
    assert close(r["loss"], gold[f"vevo_loss_{T}"]) and close(r["perplexity"], gold[f"vevo_perplexity_{T}"])


def test_fp64_reference_decides_the_golden_frames(gold, nets):
    """the condition of the GPU tests: at most 2 % of the (level, frame) pairs undecided, on the golden latents"""
    for T in R.GOLDEN_LENGTHS:
        for K in (64, 8192):
            hp, sd = nets[f"rep{K}"]
            _, _, tau, decided = R.fvq_margin_rule(sd, hp, torch.from_numpy(gold[f"rep_z_{T}"]))
            und = 1.0 - float(decided.double().mean())
            print(f"repcodec K={K} T={T}: tau = {tau:.3g}, undecided {100 * und:.2f} %")
            assert und <= UNDECIDED_CAP, (K, T, tau, und)
        hp, sd = nets["vevo"]
        _, _, tau, decided = S.margin_rule(R.vevo_codebooks(sd, hp), torch.from_numpy(gold[f"vevo_z_{T}"]))
        assert 1.0 - float(decided.double().mean()) <= UNDECIDED_CAP, (T, tau)


@pytest.mark.parametrize("K", [32, 512, 8192, 16384])
def test_unit_norm_codebooks_leave_few_frames_undecided(K):
    """random unit-norm codebooks with d = 8 against 6 000 random latents: the fp64 reference alone stays far inside the 2 % cap"""
    hp = dict(R.small_repcodec_hp(K), hidden_size=8)
    sd = {R.QP + "0.codebook.weight": torch.randn(K, 8, generator=torch.Generator().manual_seed(K))}
    z = torch.randn(2, 8, 3000, generator=torch.Generator().manual_seed(K + 1))
    _, _, tau, decided = R.fvq_margin_rule(sd, hp, z)
    und = 1.0 - float(decided.double().mean())
    print(f"K={K}: tau = {tau:.3g}, undecided {100 * und:.3f} %")
    assert und <= 0.005, (K, tau, und)


def test_state_dict_keys(nets):
    from amphion_amd.models.codec.coco.rep_coco_model import CocoContent, CocoContentStyle, CocoStyle
    from amphion_amd.models.codec.kmeans.repcodec_model import RepCodec
    from amphion_amd.models.codec.vevo.vevo_repcodec import VevoRepCodec

    def ref(name):
        with open(os.path.join(GOLDEN, f"keys_{name}.json")) as f:
            return json.load(f)

    hp = dict(R.small_repcodec_hp(), downsample_scale=2)
    m = RepCodec(**hp)
    assert list(m.state_dict()) == ref("repcodec") == list(R.repcodec_param_shapes(hp))
    assert all(tuple(v.shape) == tuple(R.repcodec_param_shapes(hp)[k]) for k, v in m.state_dict().items())
    assert "down.weight" in ref("repcodec") and "encoder.0.embed.weight" in ref("repcodec") and "encoder.1.bias" in ref("repcodec")
    hp, sd = nets["rep64"]
    m = RepCodec(**hp)
    m.load_state_dict(sd)
    assert list(m.state_dict()) == list(sd) and not any(k.startswith("down.") for k in sd)
    # cfg: vocos_intermediate_dim and vocos_num_layers are read only when cfg has vocos_dim (the reference's quirk)
    from types import SimpleNamespace
    m = RepCodec(hidden_size=16, vocos_dim=16, vocos_intermediate_dim=24, vocos_num_layers=1, codebook_size=4,
                 cfg=SimpleNamespace(vocos_intermediate_dim=99, vocos_num_layers=7, codebook_size=8))
    assert (m.vocos_intermediate_dim, m.vocos_num_layers, m.codebook_size) == (24, 1, 8)
    m = RepCodec(hidden_size=16, codebook_size=4, cfg=SimpleNamespace(vocos_dim=16, vocos_intermediate_dim=32, vocos_num_layers=2))
    assert (m.vocos_dim, m.vocos_intermediate_dim, m.vocos_num_layers) == (16, 32, 2)

    hp, sd = nets["coco"]
    cfg = R.coco_cfg(hp)
    m = CocoContentStyle(cfg=cfg)
    assert list(m.state_dict()) == ref("coco") == list(sd)
    assert all(tuple(v.shape) == tuple(sd[k].shape) for k, v in m.state_dict().items())
    m.load_state_dict(sd)
    assert "downsample_layers.2.weight" in sd and "upsample_layers.0.bias" in sd
    assert list(CocoContent(cfg).state_dict()) == list(R.coco_param_shapes(hp, chroma=False))
    assert list(CocoStyle(cfg).state_dict()) == list(R.coco_param_shapes(hp, whisper=False))
    only = CocoContentStyle(cfg=cfg, construct_only_for_quantizer=True)
    assert list(only.state_dict()) == list(R.coco_param_shapes(hp, only_quantizer=True)) and not hasattr(only, "decoder")
    rate8 = CocoStyle(R.coco_cfg(R.small_coco_hp(rate=8)))
    assert "downsample_layers.4.weight" in rate8.state_dict() and len(rate8.downsample_layers) == 6

    hp, sd = nets["vevo"]
    m = VevoRepCodec(**hp)
    assert list(m.state_dict()) == ref("vevo_repcodec") == list(sd)
    assert all(tuple(v.shape) == tuple(sd[k].shape) for k, v in m.state_dict().items())
    m.load_state_dict(sd)
    assert tuple(m.quantizer.codebook.layers[0].embed.shape) == (64, 32)


def test_drop_in_refusals(nets):
    from amphion_amd.models.codec.coco.rep_coco_model import CocoContentStyle
    from amphion_amd.models.codec.kmeans.repcodec_model import RepCodec
    from amphion_amd.models.codec.vevo import vevo_repcodec as VR

    with pytest.raises(NotImplementedError):
        VR.VevoRepCodec(**dict(R.small_vevo_hp(), enc_strides=(2, 1)))
    with pytest.raises(NotImplementedError):
        VR.VevoRepCodec(**dict(R.small_vevo_hp(), dec_strides=(1, 2)))
    with pytest.raises(NotImplementedError):
        VR.ResidualUnit(8, 8, nonlinear_activation="ReLU")
    rep = RepCodec(**nets["rep64"][0])
    coco = CocoContentStyle(cfg=R.coco_cfg(nets["coco"][0]))
    vevo = VR.VevoRepCodec(**nets["vevo"][0])
    x = R.golden_inputs(3)
    assert rep.training and coco.training and vevo.training
    for call in (lambda: rep(x["rep"]), lambda: rep.quantize(x["rep"]), lambda: coco(x["whisper"], x["chroma"]),
                 lambda: coco.quantize(x["whisper"], x["chroma"]), lambda: vevo(x["vevo"]), lambda: vevo.encoder(x["vevo"]),
                 lambda: vevo.quantizer.codebook.forward_index(x["vevo"].transpose(1, 2))):
        with pytest.raises(NotImplementedError):
            call()
    rep.eval(), coco.eval(), vevo.eval()
    # a host tensor is refused by name, not run on the CPU
    for call in (lambda: rep.quantize(x["rep"]), lambda: coco.quantize(x["whisper"], x["chroma"]), lambda: vevo(x["vevo"]),
                 lambda: vevo.projector(x["vevo"]), lambda: vevo.quantizer.inference(x["vevo"])):
        with pytest.raises(RuntimeError):
            call()
    for call in (lambda: rep.quantize(x["rep"][0]), lambda: coco.input_projection(x["whisper"]), lambda: vevo.quantizer.codebook.forward_index(x["chroma"])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match="initial"):
        vevo.quantizer.decode(torch.zeros(1, 3, dtype=torch.int64))


def test_abi_version_and_symbols():
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 150
    for name in ("amp_dsconv_create", "amp_dsconv_out_len", "amp_dsconv_workspace_bytes", "amp_dsconv_forward", "amp_dsconv_destroy", "amp_gelu"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    assert [L.amp_dsconv_out_len(None, T) for T in range(1, 10)] == [1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert [L.amp_dsconv_out_len(None, T) for T in range(1, 10)] == [(T + 2 - 3) // 2 + 1 for T in range(1, 10)]     # Conv1d's own formula
    assert L.amp_dsconv_out_len(None, 0) == 0 and L.amp_dsconv_workspace_bytes(None, 1, 1) == 0
    L.amp_dsconv_destroy(None)


def test_dsconv_refusals_need_no_device():
    from amphion_amd import _lib

    L = _lib.lib()
    w = np.zeros((4, 4, 3), np.float32)
    b = np.zeros((4,), np.float32)
    h = ctypes.c_void_p()
    wp, bp = ctypes.c_void_p(w.ctypes.data), ctypes.c_void_p(b.ctypes.data)
    for args in ((0, 4, wp, bp, ctypes.byref(h)), (4, 0, wp, bp, ctypes.byref(h)), (-1, 4, wp, bp, ctypes.byref(h)), (4, 4, None, bp, ctypes.byref(h)),
                 (4, 4, wp, bp, None)):
        assert L.amp_dsconv_create(*args) == INVALID, L.amp_last_error()
        assert b"amp_dsconv_create" in L.amp_last_error()
    w[1, 2, 1] = np.inf
    assert L.amp_dsconv_create(4, 4, wp, bp, ctypes.byref(h)) == INVALID and b"non-finite" in L.amp_last_error()
    w[1, 2, 1] = np.nan
    assert L.amp_dsconv_create(4, 4, wp, None, ctypes.byref(h)) == INVALID
    w[1, 2, 1] = 0.0
    # inside the coverage the host has no objection: the only possible failure is the absent device
    rc = L.amp_dsconv_create(4, 4, wp, None, ctypes.byref(h))
    assert rc in (0, HIP), L.amp_last_error()
    if rc == 0:
        L.amp_dsconv_destroy(h)
    else:
        assert b"no HIP device" in L.amp_last_error()
    x, y = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    assert L.amp_dsconv_forward(None, x, 1, 4, 0, None, 0, y, None) == INVALID and b"amp_dsconv_forward" in L.amp_last_error()


def test_gelu_refusals_need_no_device():
    """every refusal is decided before the launch: the pointers are never followed"""
    from amphion_amd import _lib

    L = _lib.lib()
    x, y = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    for args, want in (((None, 4, y, None), INVALID), ((x, 4, None, None), INVALID), ((x, 0, y, None), INVALID), ((x, -3, y, None), INVALID),
                       ((ctypes.c_void_p(4100), 2 ** 40, y, None), UNSUPPORTED), ((x, 2 ** 42, y, None), UNSUPPORTED)):
        assert L.amp_gelu(*args) == want, (args[1], L.amp_last_error())
        assert b"amp_gelu" in L.amp_last_error()


def test_plain_quantize_is_the_reference_quantize(gold, nets):
    """the yardstick the measurement tool times runs the reference's ops only, and gives the reference's codes"""
    x = R.golden_inputs(50)
    for K in (64, 8192):
        hp, sd = nets[f"rep{K}"]
        codes, zq = R.repcodec_quantize_plain(sd, hp, x["rep"])
        assert torch.equal(codes[0], codes_of(gold, f"rep{K}_codes_50")) and tuple(zq.shape) == (2, 50, 64)
    hp, sd = nets["coco"]
    codes, zq = R.coco_quantize_plain(sd, hp, x["whisper"], x["chroma"])
    assert torch.equal(codes[0], codes_of(gold, "coco_codes_50")) and close(zq, gold["coco_zq_50"])
