"""DualCodec's DAC decoder on the MI355X (csrc/tconv_f16x3.hip, the amp_tconv_* host side in csrc/codec.hip and the drop-in modules) against the
fp64 restatement of tests/dac_ref.py and the golden outputs of the real reference classes.

Op bound (both arithmetics), derived in tests/test_gpu_codec.py for the strided-conv op and restated in dac_ref.tconv_bound with conv_transpose1d in
place of conv1d:  2e-6 (|w| * |snake(x)| + |b|) + 3e-7 |ref| + |w| * d_snake(x)  per element.  The fused f16x3 launch is NOT bit-identical to
amp_snake -> transposed conv in f16x3 (one GEMM with K = 2 cin against the conv kernel's chunk-by-chunk walk); under AMP_PRECISION=f32 the handle
IS that sequence, which the f32 test pins bit for bit.
Module bound: max(1e-4 max|pre-tanh fp64|, 4 e32), e32 the fp32 CPU restatement's own error (printed); + e32 against the golden (written in fp32).
Every case prints its worst error / bound."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import codec_ref as C  # noqa: E402
import dac_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden")
OP_LENGTHS = (1, 2, 63, 64, 65, 130)


def op_state_dict(cin, cout, s, seed):
    shapes = {"a.alpha": (1, cin, 1)}
    D._wnT(shapes, "c.", cin, cout, 2 * s)
    return C._synth(shapes, seed)


def make_op(cin, cout, s, op, sd, fusion=None, padding=None):
    from amphion_amd import _lib
    from amphion_amd.models.codec.amphion_codec.codec import _TransposedConv

    conv = _TransposedConv(cin, cout, s, D.block_padding(s) if padding is None else padding, op)
    conv.load_state_dict({k[2:]: v for k, v in sd.items() if k.startswith("c.")})
    conv = conv.to(DEV)
    if fusion is not None:
        _lib.check(_lib.lib().amp_set_tconv_fusion(fusion))
    try:
        conv._handle(torch.device(DEV))
    finally:
        _lib.check(_lib.lib().amp_set_tconv_fusion(-1))
    return conv


def op_check(conv, sd, x, with_alpha=True):
    """worst error / bound of one call; asserts the shape against amp_tconv_out_len and the closed form"""
    from amphion_amd import _lib

    sd64 = {k: v.double() for k, v in sd.items()}
    s, p, op = conv.stride, conv.padding, conv.output_padding
    alpha = sd["a.alpha"].to(DEV) if with_alpha else None
    y = conv(x.to(DEV), alpha).cpu().double()
    ref, tol = D.tconv_bound(C.folded(sd64, "c."), sd64["c.bias"], sd64["a.alpha"] if with_alpha else None, x.double(), s, p, op)
    T = x.shape[2]
    assert y.shape == ref.shape and y.shape[2] == D.tconv_out_len(T, s, p, op) == _lib.lib().amp_tconv_out_len(conv._handle(torch.device(DEV)), T)
    assert torch.isfinite(y).all()
    return float(((y - ref).abs() / tol).max())


@pytest.mark.parametrize("s", [2, 3, 4, 5, 8])
def test_tconv_vs_fp64(conv_precision, s):
    worst = 0.0
    for op in sorted({0, s % 2}):
        sd = op_state_dict(64, 32, s, 200 + 2 * s + op)
        conv = make_op(64, 32, s, op, sd)
        assert conv.fused(torch.device(DEV)) == (conv_precision == "f16x3")
        for T in OP_LENGTHS:
            x = C.synth_latent(2, 64, T, 10 * s + T + op)
            for with_alpha in (True, False):
                frac = op_check(conv, sd, x, with_alpha)
                worst = max(worst, frac)
                assert frac <= 1.0, (s, op, T, with_alpha, frac)
    from amphion_amd import _lib

    _lib.range_check(DEV)
    print(f"tconv 64->32 s={s} [{conv_precision}]: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("cin,cout,s", [(32, 16, 2), (96, 48, 5), (192, 96, 4), (384, 192, 5), (64, 192, 8)])
def test_tconv_fused_widths(cin, cout, s):
    """fusion forced on: 240 rows (M padded to the row block), the 100-KB window, and 1536 rows (the row-group sweep: groups of 4, 2, 1)"""
    sd = op_state_dict(cin, cout, s, 300 + cin + s)
    conv = make_op(cin, cout, s, s % 2, sd, fusion=1)
    assert conv.fused(torch.device(DEV))
    worst = 0.0
    for T in (1, 65, 130):
        frac = op_check(conv, sd, C.synth_latent(2, cin, T, cin + s + T))
        worst = max(worst, frac)
        assert frac <= 1.0, (cin, cout, s, T, frac)
    print(f"fused tconv {cin}->{cout} s={s}: worst error / bound = {worst:.3f}")


def test_tconv_wide_input_runs_unfused():
    sd = op_state_dict(416, 64, 4, 77)
    conv = make_op(416, 64, 4, 0, sd, fusion=1)
    assert not conv.fused(torch.device(DEV))
    frac = op_check(conv, sd, C.synth_latent(2, 416, 65, 78))
    print(f"unfused tconv 416->64 s=4: error / bound = {frac:.3f}")
    assert frac <= 1.0


@pytest.mark.parametrize("cin,cout,s", [(64, 32, 2), (96, 48, 5), (192, 96, 4)])
def test_tconv_f32_is_snake_then_transposed_conv(cin, cout, s):
    """AMP_PRECISION=f32: the handle and amp_snake -> transposed amp_conv_forward through the op-level modules agree bit for bit (op = 0)"""
    from amphion_amd import _lib
    from amphion_amd.models.codec.amphion_codec.codec import snake
    from amphion_amd.modules.hip_ops import HipConv1d

    sd = op_state_dict(cin, cout, s, 50 + cin)
    _lib.set_precision("f32")
    try:
        conv = make_op(cin, cout, s, 0, sd)
        assert not conv.fused(torch.device(DEV))
        plain = HipConv1d(cin, cout, 2 * s, transposed=True, stride=s, padding=D.block_padding(s))
        plain.load_state_dict({k[2:]: v for k, v in sd.items() if k.startswith("c.")})
        plain = plain.to(DEV)
        alpha = sd["a.alpha"].to(DEV)
        for T in (1, 65, 130):
            x = C.synth_latent(2, cin, T, T).to(DEV)
            assert torch.equal(conv(x, alpha), plain(snake(x, alpha))), (cin, s, T)
            assert torch.equal(conv(x), plain(x)), (cin, s, T)
            assert op_check(conv, sd, x.cpu()) <= 1.0
    finally:
        _lib.set_precision("f16x3")


def test_tconv_fusion_switch():
    """amp_set_tconv_fusion picks the route of handles created afterwards; both routes meet the bound"""
    from amphion_amd import _lib

    sd = op_state_dict(96, 48, 4, 91)
    x = C.synth_latent(2, 96, 130, 92)
    for mode, fused in ((0, False), (1, True), (-1, None)):
        conv = make_op(96, 48, 4, 0, sd, fusion=mode)
        if fused is not None:
            assert conv.fused(torch.device(DEV)) == fused
        frac = op_check(conv, sd, x)
        print(f"tconv fusion mode {mode}: fused {conv.fused(torch.device(DEV))}, error / bound = {frac:.3f}")
        assert frac <= 1.0
    with pytest.raises(_lib.AmpError):
        _lib.check(_lib.lib().amp_set_tconv_fusion(2))


def test_tconv_batch_independence():
    sd = op_state_dict(64, 32, 3, 95)
    conv = make_op(64, 32, 3, 1, sd, fusion=1)
    alpha = sd["a.alpha"].to(DEV)
    x = C.synth_latent(3, 64, 130, 96).to(DEV)
    assert torch.equal(conv(x, alpha)[1], conv(x[1:2].contiguous(), alpha)[0])


def test_tconv_range_guard():
    """an input beyond the f16x3 operand range (|snake(x)| * 16 > 65504) raises AMP_ERR_RANGE through the fused launch; the next check is clean"""
    from amphion_amd import _lib

    sd = op_state_dict(64, 32, 4, 97)
    conv = make_op(64, 32, 4, 0, sd, fusion=1)
    assert conv.fused(torch.device(DEV))
    alpha = sd["a.alpha"].to(DEV)
    x = C.synth_latent(2, 64, 130, 98)
    _lib.range_check(DEV)
    conv(x.to(DEV), alpha)
    _lib.range_check(DEV)
    x[1, 17, 100] = 5000.0
    for a in (alpha, None):
        conv(x.to(DEV), a)
        with pytest.raises(_lib.AmpError) as e:
            _lib.range_check(DEV)
        assert e.value.status == _lib.AMP_ERR_RANGE
    _lib.range_check(DEV)


def test_tconv_refusals():
    from amphion_amd import _lib

    sd = op_state_dict(32, 16, 2, 99)
    for kw in (dict(op=2), dict(op=1, padding=0)):
        with pytest.raises(_lib.AmpError):
            make_op(32, 16, 2, kw["op"], sd, padding=kw.get("padding"))


# ---- modules -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_dac.npz"))


def make_decoder(hp, sd):
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import Decoder

    m = Decoder(**hp)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


_REF = {}


def decoder_reference(tag, hp, sd, x):
    key = (tag, tuple(x.shape))
    if key not in _REF:
        pre = D.decoder_forward(sd, hp, x, torch.float64, pre_tanh=True)
        y64 = torch.tanh(pre)
        e32 = float((D.decoder_forward(sd, hp, x, torch.float32).double() - y64).abs().max())
        _REF[key] = (y64, e32, max(1e-4 * float(pre.abs().max()), 4 * e32))
    return _REF[key]


@pytest.mark.parametrize("s,amphion", [(2, True), (3, True), (3, False), (4, False), (5, True)])
def test_decoder_block_vs_fp64(conv_precision, s, amphion):
    from amphion_amd.models.codec.amphion_codec.codec import DecoderBlock as AmphionBlock
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import DecoderBlock

    cin, cout = (96, 48) if s == 4 else (64, 32)               # 96 -> 48: units of C = 48 (C % 32 != 0: the four launches)
    sd = D.synth_block_state_dict(cin, cout, s, 400 + s)
    blk = (AmphionBlock if amphion else DecoderBlock)(cin, cout, s)
    blk.load_state_dict(sd)
    blk = blk.to(DEV).eval()
    op = s % 2 if amphion else 0
    x = C.synth_latent(2, cin, 33, 401 + s)
    P = {k: v.double() for k, v in sd.items()}
    y64 = D.decoder_block_forward(P, "block.", x.double(), s, op)
    e32 = float((D.decoder_block_forward(sd, "block.", x, s, op).double() - y64).abs().max())
    bound = max(1e-4 * float(y64.abs().max()), 4 * e32)
    y = blk(x.to(DEV)).cpu().double()
    err = float((y - y64).abs().max())
    print(f"DecoderBlock {cin}->{cout} s={s} op={op} [{conv_precision}]: err {err:.3e}, torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert y.shape == y64.shape and y.shape[2] == 33 * s - (s % 2 - op) and err <= bound


@pytest.mark.parametrize("name,T", [("small", 1), ("small", 7), ("small", 33), ("even", 33)])
def test_decoder_vs_fp64_and_golden(conv_precision, gold, name, T):
    hp = D.small_decoder_hp() if name == "small" else D.even_decoder_hp()
    sd = D.synth_decoder_state_dict(hp, int(gold[f"{name}_seed"]))
    x = torch.from_numpy(gold[f"{name}_x_{T}"])
    y64, e32, bound = decoder_reference(name, hp, sd, x)
    y = make_decoder(hp, sd)(x.to(DEV)).cpu().double()
    err, err_g = float((y - y64).abs().max()), float((y - torch.from_numpy(gold[f"{name}_y_{T}"]).double()).abs().max())
    print(f"Decoder {name} T={T} [{conv_precision}]: err vs fp64 {err:.3e}, vs golden {err_g:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert y.shape == y64.shape and err <= bound and err_g <= bound + e32


def test_decoder_recipe_width():
    hp = D.recipe_decoder_hp()
    sd = D.synth_decoder_state_dict(hp, 500)
    x = C.synth_latent(1, hp["input_channel"], 3, 501)
    y64, e32, bound = decoder_reference("recipe", hp, sd, x)
    m = make_decoder(hp, sd)
    y = m(x.to(DEV)).cpu().double()
    err = float((y - y64).abs().max())
    fused = [m.model[1 + i].block[1].fused(torch.device(DEV)) for i in range(4)]
    print(f"Decoder recipe width {tuple(y.shape)}: err vs fp64 {err:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}; fused up-sampling steps {fused}")
    assert y.shape == y64.shape == (1, 1, 3 * 960 - 4) and err <= bound         # the odd rate 5 drops one sample, x 4 after it
    assert fused[0] is False                                                       # cin = 1536 is beyond the fused kernel


def test_encoder_is_the_codec_encoder(gold):
    from amphion_amd.models.codec.amphion_codec.codec import CodecEncoder
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import Encoder

    hp = D.small_dac_encoder_hp()
    sd = D.synth_dac_encoder_state_dict(hp, int(gold["enc_seed"]))
    chp = dict(d_model=hp["d_model"], up_ratios=hp["strides"], out_channels=hp["d_latent"], use_tanh=False)
    enc, ref = Encoder(**hp), CodecEncoder(**chp)
    enc.load_state_dict(sd)
    ref.load_state_dict(sd)
    enc, ref = enc.to(DEV).eval(), ref.to(DEV).eval()
    x = torch.from_numpy(gold["enc_x"])
    z = enc(x.to(DEV))
    assert torch.equal(z, ref(x.to(DEV)))
    z64 = C.encoder_forward(sd, chp, x, torch.float64)
    e32 = float((C.encoder_forward(sd, chp, x, torch.float32).double() - z64).abs().max())
    bound = max(1e-4 * float(z64.abs().max()), 4 * e32)
    err, err_g = float((z.cpu().double() - z64).abs().max()), float((z.cpu().double() - torch.from_numpy(gold["enc_z"]).double()).abs().max())
    print(f"Encoder: err vs fp64 {err:.3e}, vs golden {err_g:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert err <= bound and err_g <= bound + e32


def test_state_dict_round_trip_and_refusals():
    hp = D.small_decoder_hp()
    sd = D.synth_decoder_state_dict(hp, 3)
    dec = make_decoder(hp, sd)
    back = dec.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k].cpu(), sd[k]) for k in sd)
    x = C.synth_latent(1, hp["input_channel"], 7, 4)
    y = dec(x.to(DEV))
    folded = D.fold_state_dict(sd)
    dec2 = make_decoder(hp, folded)
    assert set(dec2.state_dict()) == set(folded)
    y64, e32, bound = decoder_reference("rt", hp, sd, x)
    assert float((dec2(x.to(DEV)).cpu().double() - y64).abs().max()) <= bound and float((y.cpu().double() - y64).abs().max()) <= bound
    with pytest.raises(RuntimeError):
        dec(x)                                                       # a host tensor: no CPU fallback
    with pytest.raises(ValueError):
        dec(torch.zeros(1, hp["input_channel"] + 32, 7, device=DEV))
    with pytest.raises(ValueError):
        dec.model[1](torch.zeros(1, 8, 7, device=DEV))
