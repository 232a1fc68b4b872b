"""The Amphion acoustic codec on the MI355X (csrc/fvq.hip, csrc/codec_unit_f16x3.hip, csrc/codec.hip and the drop-in modules) against the fp64
restatement of tests/codec_ref.py and the golden outputs of the real reference classes.

Quantizer (exact fp32, integers): the margin rule of codec_ref.margin_rule.  tau = 8 x the largest |dist32 - dist64| of the fp32 CPU restatement
on the same inputs (computed and printed, not a constant); a (level, frame) is decided when the fp64 margin at every level up to it exceeds tau;
codes must be IDENTICAL on decided pairs, nothing is compared elsewhere; undecided frames <= 2 % is asserted on the fp64 reference alone, first.
quantized_out / vq2emb bound on fully decided frames: 4 x the fp32 CPU restatement's own error against fp64, floor 1e-6 * max|z| (printed).

Fused unit (f16x3) bound, derived as tests/test_gpu_diffwave.py derives the DiffWave layer's: a split-f16 product term is exact to 2^-22 of
|w||v| and the fp32 accumulation adds a few 2^-24 of the partial sums: a GEMM output is off by 2e-6 * sum|w||v| + 3e-7 * |sum| plus sum|w| times
its operand's error.  snake(v) = v + sin^2(a v) / (a + 1e-9): the library's sin^2 is within 3.3e-7 of the exact one of its fp32 argument
(csrc/act1d_math.h), the argument a v carries one rounding (1.2e-7 |a v|, |d sin^2| <= 1), the fma one more: d_snake(v) = (3.3e-7 + 1.2e-7 |a v|) /
a + 2.4e-7 |snake(v)|; an input error e passes with |1 + sin(2 a v)| <= 2.  The epilogue adds the residual and stores: 1.2e-7 (|x| + |r|) + 1.2e-7 |y|.
The strided conv op has the first two steps only.  The fused f16x3 launch is NOT bit-identical to the four-call sequence in f16x3 (one GEMM with
K = 7 C sums in a different order than the conv kernel's chunk-by-chunk walk); under AMP_PRECISION=f32 the handle IS the four-call sequence
(amp_codec_unit_forward runs it), which the f32 test pins bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import codec_ref as C  # noqa: E402
import vocos_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden")
QP = "quantizers."


def make_rvq(hp, sd):
    from amphion_amd.models.codec.amphion_codec.quantize import ResidualVQ

    m = ResidualVQ(input_dim=hp["D"], num_quantizers=hp["N"], codebook_size=hp["K"], codebook_dim=hp["d"], quantizer_type="fvq",
                   use_l2_normlize=hp["l2"])
    m.load_state_dict(sd)
    return m.to(DEV).eval()


_REF = {}


def reference(tag, hp, sd, z, n=None):
    """the margin rule's CPU references, computed once per case and shared"""
    key = (tag, tuple(z.shape), n)
    if key not in _REF:
        _REF[key] = C.margin_rule(sd, hp, z, n)
    return _REF[key]


def check_encode(tag, hp, sd, z, n=None):
    r64, r32, tau, decided = reference(tag, hp, sd, z, n)
    frames_ok = decided[-1]                                  # decided at every level
    undecided = 1.0 - float(frames_ok.double().mean())
    print(f"{tag} z{tuple(z.shape)}: tau {tau:.3e}, smallest fp64 margin {float(r64['margin'].min()):.3e}, undecided frames {undecided:.4f}")
    assert undecided <= 0.02, "the fp64 reference itself leaves too many frames undecided for this seed"
    m = make_rvq(hp, sd)
    zq, codes, _, _, allq = m(z.to(DEV), n_quantizers=n)
    codes, zq = codes.cpu(), zq.cpu().double()
    assert codes.dtype == torch.int64 and codes.shape == r64["codes"].shape
    assert bool((codes == r64["codes"])[decided].all())
    mask = frames_ok[:, None, :].expand_as(zq)
    e32 = float((r32["zq"].double() - r64["zq"])[mask].abs().max()) if bool(mask.any()) else 0.0
    bound = max(4 * e32, 1e-6 * float(z.abs().max()))
    err = float((zq - r64["zq"])[mask].abs().max()) if bool(mask.any()) else 0.0
    print(f"    quantized_out: err {err:.3e}, fp32 restatement {e32:.3e}, bound {bound:.3e}")
    assert err <= bound
    # all_quantized sums to quantized_out in level order
    acc = torch.zeros_like(allq[0])
    for q in allq:
        acc = acc + q
    assert torch.equal(acc.cpu().double(), zq)
    return m, codes, zq, bound, r64, frames_ok


@pytest.fixture(scope="module")
def small_fvq():
    hp = C.small_fvq_hp()
    return hp, C.synth_fvq_state_dict(hp, 11)


@pytest.mark.parametrize("T", [1, 63, 65, 200])
def test_fvq_encode_small(small_fvq, T):
    hp, sd = small_fvq
    check_encode("small", hp, sd, C.synth_latent(2, hp["D"], T, 100 + T))


def test_fvq_encode_recipe():
    hp = C.recipe_fvq_hp()
    sd = C.synth_fvq_state_dict(hp, 0)
    check_encode("recipe", hp, sd, C.synth_latent(2, hp["D"], 150, 0))


def test_fvq_ties_resolve_to_lowest_index(small_fvq):
    hp, sd = small_fvq
    sd = dict(sd)
    K = hp["K"]
    for i in range(hp["N"]):
        cb = sd[f"{QP}{i}.codebook.weight"].clone()
        cb[K // 2:] = cb[: K // 2]                       # every row twice: distances tie exactly
        sd[f"{QP}{i}.codebook.weight"] = cb
    z = C.synth_latent(2, hp["D"], 65, 7)
    m = make_rvq(hp, sd)
    _, codes, _, _, _ = m(z.to(DEV))
    assert int(codes.max()) < K // 2 and int(codes.min()) >= 0
    # the same codes as the un-duplicated codebook gives (the CPU GEMM of the restatement does not return bit-equal distances for equal rows,
    # so it cannot referee the tie itself)
    _, half, _, _, _ = make_rvq(dict(hp, K=K // 2), {k: (v[: K // 2] if k.endswith("codebook.weight") else v) for k, v in sd.items()})(z.to(DEV))
    assert torch.equal(codes, half)


def test_fvq_fewer_quantizers(small_fvq):
    hp, sd = small_fvq
    _, codes, _, _, _, _ = check_encode("small", hp, sd, C.synth_latent(2, hp["D"], 65, 165), n=2)
    assert codes.shape[0] == 2


def test_fvq_identity_projections():
    hp = dict(D=8, d=8, K=64, N=3, l2=True)
    sd = C.synth_fvq_state_dict(hp, 21)
    assert not any("project" in k for k in sd)
    check_encode("identity", hp, sd, C.synth_latent(2, 8, 65, 22))


def test_fvq_without_l2_normalize():
    hp = dict(C.small_fvq_hp(), l2=False)
    sd = C.synth_fvq_state_dict(hp, 31)
    # raw Euclidean distances: in_project has unit gain, so z_e and the N(0, 1) codebook rows share their scale
    check_encode("no_l2", hp, sd, C.synth_latent(2, hp["D"], 65, 32))


def test_vq2emb(small_fvq):
    from amphion_amd._lib import AMP_ERR_INVALID, AmpError

    hp, sd = small_fvq
    z = C.synth_latent(2, hp["D"], 200, 300)
    m, codes, zq, bound, r64, _ = check_encode("small", hp, sd, z)
    emb = m.vq2emb(codes.to(DEV)).cpu().double()
    err_enc = float((emb - zq).abs().max())
    ref = C.vq2emb(sd, hp, codes, torch.float64)
    e32 = float((C.vq2emb(sd, hp, codes, torch.float32).double() - ref).abs().max())
    b2 = max(4 * e32, 1e-6 * float(z.abs().max()))
    err = float((emb - ref).abs().max())
    print(f"vq2emb: vs encode's quantized_out {err_enc:.3e} (bound {bound:.3e}); vs fp64 {err:.3e} (fp32 restatement {e32:.3e}, bound {b2:.3e})")
    assert err_enc <= bound and err <= b2
    part = m.vq2emb(codes.to(DEV), n_quantizers=2).cpu().double()
    assert float((part - C.vq2emb(sd, hp, codes, torch.float64, n=2)).abs().max()) <= b2
    for bad in (hp["K"], -1, 2 ** 40):
        c = codes.clone()
        c[1, 1, 17] = bad
        with pytest.raises(AmpError) as e:
            m.vq2emb(c.to(DEV))
        assert e.value.status == AMP_ERR_INVALID
    again = m.vq2emb(codes.to(DEV)).cpu().double()       # the flag was cleared and nothing faulted
    assert torch.equal(again, emb)


# ---- fused residual unit -------------------------------------------------------------------------------------------------------------
def unit_state_dict(Cn, seed):
    shapes = {}
    shapes["0.alpha"] = (1, Cn, 1)
    C._wn(shapes, "1.", Cn, Cn, 7)
    shapes["2.alpha"] = (1, Cn, 1)
    C._wn(shapes, "3.", Cn, Cn, 1)
    return C._synth(shapes, seed)


d_snake, unit_bound = C.d_snake, C.unit_bound          # the derived bounds live next to the fp64 restatement (tests/codec_ref.py)


def make_unit(Cn, dil, sd):
    from amphion_amd.models.codec.amphion_codec.codec import ResidualUnit

    u = ResidualUnit(Cn, dilation=dil)
    u.block.load_state_dict(sd)
    return u.to(DEV).eval()


@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("Cn", [32, 96, 192])
def test_fused_unit_vs_fp64(Cn, dil):
    from amphion_amd import _lib

    sd = unit_state_dict(Cn, 40 + Cn + dil)
    sd64 = {k: v.double() for k, v in sd.items()}
    _lib.check(_lib.lib().amp_set_codec_unit_fusion(1))        # wherever the kernel is built: the default policy stops at C = 96
    try:
        u = make_unit(Cn, dil, sd)
        assert u.fused(torch.device(DEV))
    finally:
        _lib.check(_lib.lib().amp_set_codec_unit_fusion(-1))
    worst = 0.0
    for T in (1, 26, 64, 65, 200):
        x = C.synth_latent(2, Cn, T, Cn + dil + T)
        y = u(x.to(DEV)).cpu().double()
        ref, tol = unit_bound(sd64, x.double(), dil)
        frac = float(((y - ref).abs() / tol).max())
        worst = max(worst, frac)
        assert torch.isfinite(y).all() and frac <= 1.0, (Cn, dil, T, frac)
    _lib.range_check(DEV)
    print(f"fused unit C={Cn} d={dil}: worst error / bound = {worst:.3f}")


def test_wide_unit_runs_unfused_vs_fp64():
    sd = unit_state_dict(384, 77)
    sd64 = {k: v.double() for k, v in sd.items()}
    u = make_unit(384, 3, sd)
    assert not u.fused(torch.device(DEV))
    x = C.synth_latent(2, 384, 65, 78)
    ref, tol = unit_bound(sd64, x.double(), 3)
    frac = float(((u(x.to(DEV)).cpu().double() - ref).abs() / tol).max())
    print(f"unfused unit C=384: error / bound = {frac:.3f}")
    assert frac <= 1.0


@pytest.mark.parametrize("Cn,dil", [(32, 1), (96, 9), (192, 3)])
def test_unit_f32_is_the_four_call_sequence(Cn, dil):
    """AMP_PRECISION=f32: the handle and snake -> conv -> snake -> conv (+ residual) through the op-level modules agree bit for bit, and both
    meet the f16x3 bound against fp64 (the exact-fp32 arithmetic is well inside it)"""
    from amphion_amd import _lib
    from amphion_amd.models.codec.amphion_codec.codec import snake

    sd = unit_state_dict(Cn, 50 + Cn)
    _lib.set_precision("f32")
    try:
        u = make_unit(Cn, dil, sd)
        assert not u.fused(torch.device(DEV))
        for T in (26, 65, 200):
            x = C.synth_latent(2, Cn, T, T).to(DEV)
            y = u(x)
            a1, c1, a2, c2 = u.block
            seq = c2(snake(c1(snake(x, a1.alpha)), a2.alpha), res=x)
            assert torch.equal(y, seq), (Cn, dil, T)
            ref, tol = unit_bound({k: v.double() for k, v in sd.items()}, x.cpu().double(), dil)
            assert bool(((y.cpu().double() - ref).abs() <= tol).all())
    finally:
        _lib.set_precision("f16x3")


# ---- strided conv op -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 5, 8])
def test_strided_conv_vs_fp64(conv_precision, s):
    from amphion_amd.models.codec.amphion_codec.codec import _StridedConv

    shapes = {"a.alpha": (1, 32, 1)}
    C._wn(shapes, "c.", 64, 32, 2 * s)
    sd = C._synth(shapes, 60 + s)
    conv = _StridedConv(32, 64, s, (s + 1) // 2)
    conv.load_state_dict({k[2:]: v for k, v in sd.items() if k.startswith("c.")})
    conv = conv.to(DEV)
    sd64 = {k: v.double() for k, v in sd.items()}
    alpha = sd["a.alpha"].to(DEV)
    w = C.folded(sd64, "c.")
    worst = 0.0
    for T in (s, 2 * s + 1, 97, 240):
        x = C.synth_latent(2, 32, T, s + T)
        y = conv(x.to(DEV), alpha).cpu().double()
        x64 = x.double()
        ref = C.strided_conv(sd64, "a.alpha", "c.", x64, s)
        assert y.shape == ref.shape and ref.shape[2] == (T + 2 * ((s + 1) // 2) - 2 * s) // s + 1
        p = (s + 1) // 2
        ref_b, tol = C.sconv_bound(w, sd64["c.bias"], sd64["a.alpha"], x64, s, p)
        assert torch.equal(ref_b, ref)
        frac = float(((y - ref).abs() / tol).max())
        worst = max(worst, frac)
        assert frac <= 1.0, (s, T, frac)
        plain = conv(x.to(DEV)).cpu().double()                 # without the activation
        ref0 = C.strided_conv(sd64, None, "c.", x64, s)
        ref0_b, tol0 = C.sconv_bound(w, sd64["c.bias"], None, x64, s, p)
        assert torch.equal(ref0_b, ref0)
        assert bool(((plain - ref0).abs() <= tol0).all()), (s, T)
    print(f"strided conv s={s} [{conv_precision}]: worst error / bound = {worst:.3f}")


# ---- modules -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_codec.npz"))


def make_encoder(hp, sd):
    from amphion_amd.models.codec.amphion_codec.codec import CodecEncoder

    m = CodecEncoder(**hp)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def make_decoder(fhp, sd):
    from amphion_amd.models.codec.amphion_codec.codec import CodecDecoder

    m = CodecDecoder(**C.decoder_kwargs(fhp))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.mark.parametrize("T", [230, 240])
def test_codec_encoder_small(conv_precision, gold, T):
    hp = C.small_encoder_hp()
    sd = C.synth_encoder_state_dict(hp, int(gold["enc_seed"]))
    x = torch.from_numpy(gold[f"x_{T}"])
    z64 = C.encoder_forward(sd, hp, x, torch.float64)
    e32 = float((C.encoder_forward(sd, hp, x, torch.float32).double() - z64).abs().max())
    bound = max(1e-4 * float(z64.abs().max()), 4 * e32)
    z = make_encoder(hp, sd)(x.to(DEV)).cpu().double()
    err, err_g = float((z - z64).abs().max()), float((z - torch.from_numpy(gold[f"z_{T}"]).double()).abs().max())
    print(f"encoder T={T} [{conv_precision}]: err vs fp64 {err:.3e}, vs golden {err_g:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert z.shape == z64.shape and err <= bound and err_g <= bound + e32


def test_codec_encoder_use_tanh(conv_precision):
    """use_tanh=True: the tanh is the last conv's store; |d tanh| <= 1, so the plain encoder's bound holds"""
    hp = dict(C.small_encoder_hp(), use_tanh=True)
    sd = C.synth_encoder_state_dict(hp, 81)
    x = C.synth_wave(2, 230, 82)
    z64 = C.encoder_forward(sd, hp, x, torch.float64)
    pre = C.encoder_forward(sd, C.small_encoder_hp(), x, torch.float64)
    e32 = float((C.encoder_forward(sd, hp, x, torch.float32).double() - z64).abs().max())
    bound = max(1e-4 * float(pre.abs().max()), 4 * e32)
    z = make_encoder(hp, sd)(x.to(DEV)).cpu().double()
    err = float((z - z64).abs().max())
    print(f"encoder use_tanh [{conv_precision}]: err vs fp64 {err:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}; max |z| {float(z.abs().max()):.3f}")
    assert float(z.abs().max()) <= 1.0 and float((z - pre).abs().max()) > 0.1 and err <= bound


def test_unit_fusion_switch():
    """amp_set_codec_unit_fusion picks the route of handles created afterwards; both routes meet the unit's bound"""
    from amphion_amd import _lib

    sd = unit_state_dict(96, 91)
    x = C.synth_latent(2, 96, 130, 92)
    ref, tol = unit_bound({k: v.double() for k, v in sd.items()}, x.double(), 3)
    try:
        for mode, fused in ((0, False), (1, True), (-1, True)):
            _lib.check(_lib.lib().amp_set_codec_unit_fusion(mode))
            u = make_unit(96, 3, sd)
            assert u.fused(torch.device(DEV)) == fused
            assert bool(((u(x.to(DEV)).cpu().double() - ref).abs() <= tol).all())
        _lib.check(_lib.lib().amp_set_codec_unit_fusion(-1))
        assert not make_unit(192, 3, unit_state_dict(192, 93)).fused(torch.device(DEV))     # the policy: the four launches are faster there
    finally:
        _lib.check(_lib.lib().amp_set_codec_unit_fusion(-1))


def test_strided_conv_many_rows():
    """B * cin beyond 65 535 rows (the y extent of a grid): the rows ride in grid.x"""
    from amphion_amd.models.codec.amphion_codec.codec import _StridedConv

    shapes = {}
    C._wn(shapes, "", 32, 32, 4)
    sd = C._synth(shapes, 95)
    conv = _StridedConv(32, 32, 2, 1)
    conv.load_state_dict(sd)
    conv = conv.to(DEV)
    x = C.synth_latent(2050, 32, 9, 96)                   # 65 600 rows
    y = conv(x.to(DEV)).cpu().double()
    sd64 = {k: v.double() for k, v in sd.items()}
    ref = F.conv1d(x.double(), C.folded(sd64, ""), sd64["bias"], stride=2, padding=1)
    tol = 2e-6 * (F.conv1d(x.double().abs(), C.folded(sd64, "").abs(), stride=2, padding=1) + sd64["bias"].abs()[None, :, None]) + 3e-7 * ref.abs()
    assert y.shape == ref.shape and bool(((y - ref).abs() <= tol).all())


def test_end_to_end(gold):
    ehp, fhp = C.small_encoder_hp(), C.small_fvq_hp()
    esd = C.synth_encoder_state_dict(ehp, int(gold["enc_seed"]))
    dsd = C.decoder_state_dict(fhp, int(gold["dec_seed"]))
    enc, dec = make_encoder(ehp, esd), make_decoder(fhp, dsd)
    x = torch.from_numpy(gold["x_240"]).to(DEV)
    z = enc(x)
    zq, codes = dec.quantize(z)
    emb = dec.vq2emb(codes)
    wav = dec(emb)
    qsd = {k[len("quantizer."):]: v for k, v in dsd.items() if k.startswith("quantizer.")}
    r64, _, tau, decided = C.margin_rule(qsd, fhp, z.cpu())                    # the fp64 quantizer applied to the HIP latent
    print(f"end to end: tau {tau:.3e}, undecided frames {1 - float(decided[-1].double().mean()):.4f}")
    assert 1 - float(decided[-1].double().mean()) <= 0.02
    assert bool((codes.cpu() == r64["codes"])[decided].all())
    vsd = {k[len("model."):]: v for k, v in dsd.items() if k.startswith("model.")}
    ref = V.vocos_forward(vsd, C.SMALL_VOCOS_HP, C.vq2emb(qsd, fhp, codes.cpu(), torch.float64), torch.float64)
    err = float((wav.cpu().double() - ref).abs().max())
    print(f"    wave {tuple(wav.shape)}: err vs fp64 from the HIP codes {err:.3e}")
    assert wav.shape == ref.shape and err <= 1e-4
    # forward(vq=True) returns the reference's 5-tuple
    out = dec(z, vq=True, eval_vq=True, n_quantizers=2)
    assert len(out) == 5 and out[1].shape == (2,) + tuple(codes.shape[1:]) and out[4].shape == (2,) + tuple(z.shape)
    assert float(out[2].abs().sum()) == 0.0 and float(out[3].abs().sum()) == 0.0 and torch.equal(out[1], codes[:2])


def test_state_dict_round_trip_and_refusals():
    ehp, fhp = C.small_encoder_hp(), C.small_fvq_hp()
    esd, dsd = C.synth_encoder_state_dict(ehp, 3), C.decoder_state_dict(fhp, 4)
    enc, dec = make_encoder(ehp, esd), make_decoder(fhp, dsd)
    for m, sd in ((enc, esd), (dec, dsd)):
        back = m.state_dict()
        assert list(back) == list(sd) and all(torch.equal(back[k].cpu(), sd[k]) for k in sd)
    dec.quantizer.train()
    with pytest.raises(NotImplementedError):
        dec.quantizer(torch.zeros(1, fhp["D"], 4, device=DEV))
    dec.quantize(torch.zeros(1, fhp["D"], 4, device=DEV))          # quantize() puts the quantizer in eval mode, like the reference
    with pytest.raises(RuntimeError):
        enc(torch.zeros(1, 1, 64))                                  # a host tensor: no CPU fallback
