"""FACodec on the MI355X (csrc/aa_unit_f16x3.hip, csrc/codec.hip: amp_aa_unit_*, and the drop-in modules of amphion_amd/models/codec/ns3_codec)
against the fp64 restatement of tests/facodec_ref.py and the golden outputs of the real reference classes.

Fused unit (f16x3): the bound is facodec_ref.unit_bound -- tests/test_gpu_codec.py's derivation with Activation1d's two FIR gains and Snake's
Lipschitz factor in place of the element-wise Snake, per element, from operand magnitudes.  The handle's four-launch f16x3 route (existing
kernels) must meet the same bound, which calibrates it, and the two routes may differ by at most the sum of their bounds.  Under
AMP_PRECISION=f32 the handle IS the four-call sequence, bit for bit.

Quantizer (exact fp32, integers): facodec_ref.margin_rule -- codes identical to fp64 on decided (level, frame) pairs, nothing compared elsewhere;
a frame counts for the residual group only when every prosody and content level decided it.  Values: max(4 x the fp32 CPU restatement's own
error, 1e-6 max|x|)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import codec_ref as C  # noqa: E402
import facodec_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden")
TN = 54          # output columns per workgroup of the fused unit (csrc/amp_internal.h: AA_TN)
UNIT_T = (1, 5, 6, 11, TN - 1, TN, TN + 1, 2 * TN + 5)


# ---- the unit ------------------------------------------------------------------------------------------------------------------------
def make_unit(Cn, dil, sd, mode):
    """a ResidualUnit whose handle was created under amp_set_aa_unit_fusion(mode)"""
    from amphion_amd import _lib
    from amphion_amd.models.codec.ns3_codec.facodec import ResidualUnit

    u = ResidualUnit(Cn, dilation=dil)
    u.load_state_dict(sd)
    u = u.to(DEV).eval()
    _lib.check(_lib.lib().amp_set_aa_unit_fusion(mode))
    try:
        u.fused(torch.device(DEV))
    finally:
        _lib.check(_lib.lib().amp_set_aa_unit_fusion(-1))
    return u


def unit_input(Cn, T, seed):
    """B = 2; item 1 is another draw, twice as large"""
    x = C.synth_latent(2, Cn, T, seed)
    x[1] *= 2.0
    return x


def check_unit_routes(Cn, dil, sd, Ts, want_fused=True):
    from amphion_amd import _lib

    sd64 = {k: v.double() for k, v in sd.items()}
    fused, plain = make_unit(Cn, dil, sd, 1), make_unit(Cn, dil, sd, 0)
    assert fused.fused(torch.device(DEV)) == want_fused and not plain.fused(torch.device(DEV))
    worst = [0.0, 0.0, 0.0]
    for T in Ts:
        x = unit_input(Cn, T, 1000 * Cn + 10 * dil + T)
        ref, tol = R.unit_bound(sd64, x.double(), dil)
        yf, yp = fused(x.to(DEV)), plain(x.to(DEV))
        for b in range(2):                                    # an item never depends on its batch
            assert torch.equal(fused(x[b:b + 1].to(DEV))[0], yf[b]), (Cn, dil, T, b)
        yf, yp = yf.cpu().double(), yp.cpu().double()
        assert torch.isfinite(yf).all() and torch.isfinite(yp).all()
        fr = [float(((yf - ref).abs() / tol).max()), float(((yp - ref).abs() / tol).max()), float(((yf - yp).abs() / (2 * tol)).max())]
        print(f"    C={Cn} d={dil} T={T}: fused err / bound {fr[0]:.3f}, four launches {fr[1]:.3f}, fused vs four launches / (2 x bound) {fr[2]:.3f}")
        worst = [max(a, b) for a, b in zip(worst, fr)]
        assert fr[1] <= 1.0, ("the four-launch route misses the bound: the derivation is wrong", Cn, dil, T, fr[1])
        assert fr[0] <= 1.0 and fr[2] <= 1.0, (Cn, dil, T, fr)
    _lib.range_check(DEV)
    print(f"aa unit C={Cn} d={dil}: worst error / bound: fused {worst[0]:.3f}, four launches {worst[1]:.3f}")


@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("Cn", [32, 64, 128])
def test_fused_unit_vs_fp64(Cn, dil):
    check_unit_routes(Cn, dil, R.synth_unit_state_dict(Cn, 40 + Cn + dil), UNIT_T)


def test_fused_unit_plain_snake(monkeypatch):
    """Activation1d(Snake): beta = NULL, 1 / (alpha + 1e-9) scales the periodic term"""
    import amphion_amd.models.codec.ns3_codec.facodec as Fm
    from amphion_amd.modules.activation_functions.snake import Snake
    from amphion_amd.modules.anti_aliasing.act import Activation1d

    sd = {k: v for k, v in R.synth_unit_state_dict(64, 7).items() if not k.endswith("act.beta")}
    monkeypatch.setattr(Fm, "_aa", lambda c: Activation1d(activation=Snake(c, alpha_logscale=True)))
    check_unit_routes(64, 3, sd, (11, TN + 1))


@pytest.mark.parametrize("Cn", [48, 256])
def test_unbuilt_widths_run_the_four_launches(Cn):
    sd = R.synth_unit_state_dict(Cn, 60 + Cn)
    sd64 = {k: v.double() for k, v in sd.items()}
    u = make_unit(Cn, 3, sd, 1)
    assert not u.fused(torch.device(DEV))
    x = unit_input(Cn, 65, Cn)
    ref, tol = R.unit_bound(sd64, x.double(), 3)
    frac = float(((u(x.to(DEV)).cpu().double() - ref).abs() / tol).max())
    print(f"unfused aa unit C={Cn}: error / bound = {frac:.3f}")
    assert frac <= 1.0


def test_fusion_switch_affects_later_handles_only():
    from amphion_amd import _lib

    sd = R.synth_unit_state_dict(32, 5)
    dev = torch.device(DEV)
    on, off = make_unit(32, 1, sd, 1), make_unit(32, 1, sd, 0)
    assert on.fused(dev) and not off.fused(dev)
    L = _lib.lib()
    try:
        _lib.check(L.amp_set_aa_unit_fusion(0))
        assert on.fused(dev)                                   # an existing handle keeps its route
        _lib.check(L.amp_set_aa_unit_fusion(1))
        assert not off.fused(dev)
        assert L.amp_set_aa_unit_fusion(2) < 0 and L.amp_set_aa_unit_fusion(-2) < 0
    finally:
        _lib.check(L.amp_set_aa_unit_fusion(-1))


@pytest.mark.parametrize("Cn,dil", [(32, 1), (64, 9), (128, 3)])
def test_unit_f32_is_the_four_call_sequence(Cn, dil):
    from amphion_amd import _lib

    sd = R.synth_unit_state_dict(Cn, 50 + Cn)
    _lib.set_precision("f32")
    try:
        u = make_unit(Cn, dil, sd, 1)
        assert not u.fused(torch.device(DEV))
        for T in (5, 26, 65, 113):
            x = unit_input(Cn, T, T).to(DEV)
            y = u(x)
            a1, c1, a2, c2 = u.block
            seq = c2(a2(c1(a1(x))), res=x)
            assert torch.equal(y, seq), (Cn, dil, T)
            ref, tol = R.unit_bound({k: v.double() for k, v in sd.items()}, x.cpu().double(), dil)
            assert bool(((y.cpu().double() - ref).abs() <= tol).all())
    finally:
        _lib.set_precision("f16x3")


# ---- modules -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_facodec.npz"))


def make_encoder(hp, sd):
    from amphion_amd.models.codec.ns3_codec import FACodecEncoder

    m = FACodecEncoder(**hp)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def make_decoder(hp, sd):
    from amphion_amd.models.codec.ns3_codec import FACodecDecoder

    m = FACodecDecoder(**hp)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


_DEC = {}


def small_decoder(gold):
    """(hp, state_dict, module) of the small decoder, built once"""
    if "d" not in _DEC:
        hp = R.small_decoder_hp()
        sd = R.synth_decoder_state_dict(hp, int(gold["dec_seed"]))
        _DEC["d"] = (hp, sd, make_decoder(hp, sd))
    return _DEC["d"]


# ---- quantizer -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 63, 65])
def test_quantize(gold, T):
    from amphion_amd._lib import AMP_ERR_INVALID, AmpError

    hp, sd, dec = small_decoder(gold)
    x = C.synth_latent(2, hp["vq_dim"], T, R.QUANT_SEEDS[T])
    r64, r32, tau, decided = R.margin_rule(sd, hp, x)
    undecided = 1.0 - float(decided.all(0).double().mean())
    print(f"quantize T={T}: tau {tau:.3e}, undecided frames {undecided:.4f}")
    assert undecided <= 0.02, "the fp64 reference itself leaves too many frames undecided for this seed"
    outs, qs, commit, buf = dec.quantize(x.to(DEV))
    assert qs.dtype == torch.int64 and qs.shape == r64["qs"].shape and float(commit.abs().sum()) == 0.0 and len(buf) == 3
    assert bool((qs.cpu() == r64["qs"])[decided].all())
    ok = decided.all(0)
    mask = ok[:, None, :].expand_as(outs)
    floor = 1e-6 * float(x.abs().max())
    for name, got, a64, a32 in [("outs", outs, r64["outs"], r32["outs"])] + [(f"quantized_buf[{i}]", buf[i], r64["quantized_buf"][i],
                                                                             r32["quantized_buf"][i]) for i in range(3)]:
        e32 = float((a32.double() - a64)[mask].abs().max())
        err = float((got.cpu().double() - a64)[mask].abs().max())
        print(f"    {name}: err {err:.3e}, fp32 restatement {e32:.3e}, bound {max(4 * e32, floor):.3e}")
        assert err <= max(4 * e32, floor), name
    # vq2emb from the HIP codes: against encode's own sum, and against fp64 from the same codes
    emb = dec.vq2emb(qs).cpu().double()
    assert float((emb - outs.cpu().double()).abs().max()) <= max(4 * float((r32["outs"].double() - r64["outs"])[mask].abs().max()), floor)
    for use_res in (True, False):
        ref = R.vq2emb(sd, hp, qs.cpu(), torch.float64, use_res)
        e32 = float((R.vq2emb(sd, hp, qs.cpu(), torch.float32, use_res).double() - ref).abs().max())
        err = float((dec.vq2emb(qs, use_residual_code=use_res).cpu().double() - ref).abs().max())
        print(f"    vq2emb(use_residual_code={use_res}): err {err:.3e}, fp32 restatement {e32:.3e}")
        assert err <= max(4 * e32, floor)
    if T > 1:
        for level, bad in ((0, 2 ** hp["codebook_size_prosody"]), (2, -1), (4, 2 ** 40)):
            c = qs.clone()
            c[level, 1, T // 2] = bad
            with pytest.raises(AmpError) as e:
                dec.vq2emb(c)
            assert e.value.status == AMP_ERR_INVALID
        assert torch.equal(dec.vq2emb(qs).cpu().double(), emb)    # the flag was cleared and nothing faulted
        # n_quantizers caps every group: 1 + 1 + 1 levels
        outs1, qs1, _, buf1 = dec.quantize(x.to(DEV), n_quantizers=1)
        assert qs1.shape[0] == 3 and torch.equal(qs1[0], qs[0]) and torch.equal(qs1[1], qs[1]) and torch.equal(buf1[0], buf[0])


# ---- timbre path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 33])
def test_speaker_embedding(gold, T):
    """spk_embs within max(4 x the fp32 CPU restatement's own error, 1e-6 max|ref|) of fp64.  The one-frame case is the sharp one: nothing
    averages the per-frame error down, and it caught the conv kernels' residual argument (accumulating onto the residual stream) at 6.2e-6
    against a bound of 5.6e-6; with the residual added after the accumulation (amp_pw_forward) it is 1.8e-6."""
    hp, sd, dec = small_decoder(gold)
    x = C.synth_latent(2, 256, T, 500 + T)
    ref = R.speaker_embedding(sd, x, torch.float64)
    e32 = float((R.speaker_embedding(sd, x, torch.float32).double() - ref).abs().max())
    bound = max(4 * e32, 1e-6 * float(ref.abs().max()))
    spk = dec(x.to(DEV), vq=True)[4].cpu().double()
    err = float((spk - ref).abs().max())
    print(f"spk_embs T={T}: err {err:.3e}, fp32 restatement {e32:.3e}, bound {bound:.3e}")
    assert spk.shape == (2, 256) and err <= bound
    # the position table is indexed with the batch index: item 1's input placed at index 0 gives another embedding
    alone = dec(x[1:2].to(DEV), vq=True)[4].cpu().double()
    ref0 = R.speaker_embedding(sd, x[1:2], torch.float64)
    assert float((alone - ref0).abs().max()) <= bound
    assert float((alone[0] - spk[1]).abs().max()) > 100 * bound


# ---- encoder and decoder -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [230, 240])
def test_encoder_small(conv_precision, gold, T):
    hp = R.small_encoder_hp()
    sd = R.synth_encoder_state_dict(hp, int(gold["enc_seed"]))
    x = torch.from_numpy(gold[f"x_{T}"])
    z64 = R.encoder_forward(sd, hp, x, torch.float64)
    e32 = float((R.encoder_forward(sd, hp, x, torch.float32).double() - z64).abs().max())
    bound = max(1e-4 * float(z64.abs().max()), 4 * e32)
    z = make_encoder(hp, sd)(x.to(DEV)).cpu().double()
    err, err_g = float((z - z64).abs().max()), float((z - torch.from_numpy(gold[f"z_{T}"]).double()).abs().max())
    print(f"encoder T={T} [{conv_precision}]: err vs fp64 {err:.3e}, vs golden {err_g:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert z.shape == z64.shape and err <= bound and err_g <= bound + e32


@pytest.mark.parametrize("n", [1, 7, 33])
def test_decoder_inference_small(conv_precision, gold, n):
    hp, sd, _ = small_decoder(gold)
    dec = make_decoder(hp, sd)                     # handles of this precision
    x, spk = torch.from_numpy(gold[f"dec_x_{n}"]), torch.from_numpy(gold["dec_spk"])
    w64 = R.decoder_inference(sd, hp, x, spk, torch.float64)
    e32 = float((R.decoder_inference(sd, hp, x, spk, torch.float32).double() - w64).abs().max())
    bound = max(1e-4 * float(w64.abs().max()), 4 * e32)
    w = dec.inference(x.to(DEV), spk.to(DEV)).cpu().double()
    err, err_g = float((w - w64).abs().max()), float((w - torch.from_numpy(gold[f"dec_wav_{n}"]).double()).abs().max())
    print(f"decoder {n} frames [{conv_precision}]: err vs fp64 {err:.3e}, vs golden {err_g:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert w.shape == w64.shape == (2, 1, n * 6) and err <= bound and err_g <= bound + e32


def test_recipe_encoder_frame_counts():
    """the public rates (hop 200): 1599, 1600 and 1601 samples all give 8 frames; one of them against fp64"""
    hp = R.recipe_encoder_hp()
    sd = R.synth_encoder_state_dict(hp, 12)
    enc = make_encoder(hp, sd)
    for T in (1599, 1600, 1601):
        x = C.synth_wave(1, T, T)
        z = enc(x.to(DEV))
        assert tuple(z.shape) == (1, 256, 8)
    z64 = R.encoder_forward(sd, hp, x, torch.float64)
    e32 = float((R.encoder_forward(sd, hp, x, torch.float32).double() - z64).abs().max())
    bound = max(1e-4 * float(z64.abs().max()), 4 * e32)
    err = float((z.cpu().double() - z64).abs().max())
    print(f"recipe encoder T=1601: err vs fp64 {err:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_end_to_end(conv_precision, gold):
    """wave -> encoder -> forward(vq=True) -> inference, each stage against fp64 run from the HIP stage before it"""
    ehp = R.small_encoder_hp()
    esd = R.synth_encoder_state_dict(ehp, int(gold["enc_seed"]))
    hp, sd, _ = small_decoder(gold)
    enc, dec = make_encoder(ehp, esd), make_decoder(hp, sd)
    x = torch.from_numpy(gold["x_240"]).to(DEV)
    z = enc(x)
    outs, qs, commit, buf, spk = dec(z, vq=True, eval_vq=True)
    assert float(commit.abs().sum()) == 0.0 and commit.shape == (6,)
    r64, _, tau, decided = R.margin_rule(sd, hp, z.cpu())
    print(f"end to end [{conv_precision}]: tau {tau:.3e}, undecided frames {1 - float(decided.all(0).double().mean()):.4f}")
    assert bool((qs.cpu() == r64["qs"])[decided].all())
    emb64 = R.vq2emb(sd, hp, qs.cpu(), torch.float64)
    w64 = R.decoder_inference(sd, hp, emb64, spk.cpu(), torch.float64)
    e32 = float((R.decoder_inference(sd, hp, emb64, spk.cpu(), torch.float32).double() - w64).abs().max())
    bound = max(1e-4 * float(w64.abs().max()), 4 * e32)
    wav = dec.inference(outs, spk)
    err = float((wav.cpu().double() - w64).abs().max())
    print(f"    wave {tuple(wav.shape)}: err vs fp64 from the HIP codes {err:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert wav.shape == w64.shape and err <= bound


def test_state_dict_round_trip_and_refusals(gold):
    ehp, hp = R.small_encoder_hp(), R.small_decoder_hp()
    esd, dsd = R.synth_encoder_state_dict(ehp, 3), R.synth_decoder_state_dict(hp, 4)
    for make, h, sd in ((make_encoder, ehp, esd), (make_decoder, hp, dsd)):
        for form in (sd, R.fold(sd)):
            back = make(h, form).state_dict()
            assert list(back) == list(form) and all(torch.equal(back[k].cpu(), form[k]) for k in form)
    extra = dict(dsd)
    extra["f0_predictor.heads.0.weight"] = torch.zeros(1, 256)
    extra["x_timbre_predictor.1.heads.0.bias"] = torch.zeros(245200)
    dec = make_decoder(hp, extra)
    assert not any(k.startswith(R.PREDICTOR_PREFIXES) for k in dec.state_dict())
    with pytest.raises(RuntimeError):
        make_decoder(hp, dict(dsd, **{"unknown.weight": torch.zeros(1)}))
    x = torch.zeros(1, 256, 4, device=DEV)
    with pytest.raises(NotImplementedError):
        dec(x, vq=False, speaker_embedding=torch.zeros(1, 256, device=DEV), quantized=[x, x, x])
    dec.quantizer.train()
    with pytest.raises(NotImplementedError):
        dec.quantizer[0](x)
    dec(x, vq=True)                                             # eval_vq=True puts the quantizer in eval mode, like the reference
    with pytest.raises(RuntimeError):
        make_encoder(ehp, esd)(torch.zeros(1, 1, 64))           # a host tensor: no CPU fallback
