"""FACodec's voice-conversion classes on the MI355X (csrc/vits_text.hip: amp_layer_norm_c_style, amp_embed_sum_c; the drop-in modules
FACodecEncoderV2 / FACodecDecoderV2 / FACodecRedecoder / MelSpectrogram and the conditioned TransformerEncoder of
amphion_amd/models/codec/ns3_codec) against the fp64 restatement of tests/facodec_vc_ref.py and the golden outputs of the real reference classes.

Bounds, all taken from the tests these extend and none from what the kernels give:
  style LayerNorm op       2e-5 absolute against fp64, tests/test_gpu_vits_ops.py's plain layer-norm bound
  embedding sum op         torch.equal with the fp32 CPU sum in the same order
  transformer outputs      max(4 x the fp32 CPU restatement's own error, 1e-6 max|ref|), test_gpu_facodec.py::test_speaker_embedding's
  log-mel                  1e-4 absolute, the mel front end's documented bound (tests/test_gpu_mel.py)
  quantizer                codes equal wherever facodec_vc_ref.margin_rule3, run from the HIP prosody latent and x, decides; values
                           max(4 e32, 1e-6 max|x|) on decided frames
  waves                    max(1e-4 max|w64|, 4 e32) against fp64 and, with + e32, against the golden
The golden of FACodecRedecoder.forward is the real submodules composed as forward means them (tests/golden/make_golden_facodec_vc.py: the
reference's own forward normalises the wrong axis and raises unless T == 256)."""
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
from test_gpu_vits_ops import C_GRID, T_GRID  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden")
LN_C = sorted(set(C_GRID + [256, 264]))       # 256: the recipe's width, the last that stays in registers; 264: channels re-read past them


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_facodec_vc.npz"))


def g(gold, k):
    return torch.from_numpy(gold[k])


def load(cls, hp, sd):
    m = cls(**hp)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


_MODELS = {}


def small(gold, which):
    """(hp, state_dict, module) of a small model under the current conv precision, built once per precision"""
    from amphion_amd import _lib
    from amphion_amd.models.codec.ns3_codec import FACodecDecoderV2, FACodecRedecoder

    key = (which, _lib.get_precision())
    if key not in _MODELS:
        if which == "dec":
            hp = R.small_decoder_hp()
            sd = V.synth_decoder_v2_state_dict(hp, int(gold["dec_seed"]))
            _MODELS[key] = (hp, sd, load(FACodecDecoderV2, hp, sd))
        else:
            hp = V.small_redecoder_hp()
            sd = V.synth_redecoder_state_dict(hp, int(gold["red_seed"]))
            _MODELS[key] = (hp, sd, load(FACodecRedecoder, hp, sd))
    return _MODELS[key]


def stage_bound(ref64, ref32):
    """test_speaker_embedding's: max(4 x the fp32 restatement's own error, 1e-6 max|ref|) -> (bound, e32)"""
    e32 = float((ref32.double() - ref64).abs().max())
    return max(4 * e32, 1e-6 * float(ref64.abs().max())), e32


def wave_bound(w64, w32):
    e32 = float((w32.double() - w64).abs().max())
    return max(1e-4 * float(w64.abs().max()), 4 * e32), e32


# ---- the two ops ---------------------------------------------------------------------------------------------------------------------
def _ln_case(C_, T, seed):
    t = torch.Generator().manual_seed(seed)
    x = torch.randn(3, C_, T, generator=t) * 2.0 + 0.5
    res = torch.randn(3, C_, T, generator=t)
    style = torch.cat([1 + 0.2 * torch.randn(3, C_, generator=t), 0.1 * torch.randn(3, C_, generator=t)], dim=1)   # a row per item
    return x, res, style


def _ln_ref(x, res, style):
    C_ = x.shape[1]
    v = x.double() + (res.double() if res is not None else 0.0)
    n = torch.nn.functional.layer_norm(v.transpose(1, 2), (C_,), None, None, 1e-5).transpose(1, 2)
    return style.double()[:, :C_, None] * n + style.double()[:, C_:, None]


@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("C_", LN_C)
def test_style_layer_norm_op(C_, T):
    from amphion_amd.modules import hip_ops

    x, res, style = _ln_case(C_, T, 7000 + 13 * C_ + T)
    for r in (None, res):
        got = hip_ops.layer_norm_c_style(x.to(DEV), style.to(DEV), res=None if r is None else r.to(DEV)).cpu().double()
        err = float((got - _ln_ref(x, r, style)).abs().max())
        print(f"style LN C={C_} T={T} res={r is not None}: err {err:.3e}")
        assert got.shape == x.shape and torch.isfinite(got).all() and err <= 2e-5, (C_, T, r is not None, err)
    # the style rows really are per item: item 0's row on every item gives another result for items 1 and 2
    same = hip_ops.layer_norm_c_style(x.to(DEV), style[:1].expand(3, -1).contiguous().to(DEV)).cpu()
    first = hip_ops.layer_norm_c_style(x.to(DEV), style.to(DEV)).cpu()
    assert torch.equal(same[0], first[0]) and not torch.equal(same[1], first[1])


@pytest.mark.parametrize("C_,T", [(24, 257), (192, 33), (256, 500), (264, 65)])
def test_style_layer_norm_has_layer_norm_c_bits(C_, T):
    """one (gamma | beta) row for every item == amp_layer_norm_c with that gamma and beta, bit for bit: the same mean, variance and order;
    in place (y = x) as amp_layer_norm_c allows"""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    x, res, style = _ln_case(C_, T, 7100 + C_)
    row = style[1]
    xd, rd = x.to(DEV), res.to(DEV)
    for r in (None, rd):
        want = hip_ops.layer_norm_c(xd, row[:C_].contiguous().to(DEV), row[C_:].contiguous().to(DEV), res=r)
        got = hip_ops.layer_norm_c_style(xd, row[None].expand(3, -1).contiguous().to(DEV), res=r)
        assert torch.equal(got, want), (C_, T, r is not None)
    y = xd.clone()
    sd = style.to(DEV)
    _lib.check(_lib.lib().amp_layer_norm_c_style(_lib.ptr(y), None, _lib.ptr(sd), 3, C_, T, 1e-5, _lib.ptr(y), _lib.current_stream_ptr(y.device)))
    assert torch.equal(y, hip_ops.layer_norm_c_style(xd, sd))


def _tables(N, D, seed):
    t = torch.Generator().manual_seed(seed)
    return [torch.randn((32, 64)[n % 2], D, generator=t) for n in range(N)]


def _codes(tables, B, T, seed):
    t = torch.Generator().manual_seed(seed)
    c = torch.stack([torch.randint(0, w.shape[0], (B, T), generator=t) for w in tables])
    c[:, 0, 0] = 0
    c[:, -1, -1] = torch.tensor([w.shape[0] - 1 for w in tables])
    return c


def _embed_sum_cpu(codes, tables, init):
    """torch's fp32 sum in the kernel's documented order, transposed to [B, D, T]"""
    acc = None if init is None else init.transpose(1, 2)
    for n, w in enumerate(tables):
        e = torch.nn.functional.embedding(codes[n], w)
        acc = e if acc is None else acc + e
    return acc.transpose(1, 2).contiguous()


@pytest.mark.parametrize("D", [1, 8, 256, 257])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_embed_sum_op(N, D):
    from amphion_amd.modules import hip_ops

    tables = _tables(N, D, 8000 + 10 * N + D)
    td = [w.to(DEV) for w in tables]
    for T in (1, 63, 64, 65, 257):
        for B in (1, 3):
            codes = _codes(tables, B, T, 100 * T + B)
            init = torch.randn(B, D, T, generator=torch.Generator().manual_seed(T + B))
            for ini in (None, init):
                got = hip_ops.embed_sum_c(codes.to(DEV), td, None if ini is None else ini.to(DEV)).cpu()
                assert torch.equal(got, _embed_sum_cpu(codes, tables, ini)), (N, D, T, B, ini is not None)


def test_embed_sum_refuses_an_index_outside_its_table():
    from amphion_amd._lib import AMP_ERR_INVALID, AmpError
    from amphion_amd.modules import hip_ops

    tables = _tables(3, 256, 8100)
    td = [w.to(DEV) for w in tables]
    codes = _codes(tables, 3, 65, 8101)
    before = hip_ops.embed_sum_c(codes.to(DEV), td)
    for level, bad in ((0, 32), (1, 64), (1, -1), (2, 2 ** 40)):
        c = codes.clone()
        c[level, 1, 40] = bad
        with pytest.raises(AmpError) as e:
            hip_ops.embed_sum_c(c.to(DEV), td)
        assert e.value.status == AMP_ERR_INVALID
        assert torch.equal(hip_ops.embed_sum_c(codes.to(DEV), td), before)        # the flag was cleared, the next valid call is unharmed
    assert torch.equal(before.cpu(), _embed_sum_cpu(codes, tables, None))
    with pytest.raises(TypeError):
        hip_ops.embed_sum_c(codes.float().to(DEV), td)
    with pytest.raises(RuntimeError):
        hip_ops.embed_sum_c(codes, td)
    with pytest.raises(ValueError):
        hip_ops.embed_sum_c(codes[:2].to(DEV), td)
    with pytest.raises(ValueError):
        hip_ops.embed_sum_c(codes.to(DEV), td, torch.zeros(3, 255, 65, device=DEV))


# ---- the conditioned encoder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 33])
def test_conditioned_encoder(gold, T):
    hp, sd, red = small(gold, "red")
    enc = red.timbre_cond_prosody_enc
    x = C.synth_latent(2, 256, T, 600 + T).transpose(1, 2).contiguous()                    # [B, T, 256]
    spk = 0.5 * C.synth_latent(2, 256, 1, 650 + T)[:, :, 0]
    ref = V.cond_encoder(sd, x, spk, torch.float64)
    bound, e32 = stage_bound(ref, V.cond_encoder(sd, x, spk, torch.float32))
    cond = spk.unsqueeze(1).expand(-1, T, -1)
    y = enc(x.to(DEV), key_padding_mask=None, condition=cond.to(DEV))
    err = float((y.cpu().double() - ref).abs().max())
    print(f"conditioned encoder T={T}: err {err:.3e}, fp32 restatement {e32:.3e}, bound {bound:.3e}")
    assert tuple(y.shape) == (2, T, 256) and err <= bound
    assert torch.equal(enc(x.to(DEV), None, cond.to(DEV)), y)                               # a repeated call returns equal bits
    other = enc(x.to(DEV), None, (-cond).to(DEV)).cpu().double()
    assert float((other - y.cpu().double()).abs().max()) > 100 * bound
    ref_o = V.cond_encoder(sd, x, -spk, torch.float64)
    assert float((other - ref_o).abs().max()) <= stage_bound(ref_o, V.cond_encoder(sd, x, -spk, torch.float32))[0]
    with pytest.raises(ValueError):
        enc(x.to(DEV))
    with pytest.raises(NotImplementedError):
        enc(x.to(DEV), torch.ones(2, T, device=DEV), cond.to(DEV))


# ---- the prosody feature ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [600, 1000, 1601])
def test_get_prosody_feature(gold, L):
    from amphion_amd.models.codec.ns3_codec import FACodecEncoderV2

    hp = R.small_encoder_hp()
    enc = load(FACodecEncoderV2, hp, V.synth_encoder_v2_state_dict(hp, int(gold["enc_seed"])))
    w = g(gold, f"wave_{L}")
    pf = enc.get_prosody_feature(w.to(DEV))
    ref = V.prosody_feature(w, torch.float64)
    err, err_g = float((pf.cpu().double() - ref).abs().max()), float((pf.cpu().double() - g(gold, f"pf_{L}").double()).abs().max())
    print(f"prosody feature L={L}: err vs fp64 {err:.3e}, vs golden {err_g:.3e}")
    assert tuple(pf.shape) == (2, 20, 1 + (L - 200) // 200) and err <= 1e-4 and err_g <= 1e-4
    assert torch.equal(enc.get_prosody_feature(w.to(DEV)), pf)
    full = enc.mel_transform(w.squeeze(1).to(DEV))
    assert tuple(full.shape) == (2, 80, pf.shape[2]) and float((full.cpu().double() - V.mel_spectrogram(w.squeeze(1))).abs().max()) <= 1e-4
    if L == 600:
        with pytest.raises(ValueError):
            enc.get_prosody_feature(w[:, :, :412].to(DEV))                                  # L <= (n_fft - hop) / 2: torch's reflect pad refuses it too
        enc.get_prosody_feature(w[:, :, :413].to(DEV))
        z = enc(g(gold, "x_230").to(DEV)).cpu().double()                                    # the block is FACodecEncoder's
        block = {k: v.cpu() for k, v in enc.state_dict().items() if k.startswith("block.")}
        z64 = R.encoder_forward(block, hp, g(gold, "x_230"), torch.float64)
        bound, e32 = wave_bound(z64, R.encoder_forward(block, hp, g(gold, "x_230"), torch.float32))
        assert float((z - z64).abs().max()) <= bound and float((z - g(gold, "z_230").double()).abs().max()) <= bound + e32
        assert torch.equal(enc.inference(g(gold, "x_230").to(DEV)).cpu().double(), z)


# ---- FACodecDecoderV2.quantize -----------------------------------------------------------------------------------------------------------
def check_quantize(dec, hp, sd, x, pf, label):
    """dec.quantize(x, pf) on device tensors against fp64 run from the HIP prosody latent and x -> (outs, qs)"""
    xp = dec._prosody_latent(pf)
    ref_p = V.prosody_latent(sd, pf.cpu(), torch.float64)
    bound_p, e32_p = stage_bound(ref_p, V.prosody_latent(sd, pf.cpu(), torch.float32))
    err_p = float((xp.cpu().double() - ref_p).abs().max())
    print(f"{label}: prosody latent err {err_p:.3e}, fp32 restatement {e32_p:.3e}, bound {bound_p:.3e}")
    assert tuple(xp.shape) == (x.shape[0], 256, x.shape[2]) and err_p <= bound_p
    r64, r32, tau, decided = V.margin_rule3(sd, hp, xp.cpu(), x.cpu())
    print(f"{label}: tau {tau:.3e}, undecided frames {1 - float(decided.all(0).double().mean()):.4f}")
    outs, qs, commit, buf = dec.quantize(x, pf)
    assert qs.dtype == torch.int64 and qs.shape == r64["qs"].shape and float(commit.abs().sum()) == 0.0 and len(buf) == 3
    assert bool((qs.cpu() == r64["qs"])[decided].all())
    ok = decided.all(0)
    mask = ok[:, None, :].expand_as(outs)
    floor = 1e-6 * float(x.abs().max())
    for name, got, a64, a32 in [("outs", outs, r64["outs"], r32["outs"])] + [(f"quantized_buf[{i}]", buf[i], r64["quantized_buf"][i],
                                                                             r32["quantized_buf"][i]) for i in range(3)]:
        e32 = float((a32.double() - a64)[mask].abs().max()) if bool(ok.any()) else 0.0
        err = float((got.cpu().double() - a64)[mask].abs().max()) if bool(ok.any()) else 0.0
        print(f"    {name}: err {err:.3e}, fp32 restatement {e32:.3e}, bound {max(4 * e32, floor):.3e}")
        assert err <= max(4 * e32, floor), name
    for use_res in (True, False):
        ref = V.vq2emb_v2(sd, hp, qs.cpu(), torch.float64, use_res)
        e32 = float((V.vq2emb_v2(sd, hp, qs.cpu(), torch.float32, use_res).double() - ref).abs().max())
        err = float((dec.vq2emb(qs, use_residual=use_res).cpu().double() - ref).abs().max())
        print(f"    vq2emb(use_residual={use_res}): err {err:.3e}, fp32 restatement {e32:.3e}")
        assert err <= max(4 * e32, floor)
    return outs, qs, buf, decided


@pytest.mark.parametrize("T", [1, 63, 65])
def test_v2_quantize(gold, T):
    hp, sd, dec = small(gold, "dec")
    sx, sp = V.QUANT_SEEDS[T]
    x, pf = C.synth_latent(2, hp["vq_dim"], T, sx), V.synth_prosody_feature(2, T, sp)
    outs, qs, buf, decided = check_quantize(dec, hp, sd, x.to(DEV), pf.to(DEV), f"V2 quantize T={T}")
    # the seeds were chosen on the CPU (tests/test_oracle_facodec_vc.py); from the HIP prosody latent the rule must still decide nearly all
    assert 1.0 - float(decided.all(0).double().mean()) <= 0.02
    outs2, qs2, _, _ = dec.quantize(x.to(DEV), pf.to(DEV))
    assert torch.equal(qs2, qs) and torch.equal(outs2, outs)
    o1, q1, _, b1 = dec.quantize(x.to(DEV), pf.to(DEV), n_quantizers=1)                     # n_quantizers caps every group: 1 + 1 + 1 levels
    assert q1.shape[0] == 3 and torch.equal(q1[0], qs[0]) and torch.equal(q1[1], qs[1]) and torch.equal(b1[0], buf[0])
    fo, fq, fc, fb, spk = dec(x.to(DEV), pf.to(DEV), vq=True, eval_vq=False)
    assert torch.equal(fq, qs) and torch.equal(fo, outs) and fc.shape == (6,)
    bound, e32 = stage_bound(R.speaker_embedding(sd, x, torch.float64), R.speaker_embedding(sd, x, torch.float32))
    assert float((spk.cpu().double() - R.speaker_embedding(sd, x, torch.float64)).abs().max()) <= bound


def test_v2_forward_matches_the_golden(gold):
    hp, sd, dec = small(gold, "dec")
    x, pf = g(gold, "fwd_x"), g(gold, "fwd_pf")
    outs, qs, buf, decided = check_quantize(dec, hp, sd, x.to(DEV), pf.to(DEV), "V2 forward, golden input")
    gq = g(gold, "fwd_qs")
    assert bool((qs.cpu() == gq)[decided].all())
    same = (qs.cpu() == gq).all(0)                                  # frames on which the reference class chose the same codes at every level
    m = same[:, None, :].expand_as(outs)
    follow = V.quantize3(sd, hp, V.prosody_latent(sd, pf, torch.float64), x, torch.float64, codes=gq)
    e32 = float((g(gold, "fwd_outs").double() - follow["outs"])[m].abs().max())
    assert float((outs.cpu().double() - g(gold, "fwd_outs").double())[m].abs().max()) <= max(4 * e32, 1e-6 * float(x.abs().max())) + e32


# ---- waves -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 33])
def test_inference_waves(conv_precision, gold, n):
    """FACodecDecoderV2.inference and FACodecRedecoder.inference: timbre_norm and the style in one launch"""
    x, spk = g(gold, f"x_{n}"), g(gold, "spk")
    for which, key in (("dec", "v2_wav"), ("red", "red_inf_wav")):
        hp, sd, m = small(gold, which)
        w64 = V.styled_inference(sd, hp, x, spk, torch.float64)
        bound, e32 = wave_bound(w64, V.styled_inference(sd, hp, x, spk, torch.float32))
        w = m.inference(x.to(DEV), spk.to(DEV))
        err, err_g = float((w.cpu().double() - w64).abs().max()), float((w.cpu().double() - g(gold, f"{key}_{n}").double()).abs().max())
        print(f"{which}.inference {n} frames [{conv_precision}]: err vs fp64 {err:.3e}, vs golden {err_g:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}")
        assert w.shape == w64.shape == (2, 1, n * 6) and err <= bound and err_g <= bound + e32
        assert torch.equal(m.inference(x.to(DEV), spk.to(DEV)), w)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("n", [1, 7, 33])
def test_redecoder_waves(conv_precision, gold, n, res):
    """forward, and vq2emb + inference, from the same codes: the two summation orders of the reference"""
    hp, sd, red = small(gold, "red")
    vq, spk = g(gold, f"vq_{n}"), g(gold, "spk")
    w64 = V.redecoder_forward(sd, hp, vq, spk, torch.float64, res)
    bound, e32 = wave_bound(w64, V.redecoder_forward(sd, hp, vq, spk, torch.float32, res))
    w = red(vq.to(DEV), spk.to(DEV), use_residual_code=res)
    err, err_g = float((w.cpu().double() - w64).abs().max()), float((w.cpu().double() - g(gold, f"red_fwd_wav_{n}_{int(res)}").double()).abs().max())
    print(f"redecoder forward {n} frames res={res} [{conv_precision}]: err vs fp64 {err:.3e}, vs golden {err_g:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert w.shape == w64.shape == (2, 1, n * 6) and err <= bound and err_g <= bound + e32
    assert torch.equal(red(vq.to(DEV), spk.to(DEV), use_residual_code=res), w)
    # vq2emb: the latent at the transformer's bound, then inference from the HIP latent at the wave bound
    e64 = V.redecoder_vq2emb(sd, hp, vq, spk, torch.float64, res)
    e_bound, e_e32 = stage_bound(e64, V.redecoder_vq2emb(sd, hp, vq, spk, torch.float32, res))
    emb = red.vq2emb(vq.to(DEV), spk.to(DEV), use_residual=res)
    e_err = float((emb.cpu().double() - e64).abs().max())
    print(f"    vq2emb: err {e_err:.3e}, fp32 restatement {e_e32:.3e}, bound {e_bound:.3e}")
    assert tuple(emb.shape) == (2, 256, n) and e_err <= e_bound
    if f"red_emb_{n}_{int(res)}" in gold:
        assert float((emb.cpu().double() - g(gold, f"red_emb_{n}_{int(res)}").double()).abs().max()) <= e_bound + e_e32
    w64 = V.styled_inference(sd, hp, emb.cpu(), spk, torch.float64)
    bound, e32 = wave_bound(w64, V.styled_inference(sd, hp, emb.cpu(), spk, torch.float32))
    err = float((red.inference(emb, spk.to(DEV)).cpu().double() - w64).abs().max())
    print(f"    vq2emb + inference: err vs fp64 from the HIP latent {err:.3e}; torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_redecoder_runs_the_transformer_once_per_prosody_level():
    """vq_num_q_p = 2: vq2emb's transformer sits inside the prosody loop (facodec.py:739-744), forward's after it"""
    from amphion_amd.models.codec.ns3_codec import FACodecRedecoder

    hp = dict(V.small_redecoder_hp(), vq_num_q_p=2)
    sd = V.synth_redecoder_state_dict(hp, 77)
    red = load(FACodecRedecoder, hp, sd)
    vq, spk = V.synth_codes(hp, 2, 9, 78), 0.5 * C.synth_latent(2, 256, 1, 79)[:, :, 0]
    for fn, got in ((V.redecoder_vq2emb, red.vq2emb(vq.to(DEV), spk.to(DEV))), (V.redecoder_latent, red._latent(vq.to(DEV), spk.to(DEV), True))):
        ref = fn(sd, hp, vq, spk, torch.float64, True)
        bound, e32 = stage_bound(ref, fn(sd, hp, vq, spk, torch.float32, True))
        err = float((got.cpu().double() - ref).abs().max())
        print(f"two prosody levels, {fn.__name__}: err {err:.3e}, fp32 restatement {e32:.3e}, bound {bound:.3e}")
        assert err <= bound
    assert float((V.redecoder_vq2emb(sd, hp, vq, spk) - V.redecoder_latent(sd, hp, vq, spk, use_residual_code=True)).abs().max()) > 1e-2


# ---- conversion end to end at the recipe geometry ------------------------------------------------------------------------------------------
def test_conversion_end_to_end_recipe():
    """The README's two conversion routes on 1000-sample waves, B = 1, every stage against fp64 run from the HIP stage before it"""
    from amphion_amd.models.codec.ns3_codec import FACodecDecoder, FACodecDecoderV2, FACodecEncoderV2, FACodecRedecoder

    ehp, dhp, rhp = R.recipe_encoder_hp(), R.recipe_decoder_hp(), V.recipe_redecoder_hp()
    esd, dsd = V.synth_encoder_v2_state_dict(ehp, 51), V.synth_decoder_v2_state_dict(dhp, 52)
    d1sd, rsd = R.synth_decoder_state_dict(dhp, 53), V.synth_redecoder_state_dict(rhp, 54)
    fa_encoder_v2, fa_decoder_v2 = load(FACodecEncoderV2, ehp, esd), load(FACodecDecoderV2, dhp, dsd)
    fa_decoder, fa_redecoder = load(FACodecDecoder, dhp, d1sd), load(FACodecRedecoder, {}, rsd)          # the redecoder's defaults
    block = {k: v for k, v in esd.items() if k.startswith("block.")}
    wav_a, wav_b = C.synth_wave(1, 1000, 55).to(DEV), C.synth_wave(1, 1000, 56).to(DEV)
    with torch.no_grad():
        enc_out_a = fa_encoder_v2(wav_a)
        prosody_a = fa_encoder_v2.get_prosody_feature(wav_a)
        enc_out_b = fa_encoder_v2(wav_b)
        prosody_b = fa_encoder_v2.get_prosody_feature(wav_b)
        vq_post_emb_a, vq_id_a, _, quantized, spk_embs_a = fa_decoder_v2(enc_out_a, prosody_a, eval_vq=False, vq=True)
        vq_post_emb_b, vq_id_b, _, quantized, spk_embs_b = fa_decoder_v2(enc_out_b, prosody_b, eval_vq=False, vq=True)
        vq_post_emb_a_to_b = fa_decoder_v2.vq2emb(vq_id_a, use_residual=False)
        recon_wav_a_to_b = fa_decoder_v2.inference(vq_post_emb_a_to_b, spk_embs_b)
    assert tuple(enc_out_a.shape) == (1, 256, 5) and tuple(prosody_a.shape) == (1, 20, 5) and tuple(vq_id_a.shape) == (6, 1, 5)
    assert tuple(recon_wav_a_to_b.shape) == (1, 1, 1000)
    # encoder and prosody feature
    z64 = R.encoder_forward(block, ehp, wav_a.cpu(), torch.float64)
    bound, e32 = wave_bound(z64, R.encoder_forward(block, ehp, wav_a.cpu(), torch.float32))
    err = float((enc_out_a.cpu().double() - z64).abs().max())
    print(f"recipe encoder: err {err:.3e}, torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert float((prosody_a.cpu().double() - V.prosody_feature(wav_a.cpu())).abs().max()) <= 1e-4
    # quantize from the HIP latent and prosody feature; the speaker embedding from the HIP latent
    outs, qs, _, _ = check_quantize(fa_decoder_v2, dhp, dsd, enc_out_a, prosody_a, "recipe V2 quantize")
    assert torch.equal(qs, vq_id_a) and torch.equal(outs, vq_post_emb_a)
    s64 = R.speaker_embedding(dsd, enc_out_b.cpu(), torch.float64)
    bound, e32 = stage_bound(s64, R.speaker_embedding(dsd, enc_out_b.cpu(), torch.float32))
    assert float((spk_embs_b.cpu().double() - s64).abs().max()) <= bound
    # the converted wave from the HIP latent and the HIP speaker embedding
    w64 = V.styled_inference(dsd, dhp, vq_post_emb_a_to_b.cpu(), spk_embs_b.cpu(), torch.float64)
    bound, e32 = wave_bound(w64, V.styled_inference(dsd, dhp, vq_post_emb_a_to_b.cpu(), spk_embs_b.cpu(), torch.float32))
    err = float((recon_wav_a_to_b.cpu().double() - w64).abs().max())
    print(f"recipe V2 conversion wave: err {err:.3e}, torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert err <= bound
    # the redecoder route, from FACodecDecoder's codes
    with torch.no_grad():
        _, vq_a, _, _, _ = fa_decoder(enc_out_a, eval_vq=False, vq=True)
        _, _, _, _, spk_b = fa_decoder(enc_out_b, eval_vq=False, vq=True)
        emb = fa_redecoder.vq2emb(vq_a, spk_b, use_residual=False)
        wav = fa_redecoder.inference(emb, spk_b)
    e64 = V.redecoder_vq2emb(rsd, rhp, vq_a.cpu(), spk_b.cpu(), torch.float64, False)
    bound, e32 = stage_bound(e64, V.redecoder_vq2emb(rsd, rhp, vq_a.cpu(), spk_b.cpu(), torch.float32, False))
    err = float((emb.cpu().double() - e64).abs().max())
    print(f"recipe redecoder vq2emb: err {err:.3e}, fp32 restatement {e32:.3e}, bound {bound:.3e}")
    assert tuple(emb.shape) == (1, 256, 5) and err <= bound
    w64 = V.styled_inference(rsd, rhp, emb.cpu(), spk_b.cpu(), torch.float64)
    bound, e32 = wave_bound(w64, V.styled_inference(rsd, rhp, emb.cpu(), spk_b.cpu(), torch.float32))
    err = float((wav.cpu().double() - w64).abs().max())
    print(f"recipe redecoder wave: err {err:.3e}, torch fp32 {e32:.3e}, bound {bound:.3e}")
    assert tuple(wav.shape) == (1, 1, 1000) and err <= bound


# ---- housekeeping --------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_refusals(gold):
    from amphion_amd._lib import AMP_ERR_INVALID, AmpError
    from amphion_amd.models.codec.ns3_codec import FACodecDecoderV2, FACodecEncoderV2, FACodecRedecoder

    ehp, dhp, rhp = R.small_encoder_hp(), R.small_decoder_hp(), V.small_redecoder_hp()
    esd, dsd, rsd = V.synth_encoder_v2_state_dict(ehp, 3), V.synth_decoder_v2_state_dict(dhp, 4), V.synth_redecoder_state_dict(rhp, 5)
    for cls, h, sd in ((FACodecEncoderV2, ehp, esd), (FACodecDecoderV2, dhp, dsd), (FACodecRedecoder, rhp, rsd)):
        for form in (sd, R.fold(sd)):                       # weight-normed and folded convs
            back = load(cls, h, form).state_dict()
            assert list(back) == list(form) and all(torch.equal(back[k].cpu(), form[k]) for k in form)
    extra = dict(dsd)
    extra["f0_predictor.heads.0.weight"] = torch.zeros(1, 256)
    extra["x_timbre_predictor.1.heads.0.bias"] = torch.zeros(245200)
    dec = load(FACodecDecoderV2, dhp, extra)
    assert not any(k.startswith(R.PREDICTOR_PREFIXES) for k in dec.state_dict())
    with pytest.raises(RuntimeError):
        load(FACodecDecoderV2, dhp, dict(dsd, **{"unknown.weight": torch.zeros(1)}))
    red = load(FACodecRedecoder, rhp, rsd)
    x, pf, spk = torch.zeros(1, 256, 4, device=DEV), torch.zeros(1, 20, 4, device=DEV), torch.zeros(1, 256, device=DEV)
    vq = torch.zeros(6, 1, 4, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError):
        dec(x, pf, vq=False, speaker_embedding=spk, quantized=[x, x, x])
    with pytest.raises(ValueError):
        dec(x, pf[:, :, :3])                                  # another frame count
    with pytest.raises(ValueError):
        dec(x, torch.zeros(1, 19, 4, device=DEV))             # another channel count
    with pytest.raises(ValueError):
        dec(x[:, :255], pf)
    with pytest.raises(TypeError):
        dec(x, pf.double())
    with pytest.raises(RuntimeError):
        dec(x, pf.cpu())
    with pytest.raises(RuntimeError):
        dec.inference(x.cpu(), spk)
    with pytest.raises(ValueError):
        dec.inference(x, torch.zeros(2, 256, device=DEV))
    with pytest.raises(ValueError):
        red.inference(x[:, :255], spk)
    with pytest.raises(ValueError):
        red(vq[:2], spk)                                      # fewer levels than prosody + content
    with pytest.raises(ValueError):
        red.vq2emb(vq[:3], spk)                               # use_residual=True needs the residual levels
    red.vq2emb(vq[:3], spk, use_residual=False)
    with pytest.raises(TypeError):
        red(vq.float(), spk)
    with pytest.raises(RuntimeError):
        red(vq.cpu(), spk)
    with pytest.raises(ValueError):
        red(vq, torch.zeros(1, 255, device=DEV))
    bad = vq.clone()
    bad[1, 0, 2] = 2 ** rhp["codebook_size_content"]
    with pytest.raises(AmpError) as e:
        red(bad, spk)
    assert e.value.status == AMP_ERR_INVALID
    red(vq, spk)
    dec.train()
    with pytest.raises(NotImplementedError):
        dec(x, pf)
    red.train()
    with pytest.raises(NotImplementedError):
        red(vq, spk)
