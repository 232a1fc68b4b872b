"""DualCodec on the MI355X (amp_dwconv_layer_norm_c_causal, amp_fvq_encode_ex, amp_fvq_decode_add, amp_semantic_prepare and the drop-in modules of
amphion_amd/models/codec/dualcodec/dualcodec/model_codec/) against the fp64 restatement of tests/dualcodec_ref.py.

Bit identities (requirements, not tolerances): the causal depthwise + LayerNorm launch against the centred launch on a copy left-padded by 6 zeros,
read at columns t + 3; amp_fvq_encode_ex against torch's crop / subtract -> amp_fvq_encode -> torch's add, and its NULL forms against amp_fvq_encode;
amp_fvq_decode_add against amp_fvq_decode -> torch's add; row 0 of a batch of 2 against the batch of 1.
Quantizer codes: the margin rule of codec_ref.margin_rule (tests/test_gpu_codec.py) -- undecided frames <= 2 % asserted on the fp64 reference first,
codes identical on decided pairs.  In the module tests the fp64 quantizer is applied to the HIP latent, so encoder rounding is not charged to it.
latents / z_q / amp_semantic_prepare: 4 x the fp32 CPU restatement's own error against fp64, floor 1e-6 max|input| (computed and printed).
LayerNorm front: 2e-5 absolute, the bound of tests/test_gpu_vocos.py::test_dwconv7_layer_norm_against_fp64.
ConvNeXt block / convnext_encoder output: 1e-4 absolute with the torch fp32 error printed next to it, the rule tests/test_gpu_vocos.py applies to the
Vocos backbone's output (test_end_to_end_against_fp64); the draws of dualcodec_ref keep these activations at a few units.
Waveform: max(1e-4 max|pre-tanh fp64|, 4 e32), the decoder rule of tests/test_gpu_dac.py.
The small nets have a 1024-wide DAC latent: the reference's convnext_decoder ends in 1024 channels that are subtracted from it (dualcodec_ref)."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import codec_ref as C  # noqa: E402
import dac_ref as D  # noqa: E402
import dualcodec_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _L():
    from amphion_amd import _lib

    return _lib


def _stream():
    return _L().current_stream_ptr(torch.device(DEV))


# ---- causal depthwise conv -> LayerNorm --------------------------------------------------------------------------------------------
def _ln_case(Cn, T, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cn, T, generator=g)
    w = torch.randn(Cn, 1, 7, generator=g) / 7 ** 0.5
    b = torch.randn(Cn, generator=g) * 0.1
    lw = 1 + 0.1 * torch.randn(Cn, generator=g)
    lb = 0.05 * torch.randn(Cn, generator=g)
    return x, w, b, lw, lb


def _ln_run(fn, x, w, b, lw, lb):
    _lib = _L()
    B, Cn, T = x.shape
    y = torch.empty_like(x)
    _lib.check(fn(_p(x), _p(w), _p(b), 7, 1, _p(lw), _p(lb), None, B, Cn, T, 1e-6, 0, _p(y), _stream()))
    return y


@pytest.mark.parametrize("Cn", [32, 768])
def test_causal_dwconv_layer_norm(Cn):
    """T = 1 and 5: shorter than the 6-column history; T = 70: three 32-column tiles, the last one partial"""
    L = _L().lib()
    for T in (1, 5, 70):
        x, w, b, lw, lb = _ln_case(Cn, T, 10 * Cn + T)
        dev = [t.to(DEV) for t in (x, w, b, lw, lb)]
        y = _ln_run(L.amp_dwconv_layer_norm_c_causal, *dev)
        padded = F.pad(dev[0], (6, 0)).contiguous()
        yp = _ln_run(L.amp_dwconv_layer_norm_c, padded, *dev[1:])
        assert torch.equal(y, yp[..., 3:3 + T]), (Cn, T)
        ref = R.dwconv_layer_norm(w.double(), b.double(), lw.double(), lb.double(), x.double(), causal=True)
        err = float((y.cpu().double() - ref).abs().max())
        print(f"causal dwconv + LN C={Cn} T={T}: err vs fp64 {err:.3e}")
        assert torch.isfinite(y).all() and err < 2e-5, (Cn, T, err)
        one = _ln_run(L.amp_dwconv_layer_norm_c_causal, dev[0][:1].contiguous(), *dev[1:])
        assert torch.equal(one[0], y[0])                       # batch independence


# ---- the quantizer entry points -------------------------------------------------------------------------------------------------------
def make_rvq(qhp, sd):
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import ResidualVectorQuantize

    m = ResidualVectorQuantize(input_dim=qhp["D"], n_codebooks=qhp["N"], codebook_size=qhp["K"], codebook_dim=qhp["d"])
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    return m, m._handle.get(list(m.quantizers), torch.device(DEV))


def run_ex(h, qhp, z, T, sub, n=None, stride=None):
    """amp_fvq_encode_ex on device tensors -> (codes [n, B, T], zq, allq, latents)"""
    _lib = _L()
    B, Dn = z.shape[0], z.shape[1]
    n = qhp["N"] if n is None else n
    stride = z.shape[2] if stride is None else stride
    codes = torch.full((n, B, T), -1, dtype=torch.int64, device=DEV)
    zq = torch.empty(B, Dn, T, device=DEV)
    allq = torch.empty(n, B, Dn, T, device=DEV)
    lat = torch.empty(B, n * qhp["d"], T, device=DEV)
    _lib.check(_lib.lib().amp_fvq_encode_ex(h, _p(z), stride, _p(sub), B, T, n, _p(codes), _p(zq), _p(allq), _p(lat), _stream()))
    return codes, zq, allq, lat


def run_plain(h, qhp, z, n=None):
    """amp_fvq_encode on a contiguous device tensor -> (codes, zq, allq)"""
    _lib = _L()
    B, Dn, T = z.shape
    n = qhp["N"] if n is None else n
    codes = torch.full((n, B, T), -1, dtype=torch.int64, device=DEV)
    zq = torch.empty(B, Dn, T, device=DEV)
    allq = torch.empty(n, B, Dn, T, device=DEV)
    _lib.check(_lib.lib().amp_fvq_encode(h, _p(z), B, T, n, _p(codes), _p(zq), _p(allq), _stream()))
    return codes, zq, allq


_REF = {}


def fvq_reference(name, T, with_sub):
    """the CPU references of one op case, computed once: margin rule, fp64 / fp32 results with latents"""
    key = (name, T, with_sub)
    if key not in _REF:
        qhp, sd, z, sub = R.fvq_op_inputs(name, T)
        qsd = R.quantizer_sd(sd, "quantizers.")
        zin = (z[..., :T] - sub) if with_sub else z[..., :T].contiguous()
        r64c, _, tau, decided = C.margin_rule(qsd, qhp, zin)
        r64 = R.rvq_forward(qsd, qhp, zin, torch.float64)
        r32 = R.rvq_forward(qsd, qhp, zin, torch.float32, codes=r64["codes"])
        _REF[key] = (qhp, sd, z, sub, zin, r64c, r64, r32, tau, decided)
    return _REF[key]


@pytest.mark.parametrize("with_sub", [False, True], ids=["plain", "sub"])
@pytest.mark.parametrize("T", R.FVQ_OP_LENGTHS)
@pytest.mark.parametrize("name", list(R.FVQ_OP_CASES))
def test_fvq_encode_ex(name, T, with_sub):
    qhp, sd, z, sub, zin, r64c, r64, r32, tau, decided = fvq_reference(name, T, with_sub)
    frames_ok = decided[-1]
    undecided = 1.0 - float(frames_ok.double().mean())
    print(f"{name} T={T} sub={with_sub}: tau {tau:.3e}, smallest fp64 margin {float(r64c['margin'].min()):.3e}, undecided frames {undecided:.4f}")
    assert undecided <= 0.02, "the fp64 reference itself leaves too many frames undecided for this seed"
    m, h = make_rvq(qhp, sd)
    zd = z.to(DEV)                                             # [B, D, T + 2]: the crop rides in the row stride
    sd_ = sub.to(DEV) if with_sub else None
    codes, zq, allq, lat = run_ex(h, qhp, zd, T, sd_)
    # the three-step sequence the launch replaces, bit for bit
    zc = (zd[..., :T] - sd_).contiguous() if with_sub else zd[..., :T].contiguous()
    assert torch.equal(zc.cpu(), zin)                          # the same single fp32 subtraction on the host
    codes3, zq3, allq3 = run_plain(h, qhp, zc)
    if with_sub:
        zq3 = zq3 + sd_
    assert torch.equal(codes, codes3) and torch.equal(zq, zq3) and torch.equal(allq, allq3)
    # the NULL forms are amp_fvq_encode
    if not with_sub:
        c0, q0, a0, l0 = run_ex(h, qhp, zc, T, None)           # stride T
        assert torch.equal(c0, codes3) and torch.equal(q0, zq3) and torch.equal(a0, allq3) and torch.equal(l0, lat)
    # the module's forward is this launch
    out = m(zc) if not with_sub else m(zd, subtracted_latent=sd_)
    assert torch.equal(out[0], zq) and torch.equal(out[1], codes.transpose(0, 1)) and torch.equal(out[2], lat) and torch.equal(out[5], allq[0])
    assert out[1].dtype == torch.int64 and out[1].shape == (2, qhp["N"], T) and out[2].shape == (2, qhp["N"] * qhp["d"], T)
    # against fp64
    codes_c = codes.cpu()
    assert bool((codes_c == r64["codes"])[decided].all())
    zmax = float(zin.abs().max())
    add = sub.double() if with_sub else 0.0
    delta = 0.0
    for tag, got, ref64, ref32 in (("zq", zq, r64["zq"] + add, (r32["zq"] + sub) if with_sub else r32["zq"]),
                                   ("latents", lat, r64["latents"], r32["latents"])):
        mask = frames_ok[:, None, :].expand_as(ref64)
        e32 = float((ref32.double() - ref64)[mask].abs().max())
        bound = max(4 * e32, 1e-6 * zmax)
        err = float((got.cpu().double() - ref64)[mask].abs().max())
        print(f"    {tag}: err {err:.3e}, fp32 restatement {e32:.3e}, bound {bound:.3e}")
        assert err <= bound, (tag, err, bound)
        delta = bound                                          # the latents' bound, last
    # the losses: mean of (z_e - q)^2 with z_e off by at most delta -> 2 max|z_e - q| delta + delta^2 per level, plus fp32 evaluation (1e-6 relative)
    qsd = R.quantizer_sd(sd, "quantizers.")
    f64 = R.rvq_forward(qsd, qhp, zin, torch.float64, codes=codes_c)
    loss64 = float(R.rvq_losses(qsd, f64))
    amax = float(f64["latents"].abs().max()) + max(float(v.abs().max()) for k, v in qsd.items() if k.endswith("codebook.weight"))
    tol = qhp["N"] * (2 * amax * delta + delta * delta) + 1e-6 * loss64
    print(f"    losses: {float(out[3]):.6e} vs fp64 {loss64:.6e}, tolerance {tol:.3e}")
    assert abs(float(out[3]) - loss64) <= tol and float(out[3]) == float(out[4])
    _L().range_check(DEV)


def test_fvq_encode_ex_fewer_levels_and_batch_independence():
    qhp, sd, z, sub, zin, _, r64, _, _, decided = fvq_reference("small", 33, True)
    m, h = make_rvq(qhp, sd)
    zd, sd_ = z.to(DEV), sub.to(DEV)
    full = run_ex(h, qhp, zd, 33, sd_)
    two = run_ex(h, qhp, zd, 33, sd_, n=2)
    assert torch.equal(two[0], full[0][:2]) and torch.equal(two[2], full[2][:2]) and torch.equal(two[3], full[3][:, :16])
    assert bool((two[0].cpu() == r64["codes"][:2])[decided[:2]].all())
    codes1, zq1, allq1, lat1 = run_ex(h, qhp, zd[:1].contiguous(), 33, sd_[:1].contiguous())
    assert torch.equal(codes1[:, 0], full[0][:, 0]) and torch.equal(zq1[0], full[1][0]) and torch.equal(allq1[:, 0], full[2][:, 0])
    assert torch.equal(lat1[0], full[3][0])


def test_fvq_encode_ex_ties_resolve_to_lowest_index():
    qhp, sd, z, sub, _, _, _, _, _, _ = fvq_reference("small", 33, True)
    sd = dict(sd)
    K = qhp["K"]
    for i in range(qhp["N"]):
        cb = sd[f"quantizers.{i}.codebook.weight"].clone()
        cb[K // 2:] = cb[: K // 2]                             # every row twice: distances tie exactly
        sd[f"quantizers.{i}.codebook.weight"] = cb
    _, h = make_rvq(qhp, sd)
    codes = run_ex(h, qhp, z.to(DEV), 33, sub.to(DEV))[0]
    assert int(codes.max()) < K // 2 and int(codes.min()) >= 0
    half = {k: (v[: K // 2] if k.endswith("codebook.weight") else v) for k, v in sd.items()}
    hq = dict(qhp, K=K // 2)
    _, h2 = make_rvq(hq, half)
    assert torch.equal(codes, run_ex(h2, hq, z.to(DEV), 33, sub.to(DEV))[0])


def test_fvq_decode_add():
    _lib = _L()
    qhp, sd, z, sub, _, _, r64, _, _, _ = fvq_reference("small", 33, True)
    m, h = make_rvq(qhp, sd)
    codes = r64["codes"].to(DEV).contiguous()                  # [n, B, T]
    n, B, T = codes.shape
    add = sub.to(DEV)

    def dec(c, a, levels=n):
        out = torch.empty(B, qhp["D"], T, device=DEV)
        _lib.check(_lib.lib().amp_fvq_decode_add(h, _p(c), levels, B, T, _p(a), _p(out), _stream()))
        return out

    plain = torch.empty(B, qhp["D"], T, device=DEV)
    _lib.check(_lib.lib().amp_fvq_decode(h, _p(codes), n, B, T, _p(plain), _stream()))
    assert torch.equal(dec(codes, None), plain) and torch.equal(dec(codes, add), plain + add)
    _lib.check(_lib.lib().amp_fvq_check(h, _stream()))
    # the module: from_codes and the folded form
    z_q, z_p, back = m.from_codes(codes.transpose(0, 1))
    assert torch.equal(z_q, plain) and back.shape == (B, n, T) and z_p.shape == (B, n * qhp["d"], T)
    assert torch.equal(m.run_decode(codes.transpose(0, 1), add=add), plain + add)
    ref = C.vq2emb(R.quantizer_sd(sd, "quantizers."), qhp, codes.cpu(), torch.float64)
    e32 = float((C.vq2emb(R.quantizer_sd(sd, "quantizers."), qhp, codes.cpu(), torch.float32).double() - ref).abs().max())
    bound = max(4 * e32, 1e-6 * float(z.abs().max()))
    err = float((plain.cpu().double() - ref).abs().max())
    print(f"decode: err vs fp64 {err:.3e}, fp32 restatement {e32:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(dec(codes, add, levels=2), dec(codes[:2].contiguous(), add, levels=2))
    # a code outside the codebook: the flag is raised and row 0 is read in its place
    zero = codes.clone()
    zero[1, 1, 17] = 0
    want = dec(zero, add)
    for bad in (qhp["K"], -1, 2 ** 40):
        c = codes.clone()
        c[1, 1, 17] = bad
        got = dec(c, add)
        assert _lib.lib().amp_fvq_check(h, _stream()) == _lib.AMP_ERR_INVALID
        assert torch.equal(got, want)
        with pytest.raises(_lib.AmpError) as e:
            m.from_codes(c.transpose(0, 1))
        assert e.value.status == _lib.AMP_ERR_INVALID
    _lib.check(_lib.lib().amp_fvq_check(h, _stream()))         # cleared


# ---- semantic feature preparation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stats", [True, False], ids=["normalised", "raw"])
@pytest.mark.parametrize("T,f", [(9, 2), (10, 4), (7, 1)])
def test_semantic_prepare(T, f, stats):
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import prepare_semantic_features

    hidden, mean, std = R.synth_hidden(2, T, 1024, 900 + 10 * T + f)
    if not stats:
        mean = std = None
    ref = R.prepare_semantic_features(hidden, mean, std, f, torch.float64)
    e32 = float((R.prepare_semantic_features(hidden, mean, std, f, torch.float32).double() - ref).abs().max())
    bound = max(4 * e32, 1e-6 * float(hidden.abs().max()))
    dev = [None if t is None else t.to(DEV) for t in (mean, std)]
    y = prepare_semantic_features(hidden.to(DEV), dev[0], dev[1], f)
    err = float((y.cpu().double() - ref).abs().max())
    print(f"semantic prepare T={T} f={f} stats={stats}: err {err:.3e}, fp32 restatement {e32:.3e}, bound {bound:.3e}")
    assert y.shape == (2, 1024, T // f) and err <= bound
    # the dropped tail frames are not read into the result
    spoiled = hidden.clone()
    if T % f:
        spoiled[:, T - T % f:] = float("nan")
    assert torch.equal(prepare_semantic_features(spoiled.to(DEV), dev[0], dev[1], f), y)
    # one statistic alone, and batch independence
    if stats:
        ref_m = R.prepare_semantic_features(hidden, mean, None, f, torch.float64)
        e32_m = float((R.prepare_semantic_features(hidden, mean, None, f, torch.float32).double() - ref_m).abs().max())
        only_mean = prepare_semantic_features(hidden.to(DEV), dev[0], None, f).cpu().double()
        assert float((only_mean - ref_m).abs().max()) <= max(4 * e32_m, 1e-6 * float(hidden.abs().max()))
    assert torch.equal(prepare_semantic_features(hidden[:1].to(DEV), dev[0], dev[1], f)[0], y[0])


def test_semantic_prepare_refuses_short_input():
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import prepare_semantic_features

    _lib = _L()
    x = torch.zeros(2, 3, 1024, device=DEV)
    out = torch.zeros(2, 1024, 1, device=DEV)
    with pytest.raises(ValueError):
        prepare_semantic_features(x, factor=4)
    assert _lib.lib().amp_semantic_prepare(_p(x), None, None, 2, 3, 1024, 4, _p(out), _stream()) == _lib.AMP_ERR_INVALID


# ---- modules -------------------------------------------------------------------------------------------------------------------------
NETS = [True, False]


def make_model(hp, sd):
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import DualCodec

    m = DualCodec(**hp)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


_SD = {}


def net(causal):
    if causal not in _SD:
        hp = R.small_hp(causal)
        _SD[causal] = (hp, R.synth_dualcodec_state_dict(hp, R.MODEL_SEED))
    return _SD[causal]


@pytest.mark.parametrize("causal", NETS, ids=["causal", "centred"])
def test_convnext_block_and_encoder_vs_fp64(conv_precision, causal):
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import ConvNeXtBlock

    for gamma in (True, False):
        bsd = R.synth_convnext_block(64, "", R.MODEL_SEED + 50, gamma=gamma)
        blk = ConvNeXtBlock(64, R.INTERMEDIATE, layer_scale_init_value=0.5 if gamma else 0.0, is_causal=causal)
        blk.load_state_dict(bsd)
        blk = blk.to(DEV).eval()
        for T in (5, 33):
            x = C.synth_latent(2, 64, T, R.MODEL_SEED + 51 + T)
            ref = R.convnext_block({k: v.double() for k, v in bsd.items()}, "", x.double(), causal)
            e32 = float((R.convnext_block(bsd, "", x, causal).double() - ref).abs().max())
            y = blk(x.to(DEV)).cpu().double()
            err = float((y - ref).abs().max())
            print(f"ConvNeXtBlock causal={causal} gamma={gamma} T={T} [{conv_precision}]: err {err:.3e} (torch fp32 {e32:.3e}), peak {float(ref.abs().max()):.2f}")
            assert y.shape == ref.shape and err <= 1e-4, err
    hp, sd = net(causal)
    m = make_model(hp, sd)
    for T in R.MODEL_LENGTHS:
        _, feats = R.model_inputs(hp, T)
        ref = R.convnext_encoder(sd, hp, feats, torch.float64)
        e32 = float((R.convnext_encoder(sd, hp, feats, torch.float32).double() - ref).abs().max())
        h = m.run_convnext_encoder(feats.to(DEV))
        assert torch.equal(h, m.convnext_encoder(feats.to(DEV)))          # nn.Sequential's own walk is the same launches
        err = float((h.cpu().double() - ref).abs().max())
        print(f"convnext_encoder causal={causal} T={T} [{conv_precision}]: err {err:.3e} (torch fp32 {e32:.3e}), peak {float(ref.abs().max()):.2f}")
        assert err <= 1e-4, err
    _L().range_check(DEV)


def _decided(tag, qsd, qhp, z, n=None):
    r64, _, tau, decided = C.margin_rule(qsd, qhp, z, n)
    undecided = 1.0 - float(decided[-1].double().mean())
    print(f"    {tag}: tau {tau:.3e}, smallest fp64 margin {float(r64['margin'].min()):.3e}, undecided frames {undecided:.4f}")
    assert undecided <= 0.02
    return r64, decided


@pytest.mark.parametrize("T,extra", [(9, 2), (33, 0)])
@pytest.mark.parametrize("causal", NETS, ids=["causal", "centred"])
def test_semantic_quantize_and_encode(conv_precision, causal, T, extra):
    """the fp64 quantizers applied to the HIP latents; T = 9 with two more encoder frames than semantic frames (the crop)"""
    hp, sd = net(causal)
    m = make_model(hp, sd)
    wave, feats = R.model_inputs(hp, T, extra_frames=extra)
    wd, fd = wave.to(DEV), feats.to(DEV)
    print(f"encode causal={causal} T={T} (+{extra}) [{conv_precision}]")
    sem = m.semantic_quantize(fd)
    assert sem.shape == (2, T) and sem.dtype == torch.int64
    r64, decided = _decided("semantic", R.quantizer_sd(sd, "semantic_vq.quantizers."), R.semantic_q_hp(hp), m.run_convnext_encoder(fd).cpu())
    assert bool((sem.cpu()[None] == r64["codes"])[decided].all())
    # the acoustic side on ITS inputs: the HIP encoder latent, cropped, minus the HIP semantic latent
    semantic, sem_codes, _ = m._semantic(fd)
    z_enc = m.dac.encoder(m.dac.preprocess(wd, hp["sample_rate"]))
    assert z_enc.shape[2] == T + extra and torch.equal(sem_codes[:, 0], sem)
    zin = (z_enc[..., :T] - semantic).cpu()
    qsd, qhp = R.quantizer_sd(sd, "dac.quantizer.quantizers."), R.acoustic_q_hp(hp)
    a64, adec = _decided("acoustic", qsd, qhp, zin)
    results = {}
    for nq in (None, 1, 2):
        s_codes, a_codes = m.encode(wd, num_quantizers=nq, sample_rate=hp["sample_rate"], semantic_repr=fd)
        assert torch.equal(s_codes, sem_codes) and s_codes.shape == (2, 1, T)
        results[nq] = a_codes
    assert results[1] is None
    full, first = results[None], results[2]
    assert full.shape == (2, hp["n_codebooks"], T) and full.dtype == torch.int64 and first.shape == (2, 1, T)
    assert torch.equal(first, full[:, :1])
    assert bool((full.cpu().transpose(0, 1) == a64["codes"])[adec].all())
    # DAC.encode's six-tuple: the fp64 quantizer following the HIP codes on the HIP latent
    z, codes, latents, closs, bloss, first_q = m.dac.encode(wd, sample_rate=hp["sample_rate"], subtracted_latent=semantic)
    assert torch.equal(codes, full) and latents.shape == (2, hp["n_codebooks"] * hp["codebook_dim"], T) and first_q.shape == z.shape == semantic.shape
    f64 = R.rvq_forward(qsd, qhp, zin, torch.float64, codes=full.cpu().transpose(0, 1))
    f32 = R.rvq_forward(qsd, qhp, zin, torch.float32, codes=full.cpu().transpose(0, 1))
    sem64 = semantic.cpu().double()
    floor = 1e-6 * float(zin.abs().max())
    delta = 0.0
    for tag, got, ref64, ref32 in (("z", z, f64["zq"] + sem64, f32["zq"] + semantic.cpu()), ("latents", latents, f64["latents"], f32["latents"]),
                                   ("first_layer_quantized", first_q, f64["z_q_1"], f32["z_q_1"])):
        e32 = float((ref32.double() - ref64).abs().max())
        bound = max(4 * e32, floor)
        err = float((got.cpu().double() - ref64).abs().max())
        print(f"    {tag}: err {err:.3e}, fp32 restatement {e32:.3e}, bound {bound:.3e}")
        assert err <= bound, (tag, err, bound)
        if tag == "latents":
            delta = bound
    # the losses: mean of (z_e - q)^2 with z_e off by at most delta -> 2 max|z_e - q| delta + delta^2 per level, plus fp32 evaluation (1e-6 relative)
    loss64 = float(R.rvq_losses(qsd, f64))
    amax = float(f64["latents"].abs().max()) + max(float(v.abs().max()) for k, v in qsd.items() if k.endswith("codebook.weight"))
    tol = hp["n_codebooks"] * (2 * amax * delta + delta * delta) + 1e-6 * loss64
    print(f"    losses: {float(closs):.6e} vs fp64 {loss64:.6e}, tolerance {tol:.3e}")
    assert abs(float(closs) - loss64) <= tol and float(closs) == float(bloss)
    _L().range_check(DEV)


@pytest.mark.parametrize("T", R.MODEL_LENGTHS)
@pytest.mark.parametrize("causal", NETS, ids=["causal", "centred"])
def test_decode_from_codes(conv_precision, causal, T):
    hp, sd = net(causal)
    m = make_model(hp, sd)
    wave, feats = R.model_inputs(hp, T)
    e = R.encode(sd, hp, wave, feats)                          # fp64 codes: both sides decode the same integers
    sem, ac = e["semantic_codes"], e["acoustic_codes"].contiguous()
    for tag, codes in (("all levels", ac), ("two levels", ac[:, :2].contiguous()), ("semantic only", None)):
        pre = R.decode_from_codes(sd, hp, sem, codes, torch.float64, pre_tanh=True)
        y64 = torch.tanh(pre)
        e32 = float((R.decode_from_codes(sd, hp, sem, codes, torch.float32).double() - y64).abs().max())
        bound = max(1e-4 * float(pre.abs().max()), 4 * e32)
        y = m.decode_from_codes(sem.to(DEV), None if codes is None else codes.to(DEV))
        err = float((y.cpu().double() - y64).abs().max())
        print(f"decode_from_codes causal={causal} T={T} {tag} [{conv_precision}]: err {err:.3e}, torch fp32 {e32:.3e}, bound {bound:.3e}")
        assert y.shape == y64.shape and err <= bound, (tag, err, bound)
    _L().range_check(DEV)


def test_forward_returns_the_two_result_objects():
    from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import AttrDict

    hp, sd = net(True)
    m = make_model(hp, sd)
    wave, feats = R.model_inputs(hp, 9)
    wd, fd = wave.to(DEV), feats.to(DEV)
    ac, se = m(wd, sample_rate=hp["sample_rate"], semantic_repr=fd)
    s_codes, a_codes = m.encode(wd, sample_rate=hp["sample_rate"], semantic_repr=fd)
    assert isinstance(ac, AttrDict) and isinstance(se, AttrDict)
    assert torch.equal(ac.codes, a_codes) and torch.equal(se.codes, s_codes) and torch.equal(ac["codes"], ac.codes)
    assert ac.x.shape == wave.shape and se.x.shape == (2, 1024, 9) and se.latents.shape == (2, 8, 9) and not se.bypassed_quantize
    assert torch.isfinite(ac.x).all() and float(ac.x.abs().max()) <= 1.0 and float(se.penalty) == float(se["vq/codebook_loss"]) > 0
    ac1, se1 = m(wd, sample_rate=hp["sample_rate"], n_quantizers=1, semantic_repr=fd)
    assert ac1.codes is None and ac1.latents is None and se1.bypassed_quantize and torch.equal(se1.codes, s_codes) and ac1.x.shape == wave.shape
    assert torch.equal(ac1.z, se1.x)


@pytest.mark.parametrize("causal", NETS, ids=["causal", "centred"])
def test_batch_independence(causal):
    hp, sd = net(causal)
    m = make_model(hp, sd)
    wave, feats = R.model_inputs(hp, 33)
    wd, fd = wave.to(DEV), feats.to(DEV)
    s2, a2 = m.encode(wd, sample_rate=hp["sample_rate"], semantic_repr=fd)
    s1, a1 = m.encode(wd[:1].contiguous(), sample_rate=hp["sample_rate"], semantic_repr=fd[:1].contiguous())
    assert torch.equal(s1[0], s2[0]) and torch.equal(a1[0], a2[0])
    y2 = m.decode_from_codes(s2, a2)
    y1 = m.decode_from_codes(s2[:1].contiguous(), a2[:1].contiguous())
    assert torch.equal(y1[0], y2[0])


def test_state_dict_round_trips_and_refusals():
    hp, sd = net(True)
    m = make_model(hp, sd)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k].cpu(), sd[k]) for k in sd)
    wave, feats = R.model_inputs(hp, 9)
    wd, fd = wave.to(DEV), feats.to(DEV)
    s_codes, a_codes = m.encode(wd, sample_rate=hp["sample_rate"], semantic_repr=fd)
    y = m.decode_from_codes(s_codes, a_codes)
    folded = D.fold_state_dict(sd)
    m2 = make_model(hp, folded)
    assert set(m2.state_dict()) == set(folded)
    pre = R.decode_from_codes(sd, hp, s_codes.cpu(), a_codes.cpu(), torch.float64, pre_tanh=True)
    e32 = float((R.decode_from_codes(sd, hp, s_codes.cpu(), a_codes.cpu(), torch.float32).double() - torch.tanh(pre)).abs().max())
    bound = max(1e-4 * float(pre.abs().max()), 4 * e32)
    for tag, out in (("weight-normed", y), ("folded", m2.decode_from_codes(s_codes, a_codes))):
        err = float((out.cpu().double() - torch.tanh(pre)).abs().max())
        print(f"round trip {tag}: err {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    # a parameter changed in place rebuilds the quantizer handle
    with torch.no_grad():
        m.semantic_vq.quantizers[0].codebook.weight.mul_(-1.0)
    assert not torch.equal(m.decode_from_codes(s_codes, a_codes), y)
    with torch.no_grad():
        m.semantic_vq.quantizers[0].codebook.weight.mul_(-1.0)
    assert torch.equal(m.decode_from_codes(s_codes, a_codes), y)
    m.train()
    for call in (lambda: m.encode(wd, semantic_repr=fd), lambda: m.semantic_quantize(fd), lambda: m.decode_from_codes(s_codes, a_codes),
                 lambda: m(wd, semantic_repr=fd), lambda: m.dac.quantizer(torch.zeros(1, 1024, 4, device=DEV))):
        with pytest.raises(NotImplementedError):
            call()
    m.eval()
    with pytest.raises(RuntimeError):
        m.encode(wave, semantic_repr=feats)                    # host tensors: no CPU fallback
    with pytest.raises(ValueError):
        m.encode(wd[..., : 7 * R.hop(hp)].contiguous(), sample_rate=hp["sample_rate"], semantic_repr=fd)       # fewer encoder frames than semantic frames
    _L().range_check(DEV)
