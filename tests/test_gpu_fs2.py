"""FastSpeech2 / JETS inference on the GPU: amp_mh_attention (head dimension 128, no rotation), amp_fs2_durations,
amp_bucketize_embed_add, amp_layer_norm_c_head op by op, then the FFT block, the variance predictor and the whole model against the fp64
restatement (tests/fs2_ref.py).  Bounds: 4 x the fp32 CPU evaluation's own distance from fp64, scaled by max(1, |ref|max) -- the rule of
test_gpu_fmt.py; discrete outputs and everything torch computes with one rounding per element are compared for equality."""
import os
import zlib

import numpy as np
import pytest
import torch

import fs2_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, H, DK = 2, 2, 128
T_GRID = [1, 2, 63, 64, 65, 127, 128, 129, 257, 600]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _err(got, ref64):
    return float((got.double().cpu() - ref64).abs().max())


def _bound(cpu32, ref64):
    """4 x the fp32 CPU evaluation's error, scaled by max(1, |ref|max)"""
    e32 = float((cpu32.double() - ref64).abs().max())
    return e32, 4.0 * e32 * max(1.0, float(ref64.abs().max()))


def _masks(T):
    """None; item 1 valid for {1, T/2, T-1} keys (prefixes); a mask with holes"""
    out = [("none", None)]
    for n in sorted({1, T // 2, T - 1} - {0, T}):
        m = torch.ones(B, T, dtype=torch.bool)
        m[1, n:] = False
        out.append((f"prefix{n}", m))
    if T >= 3:
        m = torch.rand(B, T, generator=_gen("holes", T)) > 0.4
        m[:, T // 2] = True                      # at least one valid key per item
        m[0, 0] = False
        out.append(("holes", m))
    return out


def _attention_case(T, mask, qscale=1.0, fill=None):
    from amphion_amd.modules import hip_ops

    g = _gen("mh", T, qscale)
    C = H * DK
    qkv = torch.randn(B, 3 * C, T, generator=g)
    qkv[:, :C] *= qscale
    if fill is not None and mask is not None:        # masked K / V columns hold a large finite number
        bad = (~mask)[:, None, :].expand(B, 2 * C, T)
        qkv[:, C:][bad] = fill
    q64, k64, v64 = (t.double() for t in qkv.split(C, 1))
    if fill is not None and mask is not None:        # the references take zeros there
        bad = (~mask)[:, None, :].expand(B, C, T)
        k64, v64 = k64.masked_fill(bad, 0.0), v64.masked_fill(bad, 0.0)
    ref = R.mh_attention_cf(q64, k64, v64, H, mask)
    cpu = R.mh_attention_cf(q64.float(), k64.float(), v64.float(), H, mask)
    d = qkv.cuda()
    got = hip_ops.mh_attention(d[:, :C], d[:, C:2 * C], d[:, 2 * C:], H, None if mask is None else mask.cuda())
    return d, got, ref, cpu


@pytest.mark.parametrize("T", T_GRID)
def test_mh_attention_vs_fp64(T):
    """q | k | v are strided views of one [B, 3 H dk, T] tensor; masked K / V columns hold 1e30; at T = 1 the result is v's bits"""
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    fails = []
    for name, mask in _masks(T):
        d, got, ref, cpu = _attention_case(T, mask, fill=1e30)
        e32, bound = _bound(cpu, ref)
        e = _err(got, ref)
        print(f"mh_attention T={T} mask={name}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
        assert got.shape == (B, H * DK, T) and bool(torch.isfinite(got).all())
        if not e <= bound:
            fails.append((name, e, bound))
        if T == 1:
            assert torch.equal(got, d[:, 2 * H * DK:])
        _lib.range_check()                       # 1e30 in masked columns is not an operand
    assert not fails, fails


def test_mh_attention_moving_maximum():
    """q x 30: the running maximum moves from tile to tile and the rescale branch runs"""
    T = 257
    d, got, ref, cpu = _attention_case(T, _masks(T)[-1][1], qscale=30.0)
    e32, bound = _bound(cpu, ref)
    e = _err(got, ref)
    print(f"mh_attention q x 30 T={T}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert e <= bound


@pytest.mark.parametrize("T", [65, 257])
def test_mh_attention_item_alone_equals_item_in_batch(T):
    from amphion_amd.modules import hip_ops

    mask = _masks(T)[-1][1]
    d, got, _, _ = _attention_case(T, mask)
    C = H * DK
    for b in range(B):
        one = d[b:b + 1].contiguous()
        alone = hip_ops.mh_attention(one[:, :C], one[:, C:2 * C], one[:, 2 * C:], H, mask[b:b + 1].cuda())
        assert torch.equal(alone[0], got[b])


def test_mh_attention_f32_route_and_range_flag(conv_precision):
    """the exact-fp32 route (torch's SDPA) meets the same bound; the f16x3 kernel raises the op-level range flag for an operand of 1e5"""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    T = 129
    mask = _masks(T)[-1][1]
    d, got, ref, cpu = _attention_case(T, mask)
    e32, bound = _bound(cpu, ref)
    print(f"mh_attention {conv_precision} T={T}: gpu {_err(got, ref):.3e} bound {bound:.3e}")
    assert _err(got, ref) <= bound
    _lib.range_check()
    if conv_precision == "f16x3":
        C = H * DK
        big = d.clone()
        big[0, 2 * C + 3, 5] = 1e5               # a V operand of a valid key
        hip_ops.mh_attention(big[:, :C], big[:, C:2 * C], big[:, 2 * C:], H, None)
        with pytest.raises(_lib.AmpError) as e:
            _lib.range_check()
        assert e.value.status == _lib.AMP_ERR_RANGE
        _lib.range_check()                       # cleared


def test_dk128_is_still_refused_by_rope_attention():
    from amphion_amd.modules import hip_ops

    x = torch.zeros(1, 2 * 128, 8, device="cuda")
    cs = torch.zeros(8, 64, device="cuda")
    with pytest.raises(ValueError):
        hip_ops.rope_attention(x, x, x, 2, cs, cs)
    import ctypes

    from amphion_amd import _lib

    host = (ctypes.c_float * 16)()
    out = (ctypes.c_float * 16)()
    rc = _lib.lib().amp_rope_attention(host, host, host, 0, host, host, None, 1, 2, 128, 8, 0.1, out, None)
    assert rc == _lib.AMP_ERR_INVALID
    rc = _lib.lib().amp_mh_attention(host, host, host, 0, None, 1, 2, 64, 8, 0.1, out, None)
    assert rc == _lib.AMP_ERR_INVALID


# ---- amp_fs2_durations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_control", [1.0, 0.8, 1.25])
@pytest.mark.parametrize("T", [1, 5, 64, 65, 1000])
def test_fs2_durations(T, d_control):
    """inputs log(1 + n + delta), n in 0 .. 20, |delta| in [0.05, 0.45]: every rounding is decided by construction (asserted in fp64 first);
    a ragged batch of 3 whose padded tail is the masked 0; strongly negative inputs clamp to 0.  Equal to the torch fp32 ops on the CPU."""
    from amphion_amd.modules import hip_ops

    g = _gen("dur", T)
    Bn = 3
    n = torch.randint(0, 21, (Bn, T), generator=g).double()
    delta = (0.05 + 0.4 * torch.rand(Bn, T, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (Bn, T), generator=g) * 2 - 1)
    x64 = torch.log(1 + n + delta)
    if T >= 5:
        x64[0, 1], x64[2, 3] = -30.0, -4.0                # exp - 1 -> -1, rounds to -1, clamps to 0
    lens = [T, max(1, T // 2), max(1, T - 1)]
    for b, ln in enumerate(lens):
        x64[b, ln:] = 0.0
    frac = (torch.exp(x64) - 1) - torch.floor(torch.exp(x64) - 1)
    assert float((frac - 0.5).abs().min()) >= 0.04            # decided: fp32 cannot round the other way
    x = x64.float()
    ref_d = torch.clamp(torch.round(torch.exp(x) - 1) * d_control, min=0)
    ref64 = torch.clamp(torch.round(torch.exp(x64) - 1).float() * torch.tensor(d_control, dtype=torch.float32), min=0)
    assert torch.equal(ref_d, ref64)
    ref_n = ref_d.to(torch.int64)                              # int() truncation
    d, cum, mel_len = hip_ops.fs2_durations(x.cuda(), d_control)
    assert d.dtype == torch.float32 and cum.dtype == torch.int32 and mel_len.dtype == torch.int32
    assert torch.equal(d.cpu(), ref_d)                         # (-0 == 0)
    assert torch.equal(cum.cpu().long(), ref_n.cumsum(1))
    assert torch.equal(mel_len.cpu().long(), ref_n.sum(1))


# ---- amp_bucketize_embed_add -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("control", [1.0, 1.3])
@pytest.mark.parametrize("spacing", ["linear", "log"])
@pytest.mark.parametrize("n_bins", [2, 256])
@pytest.mark.parametrize("C,T", [(5, 1), (5, 33), (256, 33), (5, 257), (256, 257)])
def test_bucketize_embed_add(C, T, n_bins, spacing, control):
    """values exactly on boundaries, below the first, above the last, +-inf and NaN; every column is written; bit-equal to torch"""
    from amphion_amd.modules import hip_ops

    g = _gen("bucket", C, T, n_bins, spacing)
    Bn = 2
    if spacing == "linear":
        bins = torch.linspace(-2.5, 6.0, n_bins - 1)
    else:
        bins = torch.exp(torch.linspace(np.log(0.05), np.log(6.0), n_bins - 1))
    table = torch.randn(n_bins, C, generator=g)
    x = torch.randn(Bn, C, T, generator=g)
    pred = torch.rand(Bn, T, generator=g) * 10.0 - 3.0
    special = [float(bins[0]), float(bins[-1]), float(bins[len(bins) // 2]), -100.0, 100.0, float("inf"), float("-inf"), float("nan"), 0.0]
    for i, v in enumerate(special):
        if i < T:
            pred[i % Bn, (7 * i) % T] = v / control if control != 1.0 and np.isfinite(v) and i < 3 else v
    scaled_ref = pred * control
    idx = torch.bucketize(scaled_ref, bins)
    ref = x + table[idx].transpose(1, 2)
    y, scaled = hip_ops.bucketize_embed_add(x.cuda(), pred.cuda(), control, bins.cuda(), table.cuda())
    fin = ~scaled_ref.isnan()
    assert torch.equal(scaled.cpu().isnan(), ~fin) and torch.equal(scaled.cpu()[fin].view(torch.int32), scaled_ref[fin].view(torch.int32))
    assert torch.equal(y.cpu(), ref)
    xd = x.cuda()
    y2, _ = hip_ops.bucketize_embed_add(xd, pred.cuda(), control, bins.cuda(), table.cuda(), out=xd)      # in place
    assert y2 is xd and torch.equal(xd.cpu(), ref)


# ---- amp_layer_norm_c_head ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [5, 256, 384])
@pytest.mark.parametrize("T", [1, 31, 32, 33, 257])
def test_layer_norm_c_head(C, T):
    """ragged lens; masked columns exactly 0 whatever x holds there (NaN)"""
    from amphion_amd.modules import hip_ops

    g = _gen("lnhead", C, T)
    Bn = 3
    x = torch.randn(Bn, C, T, generator=g) * 2.0 + 0.5
    gamma, beta, w = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g) / C ** 0.5
    b0 = 0.37
    lens = torch.tensor([T, max(1, T // 2), max(1, T - 1)], dtype=torch.int32)
    pad = R.pad_mask(lens.long(), T)

    def f(x, gamma, beta, w):
        h = torch.nn.functional.layer_norm(x.transpose(1, 2), (C,), gamma, beta)
        return (torch.nn.functional.linear(h, w[None], torch.tensor([b0], dtype=x.dtype)).squeeze(-1)).masked_fill(pad, 0.0)

    ref = f(x.double(), gamma.double(), beta.double(), w.double())
    e32, bound = _bound(f(x, gamma, beta, w), ref)
    xn = x.clone()
    xn.transpose(1, 2)[pad] = float("nan")
    got = hip_ops.layer_norm_c_head(xn.cuda(), gamma.cuda(), beta.cuda(), w.cuda(), b0, lens.cuda())
    e = _err(got, ref)
    print(f"layer_norm_c_head C={C} T={T}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert got.shape == (Bn, T) and e <= bound
    assert bool((got.cpu()[pad] == 0).all())
    full = hip_ops.layer_norm_c_head(x.cuda(), gamma.cuda(), beta.cuda(), w.cuda(), b0, None)
    assert torch.equal(full.cpu()[~pad], got.cpu()[~pad])


# ---- modules and the model against the restatement ----------------------------------------------------------------------------------------
SEED = int(np.load(os.path.join(GOLDEN, "golden_fs2.npz"))["seed"])      # the seed the stored runs were decided under


@pytest.fixture(scope="module")
def hp():
    return R.small_hp()


@pytest.fixture(scope="module")
def sd(hp):
    return R.synth_state_dict(hp, SEED)


def _model(hp, sd):
    from amphion_amd.models.tts.fastspeech2 import FastSpeech2

    m = FastSpeech2(R.make_cfg(hp), stats=R.stats_of(hp), n_speaker=hp["n_speaker"] or None, n_src_vocab=hp["n_vocab"])
    m.load_state_dict(sd)
    return m.cuda().eval()


@pytest.mark.parametrize("T", [9, 65])
def test_fft_block_and_variance_predictor_modules(T, hp, sd, conv_precision):
    """a ragged batch through one FFT block and one VariancePredictor, batch-first as the reference takes them, against fp64"""
    m = _model(hp, sd)
    g = _gen("fft", T)
    x = torch.randn(2, T, hp["hidden"], generator=g)
    lens = torch.tensor([T, max(1, T // 2)])
    pad = R.pad_mask(lens, T)
    x = x.masked_fill(pad[:, :, None], 0)
    sd64, sd32 = R.cast(sd, torch.float64), R.cast(sd, torch.float32)
    pfx = "encoder.layer_stack.1"
    ref = R.fft_block(sd64, pfx, x.double(), pad, hp["heads"])
    e32, bound = _bound(R.fft_block(sd32, pfx, x, pad, hp["heads"]), ref)
    got, _ = m.encoder.layer_stack[1](x.cuda(), mask=pad.cuda(), slf_attn_mask=pad.cuda()[:, None, :].expand(-1, T, -1))
    e = _err(got, ref)
    print(f"FFTBlock {conv_precision} T={T}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert e <= bound and bool((got.cpu()[pad] == 0).all())
    pfx = "variance_adaptor.pitch_predictor"
    xin = x + 0.3                                        # padded rows are inputs of the convs
    ref = R.variance_predictor(sd64, pfx, xin.double(), pad)
    e32, bound = _bound(R.variance_predictor(sd32, pfx, xin, pad), ref)
    got = m.variance_adaptor.pitch_predictor(xin.cuda(), pad.cuda())
    e = _err(got, ref)
    print(f"VariancePredictor {conv_precision} T={T}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert e <= bound and bool((got.cpu()[pad] == 0).all())


RUNS = {
    "ragged": (dict(), [13, 9], (1.0, 1.0, 1.0)),
    "controls": (dict(), [13, 9], (1.2, 0.8, 1.25)),
    "long": (dict(max_seq_len=40), [45, 30], (1.0, 1.0, 1.0)),
    "frame_level": (dict(pitch_level="frame_level", energy_level="frame_level"), [13, 9], (1.0, 1.0, 1.0)),
    "multi_speaker": (dict(n_speaker=4), [13, 9], (1.0, 1.0, 1.0)),
}
CONT = ("output", "postnet_output", "p_predictions", "e_predictions", "log_d_predictions")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_fs2.npz"))


@pytest.fixture(scope="module")
def run_refs(gold):
    """per run: hyper-parameters, weights, the stored inputs, the fp64 and fp32 restatements -- computed once and shared"""
    out = {}
    for name, (over, text_len, controls) in RUNS.items():
        hp = R.small_hp(**over)
        sd = R.synth_state_dict(hp, SEED)
        texts, lens, spk = (torch.from_numpy(gold[f"{name}/{k}"]) for k in ("texts", "text_len", "spk_id"))
        assert tuple(gold[name + "/controls"]) == controls
        ok, tau, d_gap, b_gap, o64, o32 = R.decided(hp, sd, texts, lens, spk, controls)
        out[name] = (hp, sd, texts, lens, spk, controls, ok, o64, o32)
    return out


@pytest.mark.parametrize("name", list(RUNS))
def test_fastspeech2_forward(name, run_refs, gold, conv_precision):
    """every stored run of the real class.  Every decision of the run is at least 4 tau from its boundary (asserted: the margin rule), so
    d_rounded, mel_lens and the masks are compared for equality with the golden; the continuous outputs are within 4 x the fp32
    restatement's own distance from fp64 (x max(1, |ref|max)) of the golden, plus the golden's own distance from fp64"""
    hp, sd, texts, lens, spk, controls, ok, o64, o32 = run_refs[name]
    assert ok, "the run is not decided: pick another seed"
    G = lambda k: torch.from_numpy(gold[f"{name}/{k}"])
    m = _model(hp, sd)
    with torch.no_grad():
        got = m({"texts": texts.cuda(), "text_len": lens.cuda(), "spk_id": spk.cuda()}, *controls)
    assert torch.equal(got["d_rounded"].cpu(), G("d_rounded"))
    assert torch.equal(got["mel_lens"].cpu(), G("mel_lens")) and torch.equal(got["src_lens"].cpu(), lens)
    assert torch.equal(got["mel_masks"].cpu(), G("mel_masks")) and torch.equal(got["src_masks"].cpu(), G("src_masks"))
    fails = []
    for k in CONT:
        e32, bound = _bound(o32[k], o64[k])
        own = float((G(k).double() - o64[k]).abs().max())
        bound += own
        e = float((got[k].cpu() - G(k)).abs().max())
        print(f"FastSpeech2 {name} {conv_precision} {k}: gpu vs golden {e:.3e} cpu32 {e32:.3e} golden's own {own:.3e} bound {bound:.3e} "
              f"shape {tuple(got[k].shape)}")
        if got[k].shape != o64[k].shape or not e <= bound:
            fails.append((k, e, bound))
    assert not fails, fails


def test_fastspeech2_teacher_forced(run_refs):
    """the restatement's durations fed in: the length regulator, decoder, mel_linear and PostNet independently of the decisions"""
    hp, sd, texts, lens, spk, controls, ok, o64, o32 = run_refs["ragged"]
    m = _model(hp, sd)
    with torch.no_grad():
        got = m({"texts": texts.cuda(), "text_len": lens.cuda(), "spk_id": spk.cuda()}, durations=o64["d_rounded"].float().cuda())
    for k in ("output", "postnet_output"):
        e32, bound = _bound(o32[k], o64[k])
        assert _err(got[k], o64[k]) <= bound, k


def test_fastspeech2_refusals(run_refs):
    hp, sd, texts, lens, spk, *_ = run_refs["ragged"]
    m = _model(hp, sd)
    data = {"texts": texts.cuda(), "text_len": lens.cuda(), "spk_id": spk.cuda()}
    with pytest.raises(NotImplementedError):
        m(dict(data, durations=torch.ones_like(texts).cuda()))
    with pytest.raises(NotImplementedError):
        m(dict(data, pitch=torch.zeros(2, 13).cuda()))
    m.train()
    with pytest.raises(NotImplementedError):
        m(data)
    m.eval()
    z = torch.zeros(2, 13)
    z[0, :] = 2.0                                        # item 1 expands to no frame
    with pytest.raises(ValueError, match="zero frames"):
        m(data, durations=z.cuda())


# ---- JETS -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jets_refs(gold):
    hp = R.small_hp()
    sd = R.jets_state_dict(hp, SEED)
    texts, lens = torch.from_numpy(gold["jets/texts"]), torch.from_numpy(gold["jets/text_len"])
    ok, tau, gap, o64, o32 = R.jets_decided(hp, sd, texts, lens)
    return hp, sd, texts, lens, ok, o64, o32


def test_jets_inference(jets_refs, gold, conv_precision):
    """the stored run of the real class: d_predictions equal (the run is decided: asserted), the wave within 4 x the fp32 restatement's own
    distance from fp64 (x max(1, |ref|max)) of the golden, plus the golden's own distance from fp64"""
    from amphion_amd.models.tts.jets import Jets

    hp, sd, texts, lens, ok, o64, o32 = jets_refs
    assert ok, "the run is not decided: pick another seed"
    m = Jets(R.make_cfg(hp), stats=R.stats_of(hp), n_src_vocab=hp["n_vocab"])
    m.load_state_dict(sd)
    m = m.cuda().eval()
    with torch.no_grad():
        wav, d = m.inference({"texts": texts.cuda(), "text_len": lens.cuda(), "spk_id": torch.zeros(2, dtype=torch.long).cuda()})
    assert d.dtype == torch.int64 and torch.equal(d.cpu(), torch.from_numpy(gold["jets/d_predictions"]))
    g = torch.from_numpy(gold["jets/wav"])
    e32, bound = _bound(o32["wav"], o64["wav"])
    own = float((g.double() - o64["wav"]).abs().max())
    e = float((wav.cpu() - g).abs().max())
    print(f"Jets {conv_precision} wav {tuple(wav.shape)}: gpu vs golden {e:.3e} cpu32 {e32:.3e} golden's own {own:.3e} bound {bound + own:.3e}")
    assert wav.shape == g.shape and e <= bound + own
    with pytest.raises(NotImplementedError):
        m({"texts": texts.cuda(), "text_len": lens.cuda()})
