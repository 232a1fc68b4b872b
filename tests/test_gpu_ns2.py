"""NaturalSpeech2 inference on the GPU, op by op against the fp64 restatement (tests/ns2_ref.py): amp_cross_attention (head dimension 64, no
rotation, query and key lengths apart), the WaveNet residual layer amp_ns2_layer_* at hidden 512 and 128, amp_ns2_ode_step; then the encoder
layer, the two predictors and the WaveNet as modules, and the three runs stored from the real reference class (tests/golden/make_golden_ns2.py).
Bounds: 4 x the fp32 CPU evaluation's own distance from fp64, scaled by max(1, |ref|max) -- the rule of test_gpu_fmt.py / test_gpu_fs2.py;
what is specified bit for bit (the Tk = 1 copy, an item alone against the item in its batch, in place against out of place) is compared
for equality."""
import zlib

import pytest
import torch

import ns2_ref as R

pytestmark = pytest.mark.gpu

B, H, DK = 2, 2, 64
C = H * DK
PAIRS = [(1, 1), (1, 65), (2, 32), (127, 8), (128, 32), (129, 63), (129, 64), (300, 65), (65, 257), (257, 257)]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _err(got, ref64):
    return float((got.double().cpu() - ref64).abs().max())


def _bound(cpu32, ref64):
    """4 x the fp32 CPU evaluation's error, scaled by max(1, |ref|max)"""
    e32 = float((cpu32.double() - ref64).abs().max())
    return e32, 4.0 * e32 * max(1.0, float(ref64.abs().max()))


# ---- amp_cross_attention ----------------------------------------------------------------------------------------------------------------
def _masks(Tk):
    """None; item 1 valid for {1, Tk/2, Tk-1} keys (prefixes); a mask with holes"""
    out = [("none", None)]
    for n in sorted({1, Tk // 2, Tk - 1} - {0, Tk}):
        m = torch.ones(B, Tk, dtype=torch.bool)
        m[1, n:] = False
        out.append((f"prefix{n}", m))
    if Tk >= 3:
        m = torch.rand(B, Tk, generator=_gen("holes", Tk)) > 0.4
        m[:, Tk // 2] = True                     # at least one valid key per item
        m[0, 0] = False
        out.append(("holes", m))
    return out


def _attention_case(Tq, Tk, mask, qscale=1.0, fill=None):
    """q is a row block of a [B, C + 32, Tq] tensor, k | v the two row blocks of one stacked [B, 2C, Tk] tensor: the q batch stride differs
    from the kv batch stride and neither is dense"""
    from amphion_amd.modules import hip_ops

    g = _gen("cross", Tq, Tk, qscale)
    qw = torch.randn(B, C + 32, Tq, generator=g)
    qw[:, :C] *= qscale
    kv = torch.randn(B, 2 * C, Tk, generator=g)
    if fill is not None and mask is not None:        # masked K / V columns hold a large finite number
        kv[(~mask)[:, None, :].expand(B, 2 * C, Tk)] = fill
    q64, k64, v64 = qw[:, :C].double(), kv[:, :C].double(), kv[:, C:].double()
    if fill is not None and mask is not None:        # the references take zeros there
        bad = (~mask)[:, None, :].expand(B, C, Tk)
        k64, v64 = k64.masked_fill(bad, 0.0), v64.masked_fill(bad, 0.0)
    ref = R.cross_attention_cf(q64, k64, v64, H, mask)
    cpu = R.cross_attention_cf(q64.float(), k64.float(), v64.float(), H, mask)
    dq, dkv = qw.cuda(), kv.cuda()
    got = hip_ops.cross_attention(dq[:, :C], dkv[:, :C], dkv[:, C:], H, None if mask is None else mask.cuda())
    return dq, dkv, got, ref, cpu


@pytest.mark.parametrize("Tq,Tk", PAIRS)
def test_cross_attention_vs_fp64(Tq, Tk):
    """every mask; masked K / V columns hold 1e30; at Tk = 1 the result is v's column, bit for bit, at every query"""
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    fails = []
    for name, mask in _masks(Tk):
        dq, dkv, got, ref, cpu = _attention_case(Tq, Tk, mask, fill=1e30)
        e32, bound = _bound(cpu, ref)
        e = _err(got, ref)
        print(f"cross_attention Tq={Tq} Tk={Tk} mask={name}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
        assert got.shape == (B, C, Tq) and bool(torch.isfinite(got).all())
        if not e <= bound:
            fails.append((name, e, bound))
        if Tk == 1:
            assert torch.equal(got, dkv[:, C:].expand(B, C, Tq))
        _lib.range_check()                       # 1e30 in masked columns is not an operand
    assert not fails, fails


def test_cross_attention_moving_maximum():
    """q x 30: the running maximum moves from tile to tile and the rescale branch runs"""
    Tq, Tk = 129, 257
    _, _, got, ref, cpu = _attention_case(Tq, Tk, _masks(Tk)[-1][1], qscale=30.0)
    e32, bound = _bound(cpu, ref)
    e = _err(got, ref)
    print(f"cross_attention q x 30 Tq={Tq} Tk={Tk}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert e <= bound


@pytest.mark.parametrize("Tq,Tk", [(129, 63), (65, 257)])
def test_cross_attention_item_alone_equals_item_in_batch(Tq, Tk):
    from amphion_amd.modules import hip_ops

    mask = _masks(Tk)[-1][1]
    dq, dkv, got, _, _ = _attention_case(Tq, Tk, mask)
    for b in range(B):
        q1, kv1 = dq[b:b + 1, :C].contiguous(), dkv[b:b + 1].contiguous()
        alone = hip_ops.cross_attention(q1, kv1[:, :C], kv1[:, C:], H, mask[b:b + 1].cuda())
        assert torch.equal(alone[0], got[b])


def test_cross_attention_self_attention_on_a_stacked_tensor():
    """Tq = Tk with q | k | v the three row blocks of one tensor, read in place"""
    from amphion_amd.modules import hip_ops

    T = 129
    qkv = torch.randn(B, 3 * C, T, generator=_gen("self", T))
    mask = _masks(T)[-1][1]
    q64, k64, v64 = (t.double() for t in qkv.split(C, 1))
    ref = R.cross_attention_cf(q64, k64, v64, H, mask)
    e32, bound = _bound(R.cross_attention_cf(q64.float(), k64.float(), v64.float(), H, mask), ref)
    d = qkv.cuda()
    got = hip_ops.cross_attention(d[:, :C], d[:, C:2 * C], d[:, 2 * C:], H, mask.cuda())
    print(f"cross_attention self T={T}: gpu {_err(got, ref):.3e} bound {bound:.3e}")
    assert _err(got, ref) <= bound


def test_cross_attention_f32_route_and_range_flag(conv_precision):
    """the exact-fp32 route (torch's SDPA) meets the same bound; the f16x3 kernel raises the op-level range flag for a V operand of 1e5"""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    Tq, Tk = 129, 64
    mask = _masks(Tk)[-1][1]
    dq, dkv, got, ref, cpu = _attention_case(Tq, Tk, mask)
    e32, bound = _bound(cpu, ref)
    print(f"cross_attention {conv_precision} Tq={Tq} Tk={Tk}: gpu {_err(got, ref):.3e} bound {bound:.3e}")
    assert _err(got, ref) <= bound
    _lib.range_check()
    if conv_precision == "f16x3":
        big = dkv.clone()
        big[0, C + 3, 5] = 1e5                   # a V operand of a valid key
        hip_ops.cross_attention(dq[:, :C], big[:, :C], big[:, C:], H, None)
        with pytest.raises(_lib.AmpError) as e:
            _lib.range_check()
        assert e.value.status == _lib.AMP_ERR_RANGE
        _lib.range_check()                       # cleared


def test_cross_attention_refuses_other_head_dimensions():
    import ctypes

    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    for dk in (32, 96, 128):
        x = torch.zeros(1, 2 * dk, 8, device="cuda")
        with pytest.raises(ValueError):
            hip_ops.cross_attention(x, x, x, 2)
        host = (ctypes.c_float * 16)()
        out = (ctypes.c_float * 16)()
        rc = _lib.lib().amp_cross_attention(host, 0, host, host, 0, None, 1, 2, dk, 8, 8, 0.1, out, None)
        assert rc == _lib.AMP_ERR_INVALID


# ---- the WaveNet residual layer -----------------------------------------------------------------------------------------------------------
LAYER_T = [1, 2, 63, 64, 65, 129, 257]
DILATIONS = [1, 2, 8]


def _layer_weights(Hd):
    """one set per hidden size: conv rows of unit output variance, out_proj likewise"""
    g = _gen("layer weights", Hd)
    cw = torch.randn(2 * Hd, Hd, 3, generator=g) / (1.5 * (3 * Hd) ** 0.5)
    cb = torch.randn(2 * Hd, generator=g) * 0.1
    ow = torch.randn(2 * Hd, Hd, 1, generator=g) / Hd ** 0.5
    ob = torch.randn(2 * Hd, generator=g) * 0.1
    return cw, cb, ow, ob


_WEIGHTS = {}


def _weights(Hd):
    if Hd not in _WEIGHTS:
        w = _layer_weights(Hd)
        _WEIGHTS[Hd] = (w, tuple(t.cuda() for t in w))
    return _WEIGHTS[Hd]


def _layer_inputs(Hd, T, Bn=B):
    g = _gen("layer inputs", Hd, T, Bn)
    x = torch.randn(Bn, Hd, T, generator=g)
    dconst = torch.randn(Bn, Hd, generator=g) * 0.5
    cterm_all = torch.randn(Bn, 3 * 2 * Hd, T, generator=g) * 0.5      # three layers' stacked cterm: the middle row block is the layer's
    film = torch.cat((1.0 + 0.3 * torch.randn(Bn, 2 * Hd, T, generator=g), 0.3 * torch.randn(Bn, 2 * Hd, T, generator=g)), 1)
    skip = torch.randn(Bn, Hd, T, generator=g)
    return x, dconst, cterm_all, film, skip


def _combos():
    """(film, skip_in, dconst per item): FiLM x skip_in, each dconst form with two of them"""
    return [(f, s, f == s) for f in (False, True) for s in (False, True)]


def _run_layer(op, dev, x, dconst, cterm_all, film, skip, use_film, use_skip, per_item, Hd):
    cw, cb, ow, ob = dev
    sk = skip.cuda().clone() if use_skip else None
    xo, so = op(x.cuda(), dconst.cuda() if per_item else dconst[0].cuda(), cterm_all.cuda()[:, 2 * Hd:4 * Hd], cw, cb, ow, ob,
                film=film.cuda() if use_film else None, skip=sk)
    return xo, so


@pytest.mark.parametrize("T", LAYER_T)
@pytest.mark.parametrize("Hd", [512, 128])
def test_ns2_layer_vs_fp64(Hd, T, conv_precision):
    """dilations 1, 2, 8; with and without FiLM and skip_in; dconst shared and per item; cterm a row block of a stacked tensor.  At
    T <= 2 d the taps outside [0, T) contribute 0 although dconst != 0: the wrong form that pads x misses the same bound (checked on the
    CPU), so the bound can tell the two apart.  Both arithmetics meet the bound."""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    (cw, cb, ow, ob), dev = _weights(Hd)
    x, dconst, cterm_all, film, skip = _layer_inputs(Hd, T)
    cterm = cterm_all[:, 2 * Hd:4 * Hd]
    fails = []
    for d in DILATIONS:
        op = hip_ops.Ns2Layer(Hd, d)
        for per_item in (False, True):
            dc = dconst if per_item else dconst[:1]
            a64 = R.layer_conv(x.double(), dc.double(), cw.double(), cb.double(), d)
            a32 = R.layer_conv(x, dc, cw, cb, d)
            bad64 = R.layer_conv(x.double(), dc.double(), cw.double(), cb.double(), d, pad_x=True) if T <= 2 * d else a64
            for use_film, use_skip, pi in _combos():
                if pi != per_item:
                    continue
                f, s = (film if use_film else None), (skip if use_skip else None)
                ref = R.layer_tail(x.double(), a64, cterm.double(), ow.double(), ob.double(), None if f is None else f.double(), None if s is None else s.double())
                cpu = R.layer_tail(x, a32, cterm, ow, ob, f, s)
                bad = R.layer_tail(x.double(), bad64, cterm.double(), ow.double(), ob.double(), None if f is None else f.double(), None if s is None else s.double())
                got = _run_layer(op, dev, x, dconst, cterm_all, film, skip, use_film, use_skip, per_item, Hd)
                for name, gg, rr, cc, bb in zip(("x_out", "skip_out"), got, ref, cpu, bad):
                    e32, bound = _bound(cc, rr)
                    e = _err(gg, rr)
                    print(f"ns2 layer {conv_precision} H={Hd} T={T} d={d} film={int(use_film)} skip={int(use_skip)} per_item={int(per_item)} {name}: "
                          f"gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
                    if not e <= bound:
                        fails.append((d, use_film, use_skip, per_item, name, e, bound))
                    if T <= 2 * d:
                        assert float((bb - rr).abs().max()) > bound, "the bound cannot tell padding x from padding y"
        _lib.range_check()
    assert not fails, fails


@pytest.mark.parametrize("Hd,T,d", [(512, 129, 2), (128, 65, 8)])
def test_ns2_layer_item_alone_equals_item_in_batch_and_in_place(Hd, T, d):
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    _lib.set_precision("f16x3")
    _, dev = _weights(Hd)
    cw, cb, ow, ob = dev
    x, dconst, cterm_all, film, skip = _layer_inputs(Hd, T)
    op = hip_ops.Ns2Layer(Hd, d)
    xo, so = _run_layer(op, dev, x, dconst, cterm_all, film, skip, True, True, True, Hd)
    for b in range(B):
        xa, sa = op(x[b:b + 1].cuda(), dconst[b:b + 1].cuda(), cterm_all[b:b + 1, 2 * Hd:4 * Hd].cuda(), cw, cb, ow, ob, film=film[b:b + 1].cuda(),
                    skip=skip[b:b + 1].cuda())
        assert torch.equal(xa[0], xo[b]) and torch.equal(sa[0], so[b])
    # x_out = x (in place) and a second call of the same launch: the same bits
    xd = x.cuda()
    xi, si = op(xd, dconst.cuda(), cterm_all.cuda()[:, 2 * Hd:4 * Hd], cw, cb, ow, ob, film=film.cuda(), skip=skip.cuda(), x_out=xd)
    assert xi is xd and torch.equal(xi, xo) and torch.equal(si, so)


def test_ns2_layer_range_flag_and_refusals():
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    _lib.set_precision("f16x3")
    Hd, T = 128, 65
    _, dev = _weights(Hd)
    x, dconst, cterm_all, film, skip = _layer_inputs(Hd, T)
    op = hip_ops.Ns2Layer(Hd, 1)
    _run_layer(op, dev, x, dconst, cterm_all, film, skip, False, False, True, Hd)
    _lib.range_check()
    big = x.clone()
    big[1, 7, 33] = 1e5
    _run_layer(op, dev, big, dconst, cterm_all, film, skip, False, False, True, Hd)
    with pytest.raises(_lib.AmpError) as e:
        _lib.range_check()
    assert e.value.status == _lib.AMP_ERR_RANGE
    _lib.range_check()                           # cleared
    for Hbad, dbad in ((128, 9), (96, 1), (576, 1), (128, 0)):
        w = [t.cuda() for t in _layer_weights(Hbad)]
        with pytest.raises(_lib.AmpError) as e:
            hip_ops.Ns2Layer(Hbad, dbad)(torch.zeros(1, Hbad, 8, device="cuda"), torch.zeros(Hbad, device="cuda"),
                                         torch.zeros(1, 2 * Hbad, 8, device="cuda"), *w)
        assert e.value.status == _lib.AMP_ERR_UNSUPPORTED


# ---- amp_ns2_ode_step ---------------------------------------------------------------------------------------------------------------------
def _ode_scalars(t, h, beta_min=0.05, beta_max=20.0, sigma=1.0):
    """the step's scalars formed as the model code forms them: fp32 torch on a one-element tensor"""
    ts = torch.tensor([t], dtype=torch.float32)
    cum_beta = beta_min * ts + 0.5 * (beta_max - beta_min) * (ts ** 2)
    beta_t = beta_min + (beta_max - beta_min) * ts
    e = torch.exp(-0.5 * cum_beta / (sigma ** 2))
    var = (sigma ** 2) * (1.0 - torch.exp(-cum_beta / (sigma ** 2)))
    return float(e), float(var), float(h * beta_t), float(torch.tensor(1.0 / sigma ** 2, dtype=torch.float32))


@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 32, 130)])
@pytest.mark.parametrize("mid", [False, True])
def test_ns2_ode_step(shape, mid):
    from amphion_amd.modules import hip_ops

    g = _gen("ode", shape)
    xe, x0, xb = (torch.randn(*shape, generator=g) for _ in range(3))
    for t in (0.875, 0.125):
        sc = _ode_scalars(t, 0.25)
        ref = R.ode_step(xe.double(), x0.double(), xb.double(), *sc, mid=mid)
        e32, bound = _bound(R.ode_step(xe, x0, xb, *sc, mid=mid), ref)
        got = hip_ops.ns2_ode_step(xe.cuda(), x0.cuda(), xb.cuda(), *sc, midpoint_half=mid)
        print(f"ns2_ode_step {shape} t={t} mid={mid}: gpu {_err(got, ref):.3e} cpu32 {e32:.3e} bound {bound:.3e}")
        assert _err(got, ref) <= bound
        # in place on x_base (euler: x_eval = x_base = xt) and on a base that is not 16-byte aligned: the same bits
        xt = xe.cuda()
        euler = hip_ops.ns2_ode_step(xt, x0.cuda(), xt, *sc, midpoint_half=mid)
        buf = torch.empty(xe.numel() + 1, device="cuda")
        xt2 = buf[1:].view(shape).copy_(xe)
        inplace = hip_ops.ns2_ode_step(xt2, x0.cuda(), xt2, *sc, midpoint_half=mid, out=xt2)
        assert inplace is xt2 and torch.equal(inplace, euler)


# ---- the modules at the small model's sizes ---------------------------------------------------------------------------------------------
import os  # noqa: E402

import numpy as np  # noqa: E402
import torch.nn.functional as F  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = int(np.load(os.path.join(GOLDEN, "golden_ns2.npz"))["seed"])      # the seed the stored runs were decided under
RUNS = {"euler": (dict(), 4), "midpoint": (dict(solver="midpoint"), 3), "flow": (dict(diffusion_type="flow"), 4)}
CONT = ("prior_out", "dur_pred_log", "dur_pred", "pitch_pred_log")
DISCRETE = ("dur_pred_round", "mel_len", "pitch_token")


@pytest.fixture(scope="module")
def hp():
    return R.small_hp()


@pytest.fixture(scope="module")
def sd(hp):
    return R.synth_state_dict(hp, SEED)


def _sub(sd, prefix):
    return {k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}


def _check(name, got, ref64, cpu32):
    e32, bound = _bound(cpu32, ref64)
    e = _err(got, ref64)
    print(f"{name}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert tuple(got.shape) == tuple(ref64.shape) and e <= bound, (name, e, bound)


@pytest.mark.parametrize("T", [9, 65])
@pytest.mark.parametrize("cln", [False, True])
def test_transformer_encoder_layer(cln, T, hp, sd, conv_precision):
    """one TransformerEncoderLayer with a ragged key mask; with the style-adaptive norm the condition is a prompt of 37 frames"""
    from amphion_amd.modules.naturalpseech2.transformers import TransformerEncoderLayer

    C = hp["hidden"]
    p = ("prior_encoder.encoder" if cln else "prompt_encoder") + ".layers.1"
    m = TransformerEncoderLayer(C, hp["heads"], hp["d_inner"], hp["kernel"], 0.2, cln)
    m.load_state_dict(_sub(sd, p))
    m = m.cuda().eval()
    g = _gen("encoder layer", cln, T)
    x = torch.randn(B, T, C, generator=g)
    cond = torch.randn(B, 37, C, generator=g)
    valid = torch.arange(T)[None, :] < torch.tensor([T, max(1, T // 2)])[:, None]

    def ref(dt):
        s = R.cast(sd, dt)
        if cln:
            mean = cond.to(dt).mean(1, keepdim=True)
            style = lambda name: (lambda st: (st[..., :C], st[..., C:]))(F.linear(mean, s[name + ".style.weight"], s[name + ".style.bias"]))
        else:
            style = lambda name: None
        return R.encoder_layer(s, p, x.to(dt), hp["heads"], valid, style)

    got = m(x.cuda(), valid.float().cuda(), cond.cuda() if cln else None)
    _check(f"encoder layer cln={cln} T={T} {conv_precision}", got, ref(torch.float64), ref(torch.float32))


@pytest.mark.parametrize("which", ["duration_predictor", "pitch_predictor"])
def test_predictors(which, hp, sd, conv_precision):
    from amphion_amd.modules.naturalpseech2 import transformers as Tm

    C, N, Tr = hp["hidden"], 23, 37
    p = "prior_encoder." + which
    cfg = R.make_cfg(hp).prior_encoder[which]
    m = (Tm.DurationPredictor if which == "duration_predictor" else Tm.PitchPredictor)(cfg)
    m.load_state_dict(_sub(sd, p))
    m = m.cuda().eval()
    g = _gen(which)
    x = torch.randn(B, N, C, generator=g)
    ref_emb = torch.randn(B, Tr, C, generator=g)
    valid = torch.arange(Tr)[None, :] < torch.tensor([Tr, 23])[:, None]
    r64 = R.predictor(R.cast(sd, torch.float64), p, hp, x.double(), ref_emb.double(), valid)
    r32 = R.predictor(sd, p, hp, x, ref_emb, valid)
    out = m(x.cuda(), None, ref_emb.transpose(1, 2).contiguous().cuda(), valid.float().cuda())
    if which == "duration_predictor":
        assert set(out) == {"dur_pred_log", "dur_pred", "dur_pred_round"} and out["dur_pred_round"].dtype == torch.int64
        out = out["dur_pred_log"]
    _check(f"{which} {conv_precision}", out, r64, r32)


@pytest.mark.parametrize("T", [9, 130])
def test_wavenet_forward(T, hp, sd, conv_precision):
    """WaveNet.forward at one step time: prepare (the stacked once-per-utterance GEMMs) and one step"""
    from amphion_amd import _lib
    from amphion_amd.models.tts.naturalspeech2.wavenet import WaveNet

    C = hp["hidden"]
    w = "diffusion.diff_estimator"
    m = WaveNet(R.make_cfg(hp).diffusion.wavenet)
    m.load_state_dict(_sub(sd, w))
    m = m.cuda().eval()
    g = _gen("wavenet", T)
    x = torch.randn(B, hp["latent"], T, generator=g)
    cond = torch.randn(B, T, C, generator=g)
    spk = torch.randn(B, hp["n_query"], C, generator=g)
    t = torch.full((B,), 0.625)
    r64 = R.wavenet(R.cast(sd, torch.float64), hp, x.double(), cond.double(), t.double(), spk.double())
    r32 = R.wavenet(sd, hp, x, cond, t, spk)
    got = m(x.cuda(), None, cond.cuda(), t.cuda(), spk.cuda())
    _check(f"WaveNet T={T} {conv_precision}", got, r64, r32)
    _lib.range_check()


# ---- the stored runs ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_ns2.npz"))


@pytest.fixture(scope="module")
def run_refs(gold):
    """every stored run in fp64 and in fp32 on the CPU, once"""
    out = {}
    for name, (over, n) in RUNS.items():
        h = R.small_hp(**over)
        s = R.synth_state_dict(h, SEED)
        t = lambda k: torch.from_numpy(gold[f"{name}/{k}"])
        codes, phone, mask, z = t("ref_code"), t("phone_id"), t("ref_mask"), t("z")
        x64, p64 = R.inference(R.cast(s, torch.float64), h, codes.transpose(0, 1), phone, mask, z.double(), n)
        x32, p32 = R.inference(s, h, codes.transpose(0, 1), phone, mask, z, n)
        p64["x0"], p32["x0"] = x64, x32
        out[name] = (h, s, codes, phone, mask, z, n, p64, p32)
    return out


@pytest.mark.parametrize("name", list(RUNS))
def test_naturalspeech2_inference(name, run_refs, gold, conv_precision):
    """x0 and the continuous entries of prior_out against the real class's stored output within the bound plus the golden's own distance from
    fp64; durations, frame counts and pitch tokens equal; the weights load strictly from the regenerated state dict; the noise is the
    golden's draw, replayed through ``noise=``"""
    from amphion_amd.models.tts.naturalspeech2 import NaturalSpeech2

    h, s, codes, phone, mask, z, n, p64, p32 = run_refs[name]
    m = NaturalSpeech2(R.make_cfg(h))
    m.load_state_dict(s, strict=True)
    m = m.cuda().eval()
    x0, po = m.inference(ref_code=codes.cuda(), phone_id=phone.cuda(), ref_mask=mask.cuda(), inference_steps=n, noise=lambda shape: z.reshape(shape))
    po = dict(po, x0=x0)
    for k in DISCRETE:
        assert torch.equal(po[k].cpu(), torch.from_numpy(gold[f"{name}/{k}"])), k
    fails = []
    for k in ("x0",) + CONT:
        g = torch.from_numpy(gold[f"{name}/{k}"])
        e_g = float((g.double() - p64[k]).abs().max())
        e32, bound = _bound(p32[k], p64[k])
        e = float((po[k].cpu().double() - g.double()).abs().max())
        print(f"{name} {conv_precision} {k}: gpu vs golden {e:.3e}, bound {bound:.3e} + golden vs fp64 {e_g:.3e}")
        assert tuple(po[k].shape) == tuple(g.shape)
        if not e <= bound + e_g:
            fails.append((k, e, bound + e_g))
    assert not fails, fails


def test_code_to_latent_and_prompt_latent_entry(run_refs, gold):
    """code_to_latent equals torch's sum of look-ups; ``ref_latent=`` in place of ``ref_code`` gives the same bits"""
    from amphion_amd.models.tts.naturalspeech2 import NaturalSpeech2

    h, s, codes, phone, mask, z, n, p64, p32 = run_refs["euler"]
    m = NaturalSpeech2(R.make_cfg(h))
    m.load_state_dict(s, strict=True)
    m = m.cuda().eval()
    lat = m.code_to_latent(codes.cuda())
    assert torch.equal(lat.cpu(), R.code_to_latent(s, h, codes.transpose(0, 1)))
    noise = lambda shape: z.reshape(shape)
    a, _ = m.inference(ref_code=codes.cuda(), phone_id=phone.cuda(), ref_mask=mask.cuda(), inference_steps=2, noise=noise)
    b, _ = m.inference(ref_latent=lat, phone_id=phone.cuda(), ref_mask=mask.cuda(), inference_steps=2, noise=noise)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        m.inference(ref_code=codes.cuda(), ref_latent=lat, phone_id=phone.cuda(), ref_mask=mask.cuda())
