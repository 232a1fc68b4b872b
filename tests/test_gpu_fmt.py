"""Vevo's flow-matching transformer on the GPU, through module -> ctypes -> C ABI: the four kernels of csrc/llama_nar.hip op by op, then
``DiffLlama.forward`` and ``FlowMatchingTransformer.reverse_diffusion`` against the golden outputs of the real reference classes
(tests/golden/make_golden_fmt.py) and against the fp64 restatement (tests/fmt_ref.py).

Bounds.  Ops: 4 x the error of THE SAME FORMULA evaluated by torch in fp32 on the CPU on the same inputs, scaled by max(1, |ref|max) (the
VITS-ops rule): room for another summation order, while a wrong operand, rotation or mask is orders above it.  Models:
the fp32 CPU restatement's distance from fp64 at these very shapes is measured here and the GPU is allowed 4 x that (DESIGN.md section 20
records the figures); against the golden -- itself an fp32 evaluation that far from fp64 -- the GPU is allowed its own bound plus the golden's
distance (the triangle inequality).  Every test prints its figures before it asserts."""
import os
import zlib

import numpy as np
import pytest
import torch

import fmt_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, H, DK = 2, 2, 64
T_GRID = [1, 2, 63, 64, 65, 127, 129, 257, 600]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _err(got, ref64):
    return float((got.double().cpu() - ref64).abs().max())


def _bound(cpu32, ref64, what):
    """4 x the fp32 CPU evaluation's error, scaled by max(1, |ref|max)"""
    e32 = float((cpu32.double() - ref64).abs().max())
    b = 4.0 * e32 * max(1.0, float(ref64.abs().max()))
    return e32, b


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

    g = _gen("attn", T, qscale)
    qkv = torch.randn(B, 3 * H * DK, T, generator=g)
    qkv[:, : H * DK] *= qscale
    if fill is not None and mask is not None:        # masked K / V columns hold a large finite number
        bad = (~mask)[:, None, :].expand(B, 2 * H * DK, T)
        qkv[:, H * DK:][bad] = fill
    C = H * DK
    cos, sin = R.rope_cos_sin(T, DK)
    q64, k64, v64 = (t.double() for t in qkv.split(C, 1))
    if fill is not None and mask is not None:        # the references take zeros there: 0 * 1e30 is the kernel's business, not theirs
        bad = (~mask)[:, None, :].expand(B, C, T)
        k64, v64 = k64.masked_fill(bad, 0.0), v64.masked_fill(bad, 0.0)
    ref = R.rope_attention_cf(q64, k64, v64, H, cos.double(), sin.double(), mask)
    cpu = R.rope_attention_cf(q64.float(), k64.float(), v64.float(), H, cos, sin, mask)
    d = qkv.cuda()
    got = hip_ops.rope_attention(d[:, :C], d[:, C:2 * C], d[:, 2 * C:], H, cos.cuda(), sin.cuda(), None if mask is None else mask.cuda())
    return d, got, ref, cpu


@pytest.mark.parametrize("T", T_GRID)
def test_rope_attention_vs_fp64(T):
    """q | k | v are strided views of one [B, 3 H dk, T] tensor; masked K / V columns hold 1e30.

    Measured on the MI355X: T = 2 ... 600 at 2.7e-7 - 1.3e-6 against bounds of 1.2e-6 - 8.0e-6.  At T = 1 the softmax over the one key is
    exactly 1, torch's fp32 result is v itself and the bound is 0: the entry point returns v's bits there (a copy; the split-f16 operand of
    the kernel would hold 22 of the 24 mantissa bits, 2.4e-7 on |v| <= 4)."""
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    fails = []
    for name, mask in _masks(T):
        d, got, ref, cpu = _attention_case(T, mask, fill=1e30)
        e32, bound = _bound(cpu, ref, name)
        e = _err(got, ref)
        print(f"rope_attention T={T} mask={name}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
        assert got.shape == (B, H * DK, T) and bool(torch.isfinite(got).all())
        if not e <= bound:
            fails.append((name, e, bound))
        _lib.range_check()                       # 1e30 in masked columns is not an operand
    assert not fails, fails


def test_rope_attention_moving_maximum():
    """q x 30: scores of magnitude ~ 30 sigma, the running maximum moves from tile to tile and the rescale branch runs"""
    T = 257
    d, got, ref, cpu = _attention_case(T, _masks(T)[-1][1], qscale=30.0)
    e32, bound = _bound(cpu, ref, "x30")
    e = _err(got, ref)
    print(f"rope_attention q x 30 T={T}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert e <= bound


@pytest.mark.parametrize("T", [65, 257])
def test_rope_attention_item_alone_equals_item_in_batch(T):
    from amphion_amd.modules import hip_ops

    mask = _masks(T)[-1][1]
    d, got, _, _ = _attention_case(T, mask)
    C = H * DK
    cos, sin = (t.cuda() for t in R.rope_cos_sin(T, DK))
    for b in range(B):
        one = d[b:b + 1].contiguous()
        alone = hip_ops.rope_attention(one[:, :C], one[:, C:2 * C], one[:, 2 * C:], H, cos, sin, mask[b:b + 1].cuda())
        assert torch.equal(alone[0], got[b])


def test_rope_attention_f32_route_and_range_flag(conv_precision):
    """the exact-fp32 route (RoPE in torch + SDPA) meets the same bound; the f16x3 kernel raises the op-level range flag for an operand of 1e5"""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    T = 129
    mask = _masks(T)[-1][1]
    d, got, ref, cpu = _attention_case(T, mask)
    e32, bound = _bound(cpu, ref, conv_precision)
    print(f"rope_attention {conv_precision} T={T}: gpu {_err(got, ref):.3e} bound {bound:.3e}")
    assert _err(got, ref) <= bound
    _lib.range_check()
    if conv_precision == "f16x3":
        C = H * DK
        big = d.clone()
        big[0, 2 * C + 3, 5] = 1e5               # a V operand of a valid key
        cos, sin = (t.cuda() for t in R.rope_cos_sin(T, DK))
        hip_ops.rope_attention(big[:, :C], big[:, C:2 * C], big[:, 2 * C:], H, cos, sin, None)
        with pytest.raises(_lib.AmpError) as e:
            _lib.range_check()
        assert e.value.status == _lib.AMP_ERR_RANGE
        _lib.range_check()                       # cleared


@pytest.mark.parametrize("C", [7, 128, 1024])
@pytest.mark.parametrize("T", [1, 255, 257])
def test_rms_norm_c_adaptive(C, T):
    """w is a slice of a wider tensor, read through its batch stride"""
    from amphion_amd.modules import hip_ops

    g = _gen("rms", C, T)
    Bn = max(2, -(-20000 // (C * T)))
    x = torch.randn(Bn, C, T, generator=g) * 3.0
    wide = 1.0 + 0.3 * torch.randn(Bn, 3 * C, generator=g)
    w = wide[:, C:2 * C]
    ref = R.adaptive_rms_norm(x.double().transpose(1, 2), w.double()).transpose(1, 2)
    cpu = R.adaptive_rms_norm(x.transpose(1, 2), w).transpose(1, 2)
    got = hip_ops.rms_norm_c_adaptive(x.cuda(), wide.cuda()[:, C:2 * C], eps=R.EPS)
    e32, bound = _bound(cpu, ref, "rms")
    print(f"rms_norm_c_adaptive C={C} T={T} B={Bn}: gpu {_err(got, ref):.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert _err(got, ref) <= bound


@pytest.mark.parametrize("n", [20003, 40964, 262147])
def test_silu(n):
    from amphion_amd.modules import hip_ops

    x = torch.randn(n, generator=_gen("silu", n)) * 4.0
    ref = torch.nn.functional.silu(x.double())
    e32, bound = _bound(torch.nn.functional.silu(x), ref, "silu")
    d = x.cuda()
    got = hip_ops.silu(d)
    print(f"silu n={n}: gpu {_err(got, ref):.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert _err(got, ref) <= bound
    if n > 4:                                                                              # a base that is not 16-byte aligned: the scalar form
        assert torch.equal(hip_ops.silu(d[1:]), got[1:])
    assert torch.equal(hip_ops.silu(d, out=d), got)                                        # in place


@pytest.mark.parametrize("F,T", [(5, 7), (12, 85), (33, 601), (256, 100)])
def test_swiglu(F, T):
    """F * T = 35, 1020 (a multiple of 4, not of the block), 19833, 25600 (whole blocks); the batch holds at least 20 000 outputs"""
    from amphion_amd.modules import hip_ops

    Bn = max(3, -(-20000 // (F * T)))
    gu = torch.randn(Bn, 2 * F, T, generator=_gen("swiglu", F, T)) * 3.0
    f = lambda t: torch.nn.functional.silu(t[:, :F]) * t[:, F:]
    ref = f(gu.double())
    e32, bound = _bound(f(gu), ref, "swiglu")
    got = hip_ops.swiglu(gu.cuda())
    print(f"swiglu F={F} T={T}: gpu {_err(got, ref):.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert got.shape == (Bn, F, T) and _err(got, ref) <= bound


def test_refusals():
    """host-side checks only: nothing here launches"""
    import ctypes

    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    L = _lib.lib()
    T = 8
    x = torch.zeros(1, 3 * 64, T).cuda()
    cos, sin = (t.cuda() for t in R.rope_cos_sin(T, 64))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.zeros(1, 64, T).cuda()
    args = lambda **k: [k.get("q", p(x)), p(x[:, 64:]), p(x[:, 128:]), 3 * 64 * T, p(cos), p(sin), None, k.get("B", 1), k.get("H", 1), k.get("dk", 64),
                        k.get("T", T), ctypes.c_float(0.125), k.get("out", p(out)), None]
    for kw in (dict(dk=48), dict(dk=128), dict(T=0), dict(B=0), dict(q=None), dict(out=None), dict(T=40000), dict(B=70000), dict(out=p(x))):
        assert L.amp_rope_attention(*args(**kw)) == _lib.AMP_ERR_INVALID, kw
        assert L.amp_last_error()
    assert L.amp_rms_norm_c_adaptive(None, p(x), 0, 1, 4, 4, ctypes.c_float(1e-6), p(out), None) == _lib.AMP_ERR_INVALID
    assert L.amp_rms_norm_c_adaptive(p(x), p(x), 0, 1, 0, 4, ctypes.c_float(1e-6), p(out), None) == _lib.AMP_ERR_INVALID
    assert L.amp_silu(None, 4, p(out), None) == _lib.AMP_ERR_INVALID and L.amp_silu(p(x), 0, p(out), None) == _lib.AMP_ERR_INVALID
    assert L.amp_swiglu(None, 1, 2, 2, p(out), None) == _lib.AMP_ERR_INVALID and L.amp_swiglu(p(x), 1, 0, 2, p(out), None) == _lib.AMP_ERR_INVALID
    assert L.amp_swiglu(p(x), 1, 2, 2, p(x), None) == _lib.AMP_ERR_INVALID
    # the wrappers: mismatched shapes, head dimension, devices
    q = torch.zeros(1, 96, T).cuda()
    with pytest.raises(ValueError):
        hip_ops.rope_attention(q, q, q, 2, cos, sin)                         # dk = 48
    q = torch.zeros(1, 128, T).cuda()
    with pytest.raises(ValueError):
        hip_ops.rope_attention(q, q[:, :64], q, 2, cos, sin)
    with pytest.raises(ValueError):
        hip_ops.rope_attention(q, q, q, 2, cos[:4], sin[:4])
    with pytest.raises(ValueError):
        hip_ops.rope_attention(q, q, q, 2, cos, sin, key_mask=torch.ones(1, T + 1, dtype=torch.bool).cuda())
    with pytest.raises(ValueError):
        hip_ops.rope_attention(q[:, :, :0], q[:, :, :0], q[:, :, :0], 2, cos[:0], sin[:0])    # T = 0
    with pytest.raises(TypeError):
        hip_ops.rope_attention(q.cpu(), q, q, 2, cos, sin)
    with pytest.raises(ValueError):
        hip_ops.rms_norm_c_adaptive(q, torch.zeros(1, 64).cuda())
    with pytest.raises(ValueError):
        hip_ops.swiglu(torch.zeros(1, 3, 4).cuda())
    with pytest.raises(ValueError):
        hip_ops.silu(torch.zeros(0).cuda())


# ---- the models ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_fmt.npz"))


@pytest.fixture(scope="module")
def sd(gold):
    return R.synth_state_dict(R.small_hp(), int(gold["seed"]))


def _model(sd):
    from amphion_amd.models.vc.flow_matching_transformer import FlowMatchingTransformer

    m = FlowMatchingTransformer(**R.small_hp())
    m.load_state_dict(sd)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def forward_refs(gold, sd):
    """per T: (x, t, cond, mask, golden y, fp64 y, fp64 hidden[0], cpu32 error, bound, bound of hidden[0]): computed once and shared"""
    hp = R.small_hp()
    sd32, sd64 = R.cast(sd, torch.float32), R.cast(sd, torch.float64)
    out = {}
    for T in (37, 150):
        x, t, codes = (torch.from_numpy(gold[f"fwd_{k}_{T}"]) for k in ("x", "t", "codes"))
        cond = sd["cond_emb.weight"][codes]
        mask = torch.ones(2, T)
        mask[1, int(gold["valid"]):] = 0
        hid, hid32 = [], []
        y64 = R.diffllama_forward(sd64, hp, x.double(), t.double(), cond.double(), mask.double(), hidden=hid)
        y32 = R.diffllama_forward(sd32, hp, x, t, cond, mask, hidden=hid32)
        e32, bound = _bound(y32, y64, "fwd")
        out[T] = (x, t, cond, mask, torch.from_numpy(gold[f"fwd_y_{T}"]).double(), y64, hid[0], e32, bound, _bound(hid32[0], hid[0], "h0")[1])
    return out


@pytest.mark.parametrize("T", [37, 150])
def test_diffllama_forward(T, gold, sd, forward_refs, conv_precision):
    """hidden 128, 2 heads of 64, 2 layers, mel 20; B = 2, item 1 masked beyond frame 29.  Bound: 4 x the measured distance of the fp32 CPU
    restatement from fp64 at this shape (9.6e-7 / 1.2e-6 at T = 37 / 150 on outputs of magnitude 1.34 / 1.62, i.e. bounds of 5.1e-6 / 8.0e-6)."""
    x, t, cond, mask, ygold, y64, h64, e32, bound, hbound = forward_refs[T]
    m = _model(sd)
    r = m.diff_estimator(x.cuda(), t.cuda(), cond.cuda(), mask.cuda(), return_dict=True)
    y, h0 = r["output"], r["hidden_states"][0]
    e, eg, eh = _err(y, y64), _err(y, ygold), _err(h0, h64)
    gold_dist = float((ygold - y64).abs().max())
    print(f"DiffLlama.forward {conv_precision} T={T}: gpu-fp64 {e:.3e} (hidden[0] {eh:.3e} of {hbound:.3e}) gpu-golden {eg:.3e} cpu32-fp64 {e32:.3e} "
          f"golden-fp64 {gold_dist:.3e} bound {bound:.3e} |y|max {float(y64.abs().max()):.3f}")
    assert y.shape == (2, T, 20) and len(r["hidden_states"]) == 2 and h0.shape == (2, T, 128)
    assert e <= bound
    assert eg <= bound + gold_dist
    assert eh <= hbound                           # the first layer's output, by the same rule


@pytest.fixture(scope="module")
def rd_refs(gold, sd):
    hp = R.small_hp()
    sd32, sd64 = R.cast(sd, torch.float32), R.cast(sd, torch.float64)
    prompt, codes, noise = (torch.from_numpy(gold[k]) for k in ("rd_prompt", "rd_codes", "rd_noise"))
    cond = sd["cond_emb.weight"][codes]
    out = {"in": (prompt, cond, noise)}
    for cfg in (0.0, 2.0):
        y64 = R.reverse_diffusion(sd64, hp, cond.double(), prompt.double(), noise.double(), n_timesteps=4, cfg=cfg)
        y32 = R.reverse_diffusion(sd32, hp, cond, prompt, noise, n_timesteps=4, cfg=cfg)
        out[cfg] = (torch.from_numpy(gold[f"rd_y_{cfg}"]).double(), y64) + _bound(y32, y64, "rd")
    return out


@pytest.mark.parametrize("cfg", [0.0, 2.0])
def test_reverse_diffusion(cfg, sd, rd_refs, conv_precision):
    """prompt 11 + target 26 frames, 4 Euler steps, the golden's noise.  Bound: 4 x the measured distance of the fp32 CPU restatement from
    fp64 (7.0e-7 / 1.2e-6 at cfg 0 / 2 on outputs of magnitude 3.6, i.e. bounds of 1.0e-5 / 1.8e-5)."""
    prompt, cond, noise = rd_refs["in"]
    ygold, y64, e32, bound = rd_refs[cfg]
    m = _model(sd)
    y = m.reverse_diffusion(cond.cuda(), prompt.cuda(), n_timesteps=4, cfg=cfg, noise=noise.cuda())
    e, eg = _err(y, y64), _err(y, ygold)
    gold_dist = float((ygold - y64).abs().max())
    print(f"reverse_diffusion {conv_precision} cfg={cfg}: gpu-fp64 {e:.3e} gpu-golden {eg:.3e} cpu32-fp64 {e32:.3e} golden-fp64 {gold_dist:.3e} "
          f"bound {bound:.3e} |y|max {float(y64.abs().max()):.3f}")
    assert y.shape == (2, 26, 20)
    assert e <= bound
    assert eg <= bound + gold_dist


def test_reverse_diffusion_draws_its_noise(sd, rd_refs):
    """noise=None draws torch.randn on the device, as the reference does: reproducible under the device seed, different across seeds"""
    prompt, cond, _ = rd_refs["in"]
    m = _model(sd)
    ys = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        ys.append(m.reverse_diffusion(cond.cuda(), prompt.cuda(), n_timesteps=2, cfg=0.5))
    assert torch.equal(ys[0], ys[1]) and not torch.equal(ys[0], ys[2]) and bool(torch.isfinite(ys[2]).all())


def test_hoists_are_bit_identical(sd, forward_refs):
    """cond_mlp(cond) computed once and handed in, and cond_mlp(0) computed as ONE column, give torch.equal results to the in-forward
    computation on the full tensors"""
    x, t, cond, mask, *_ = forward_refs[37]
    est = _model(sd).diff_estimator
    xd, td, cd, md = x.cuda(), t.cuda(), cond.cuda(), mask.cuda()
    want = est(xd, td, cd, md)
    assert torch.equal(est(xd, td, None, md, cond_embedding_cf=est.cond_embedding_cf(cd)), want)
    zero = torch.zeros_like(cd)
    col = est.zero_cond_embedding_cf(2, 37, cd.device)
    assert torch.equal(col, est.cond_embedding_cf(zero))
    assert torch.equal(est(xd, td, None, md, cond_embedding_cf=col), est(xd, td, zero, md))


def test_handles_follow_their_parameters(sd, forward_refs):
    """a to_weight or q_proj parameter changed in place changes the output (the stacked handles are rebuilt), and changing it back restores it"""
    x, t, cond, mask, *_ = forward_refs[37]
    est = _model(sd).diff_estimator
    a = (x.cuda(), t.cuda(), cond.cuda(), mask.cuda())
    y0 = est(*a)
    for p in (est.layers[1].input_layernorm.to_weight.bias, est.layers[0].self_attn.q_proj.weight, est.layers[1].mlp.up_proj.weight):
        old = p.detach().clone()
        with torch.no_grad():
            p.mul_(1.5)
        y1 = est(*a)
        assert float((y1 - y0).abs().max()) > 1e-4
        with torch.no_grad():
            p.copy_(old)
        assert torch.equal(est(*a), y0)


def test_adaptive_rms_norm_module(sd):
    """LlamaAdaptiveRMSNorm.forward on its own, batch-first as the reference takes it: to_weight on the pointwise GEMM, then the norm kernel"""
    m = _model(sd).diff_estimator.layers[0].input_layernorm
    g = _gen("norm module")
    x, c = torch.randn(3, 41, 128, generator=g), torch.randn(3, 128, generator=g)
    p = "diff_estimator.layers.0.input_layernorm.to_weight."
    f = lambda dt: R.adaptive_rms_norm(x.to(dt), torch.nn.functional.linear(c.to(dt), sd[p + "weight"].to(dt), sd[p + "bias"].to(dt)))
    ref = f(torch.float64)
    e32, bound = _bound(f(torch.float32), ref, "norm")
    got = m(x.cuda(), c.cuda())
    print(f"LlamaAdaptiveRMSNorm: gpu {_err(got, ref):.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert got.shape == (3, 41, 128) and _err(got, ref) <= bound


def test_eval_only_and_argument_checks(sd, forward_refs):
    x, t, cond, mask, *_ = forward_refs[37]
    m = _model(sd)
    est = m.diff_estimator
    for f in (lambda: m(x, mask), lambda: m.compute_loss(x, mask), lambda: m.loss_t(x, mask, t), lambda: m.forward_diffusion(x, t)):
        with pytest.raises(NotImplementedError, match="eval-only"):
            f()
    with pytest.raises(NotImplementedError, match="eval-only"):
        est.train()(x.cuda(), t.cuda(), cond.cuda(), mask.cuda())
    est.eval()
    with pytest.raises(RuntimeError):
        est(x, t, cond, mask)                     # host tensors
    with pytest.raises(ValueError):
        est(x.cuda()[:, :, :19], t.cuda(), cond.cuda(), mask.cuda())
    with pytest.raises(ValueError):
        est(x.cuda(), t.cuda(), cond.cuda(), mask.cuda()[:, :30])
    from amphion_amd.models.vc.flow_matching_transformer import DiffLlama

    with pytest.raises(NotImplementedError):
        DiffLlama(mel_dim=20, hidden_size=96, num_heads=2, num_layers=1)      # dk = 48


def test_reverse_diffusion_into_vocos(sd, rd_refs):
    """end to end, as models/vc/vevo/vevo_utils.py:554-563 composes it: reverse_diffusion -> the Vocos vocoder on mel.transpose(1, 2) gives a
    finite wave of T * hop samples"""
    from amphion_amd.models.codec.amphion_codec.vocos import Vocos

    prompt, cond, noise = rd_refs["in"]
    m = _model(sd)
    mel = m.reverse_diffusion(cond.cuda(), prompt.cuda(), n_timesteps=2, cfg=1.0, noise=noise.cuda())
    torch.manual_seed(0)
    voc = Vocos(input_channels=20, dim=32, intermediate_dim=64, num_layers=2, n_fft=64, hop_size=16, padding="same").cuda().eval()
    wav = voc(mel.transpose(1, 2))
    assert wav.shape[0] == 2 and wav.shape[-1] == 26 * 16 and bool(torch.isfinite(wav).all())
