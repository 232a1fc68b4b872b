"""MaskGCT on the GPU, through module -> ctypes -> C ABI: ``amp_rope_attention`` at head dimension 96 (the T2S model's 1536 / 16), the decoding
step's sampler ``amp_mask_sample``, then the two estimators and the two ``reverse_diffusion`` loops against the golden outputs of the real
reference classes (tests/golden/make_golden_maskgct.py) and the fp64 restatement (tests/maskgct_ref.py).

Bounds.  Continuous outputs follow the ops rule of DESIGN.md section 5: 4 x the error of THE SAME FORMULA evaluated by torch in fp32 on the CPU
against fp64 on the same inputs, scaled by max(1, |ref|max).  Sampled ids are compared with the fp32 torch formula on the CPU on every DECIDED
row: torch's best-minus-second noisy value exceeds tau_row = 2^-19 * max(1, max over the kept entries of |l / temp| and |g|) -- both sides may
differ by one rounding of l / temp, about two ulps of g from the two 1-ulp logarithms and the sum's rounding, below 2^-22 * scale, times the
project's factor 8.  Rows whose k-th and (k + 1)-th logits tie are left out (torch leaves the kept set unspecified there).  The left-out
share is printed and must stay <= 1 % per case.  Models: the fp32 CPU restatement's distance from fp64 at these very shapes is measured here
and the GPU is allowed 4 x that (the rule of DESIGN.md section 20); tokens are compared on the goldens' own draws, every stored run being
decided (tests/test_oracle_maskgct.py).  Every test prints its figures before it asserts."""
import ctypes
import math
import zlib

import pytest
import torch

import fmt_ref as R
import maskgct_ref as M

pytestmark = pytest.mark.gpu

B, H, DK = 2, 2, 96
T_GRID = [2, 31, 63, 64, 65, 129, 600]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _err(got, ref64):
    return float((got.double().cpu() - ref64).abs().max())


def _bound(cpu32, ref64):
    """4 x the fp32 CPU evaluation's error, scaled by max(1, |ref|max)"""
    e32 = float((cpu32.double() - ref64).abs().max())
    return e32, 4.0 * e32 * max(1.0, float(ref64.abs().max()))


# ---- amp_rope_attention at dk = 96 ------------------------------------------------------------------------------------------------
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

    g = _gen("attn96", T, qscale)
    C = H * DK
    qkv = torch.randn(B, 3 * C, T, generator=g)
    qkv[:, :C] *= qscale
    if fill is not None and mask is not None:        # masked K / V columns hold a large finite number
        bad = (~mask)[:, None, :].expand(B, 2 * C, T)
        qkv[:, C:][bad] = fill
    cos, sin = R.rope_cos_sin(T, DK)
    q64, k64, v64 = (t.double() for t in qkv.split(C, 1))
    if fill is not None and mask is not None:        # the references take zeros there
        bad = (~mask)[:, None, :].expand(B, C, T)
        k64, v64 = k64.masked_fill(bad, 0.0), v64.masked_fill(bad, 0.0)
    ref = R.rope_attention_cf(q64, k64, v64, H, cos.double(), sin.double(), mask)
    cpu = R.rope_attention_cf(q64.float(), k64.float(), v64.float(), H, cos, sin, mask)
    d = qkv.cuda()
    got = hip_ops.rope_attention(d[:, :C], d[:, C:2 * C], d[:, 2 * C:], H, cos.cuda(), sin.cuda(), None if mask is None else mask.cuda())
    return d, got, ref, cpu


@pytest.mark.parametrize("T", T_GRID)
def test_rope_attention_96_vs_fp64(T):
    """q | k | v are strided views of one [B, 3 H dk, T] tensor; masked K / V columns hold 1e30"""
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    fails = []
    for name, mask in _masks(T):
        d, got, ref, cpu = _attention_case(T, mask, fill=1e30)
        e32, bound = _bound(cpu, ref)
        e = _err(got, ref)
        print(f"rope_attention dk=96 T={T} mask={name}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
        assert got.shape == (B, H * DK, T) and bool(torch.isfinite(got).all())
        if not e <= bound:
            fails.append((name, e, bound))
        _lib.range_check()                       # 1e30 in masked columns is not an operand
    assert not fails, fails


def test_rope_attention_96_one_key_is_exact():
    """T = 1: the softmax over the one key is exactly 1 and the entry point returns v's bits"""
    from amphion_amd.modules import hip_ops

    C = H * DK
    qkv = torch.randn(B, 3 * C, 1, generator=_gen("attn96", 1)).cuda()
    cos, sin = (t.cuda() for t in R.rope_cos_sin(1, DK))
    got = hip_ops.rope_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], H, cos, sin)
    assert torch.equal(got, qkv[:, 2 * C:])


def test_rope_attention_96_moving_maximum():
    """q x 30: scores of magnitude ~ 30 sigma, the running maximum moves from tile to tile and the rescale branch runs"""
    T = 257
    d, got, ref, cpu = _attention_case(T, _masks(T)[-1][1], qscale=30.0)
    e32, bound = _bound(cpu, ref)
    e = _err(got, ref)
    print(f"rope_attention dk=96 q x 30 T={T}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert e <= bound


@pytest.mark.parametrize("T", [65, 257])
def test_rope_attention_96_item_alone_equals_item_in_batch(T):
    from amphion_amd.modules import hip_ops

    mask = _masks(T)[-1][1]
    d, got, _, _ = _attention_case(T, mask)
    C = H * DK
    cos, sin = (t.cuda() for t in R.rope_cos_sin(T, DK))
    for b in range(B):
        one = d[b:b + 1].contiguous()
        alone = hip_ops.rope_attention(one[:, :C], one[:, C:2 * C], one[:, 2 * C:], H, cos, sin, mask[b:b + 1].cuda())
        assert torch.equal(alone[0], got[b])


def test_rope_attention_96_f32_route_and_range_flag(conv_precision):
    """the exact-fp32 route (RoPE in torch + SDPA) meets the same bound; the f16x3 kernel raises the op-level range flag for an operand of 1e5"""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    T = 129
    mask = _masks(T)[-1][1]
    d, got, ref, cpu = _attention_case(T, mask)
    e32, bound = _bound(cpu, ref)
    print(f"rope_attention dk=96 {conv_precision} T={T}: gpu {_err(got, ref):.3e} bound {bound:.3e}")
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


# ---- amp_mask_sample --------------------------------------------------------------------------------------------------------------
TEMPS = [1.5, 0.9, 0.045, 1e-3]
SAMPLE_T = [1, 15, 16, 17, 257]
# the issue's grid, and the sizes on either side of the kernel's two register-form thresholds (1024 | 1025, 4096 | 4097)
SAMPLE_V = [2, 3, 63, 64, 65, 1000, 1024, 1025, 4096, 4097, 8191, 8192]


def _ks(V):
    return sorted({1, min(2, V), math.ceil(0.02 * V), V})


def _sub_cases(V):
    """every k at every T below 257, one k (rotating with V) at T = 257; B alternates 1 | 3, the temperature rotates; the last entry has a
    +-1e4 outlier in every row"""
    ks, out, n = _ks(V), [], 0
    for T in SAMPLE_T:
        for k in (ks if T < 257 else [ks[V % len(ks)]]):
            out.append(dict(T=T, k=k, Bn=(1, 3)[n % 2], temp=TEMPS[n % 4], outlier=False))
            n += 1
    out.append(dict(T=17, k=ks[-2], Bn=3, temp=0.9, outlier=True))
    return out


def _sample_inputs(V, c):
    g = _gen("sample", V, c["T"], c["k"], c["Bn"], c["temp"], c["outlier"])
    Bn, T = c["Bn"], c["T"]
    wide = torch.randn(Bn, V + 3, T, generator=g) * 4.0          # the logits are rows [0, V) of it: a batch stride wider than V * T
    if c["outlier"]:
        where = torch.randint(0, V, (Bn, 1, T), generator=g)
        sign = torch.where(torch.rand(Bn, 1, T, generator=g) < 0.5, -1.0, 1.0)
        wide[:, :V].scatter_(1, where, 1e4 * sign)
    u = torch.rand(Bn, T, V, generator=g)
    return wide, u


@pytest.mark.parametrize("V", SAMPLE_V)
def test_mask_sample_vs_torch(V):
    from amphion_amd.modules import hip_ops

    rows = left_out = 0
    e_gpu = e_cpu = ref_max = 0.0
    fails = []
    for c in _sub_cases(V):
        wide, u = _sample_inputs(V, c)
        k, temp = c["k"], c["temp"]
        lg = wide[:, :V].transpose(1, 2).contiguous()                      # [B, T, V] as the reference sees it
        ids32, sc32, f32, y32 = M.mask_sample(lg, k, u, temp)
        gids32, gsc32, _, _ = M.mask_sample(lg, k, None)
        ids64, sc64, _, _ = M.mask_sample(lg.double(), k, u.double(), temp)
        d = wide.cuda()
        ids, sc = hip_ops.mask_sample(d[:, :V], k, u.cuda(), temp)
        gids, gsc = hip_ops.mask_sample(d[:, :V], k)
        ids2, sc2 = hip_ops.mask_sample(d[:, :V], k, u.cuda(), temp)
        assert ids.shape == (c["Bn"], c["T"]) and ids.dtype == torch.int64 and sc.dtype == torch.float32
        assert torch.equal(ids, ids2) and torch.equal(sc, sc2), "not deterministic"
        ids, sc, gids, gsc = ids.cpu(), sc.cpu(), gids.cpu(), gsc.cpu()
        assert int(ids.min()) >= 0 and int(ids.max()) < V
        # rows left out: a tie at the k-th value, or an undecided noisy argmax
        srt = lg.sort(-1, descending=True).values
        tied = (srt[..., k - 1] == srt[..., k]) if k < V else torch.zeros_like(ids32, dtype=torch.bool)
        kept = torch.isfinite(f32)
        scale = torch.maximum((f32 / max(temp, 1e-10)).abs().masked_fill(~kept, 0.0).amax(-1), M.gumbel(u).abs().masked_fill(~kept, 0.0).amax(-1))
        tau = 2.0 ** -19 * scale.clamp_min(1.0)
        if k > 1:
            top2 = y32.topk(2, -1).values
            decided = (top2[..., 0] - top2[..., 1]) > tau
        else:
            decided = torch.ones_like(tied)
        use = decided & ~tied
        rows += use.numel()
        left_out += int((~use).sum())
        if not torch.equal(gids[~tied], gids32[~tied]):
            fails.append(("greedy ids", c))
        if not torch.equal(ids[use], ids32[use]):
            fails.append(("sampled ids", c, int((ids[use] != ids32[use]).sum())))
        # scores: against fp64 at the id both sides chose
        _, g64, _, _ = M.mask_sample(lg.double(), k, None)
        ok = use & (ids == ids32) & (ids32 == ids64)
        for got, cpu, ref, sel in ((sc, sc32, sc64, ok), (gsc, gsc32, g64, ~tied & (gids == gids32))):
            if bool(sel.any()):
                e_gpu = max(e_gpu, float((got[sel].double() - ref[sel]).abs().max()))
                e_cpu = max(e_cpu, float((cpu[sel].double() - ref[sel]).abs().max()))
                ref_max = max(ref_max, float(ref[sel].abs().max()))
    bound = 4.0 * e_cpu * max(1.0, ref_max)
    print(f"mask_sample V={V}: {rows} rows, {left_out} left out ({100.0 * left_out / rows:.3f} %); score gpu {e_gpu:.3e} cpu32 {e_cpu:.3e} bound {bound:.3e}")
    assert not fails, fails
    assert left_out <= 0.01 * rows
    assert e_gpu <= bound


def test_mask_sample_ties_go_to_the_lower_index():
    """a row of equal logits: the kept set is the first k indices, the greedy id is 0, and with equal noise the sampled id is 0 as well"""
    from amphion_amd.modules import hip_ops

    for V, k in ((65, 3), (1025, 21), (8192, 164)):
        lg = torch.zeros(2, V, 5).cuda()
        u = torch.rand(2, 5, V, generator=_gen("tie", V))
        u[..., k:] = 0.999999                                          # the largest noise sits outside the kept set
        ids, sc = hip_ops.mask_sample(lg, k, u.cuda(), 0.9)
        y = M.gumbel(u[..., :k])
        assert torch.equal(ids.cpu(), y.argmax(-1)), (V, k)
        assert float((sc.cpu() - 1.0 / k).abs().max()) <= 4.0 * 2.0 ** -24
        ids, _ = hip_ops.mask_sample(lg, k, torch.full((2, 5, V), 0.5).cuda(), 0.9)
        assert int(ids.abs().max()) == 0
        ids, _ = hip_ops.mask_sample(lg, k)
        assert int(ids.abs().max()) == 0


def test_mask_sample_nan_logits_stay_inside():
    """logits are assumed finite; a NaN must still give ids in [0, V) (the scores of such rows are NaN)"""
    from amphion_amd.modules import hip_ops

    V, T = 65, 17
    lg = torch.randn(2, V, T, generator=_gen("nan")) * 4.0
    lg[0, 7, 3] = float("nan")
    lg[1, :, 5] = float("nan")
    lg[1, 64, 6] = -float("nan")
    d = lg.cuda()
    for u in (None, torch.rand(2, T, V, generator=_gen("nan", "u")).cuda()):
        for k in (1, 2, V):
            ids, sc = hip_ops.mask_sample(d, k, u, 0.9)
            assert int(ids.min()) >= 0 and int(ids.max()) < V
            assert bool(torch.isfinite(sc[0, 4:]).all())


def test_mask_sample_refusals():
    """host-side checks only: nothing here launches"""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    L = _lib.lib()
    V, T = 8, 4
    x = torch.zeros(1, V, T).cuda()
    u = torch.zeros(1, T, V).cuda()
    ids = torch.zeros(1, T, dtype=torch.int64).cuda()
    sc = torch.zeros(1, T).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    args = lambda **k: [k.get("x", p(x)), k.get("bs", 0), k.get("B", 1), k.get("V", V), k.get("T", T), k.get("k", 2), k.get("u", p(u)),
                        ctypes.c_float(k.get("temp", 1.0)), k.get("ids", p(ids)), k.get("sc", p(sc)), None]
    for kw in (dict(V=1), dict(V=8193), dict(k=0), dict(k=V + 1), dict(x=None), dict(ids=None), dict(sc=None), dict(B=0), dict(T=0), dict(B=70000),
               dict(bs=V * T - 1), dict(temp=float("nan")), dict(ids=p(x)), dict(sc=p(x)), dict(sc=p(u)), dict(sc=p(ids))):
        assert L.amp_mask_sample(*args(**kw)) == _lib.AMP_ERR_INVALID, kw
        assert L.amp_last_error()
    with pytest.raises(ValueError):
        hip_ops.mask_sample(x, 0)
    with pytest.raises(ValueError):
        hip_ops.mask_sample(x, 2, u[:, :, :4])
    with pytest.raises(ValueError):
        hip_ops.mask_sample(torch.zeros(1, 8193, 2).cuda(), 2)
    with pytest.raises(TypeError):
        hip_ops.mask_sample(x.cpu(), 2)


# ---- the models -------------------------------------------------------------------------------------------------------------------
import os  # noqa: E402

import numpy as np  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HPS = {"s2a": M.small_hp_s2a(), "t2s": M.small_hp_t2s()}
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "golden_maskgct.npz")))
    g.update(np.load(os.path.join(GOLDEN, "golden_maskgct_embeds.npz")))
    return g


@pytest.fixture(scope="module")
def sds(gold):
    return {k: M.synth_state_dict(k, HPS[k], int(gold["seed"])) for k in HPS}


def _model(kind, sd):
    from amphion_amd.models.tts.maskgct import MaskGCT_S2A, MaskGCT_T2S

    m = (MaskGCT_S2A if kind == "s2a" else MaskGCT_T2S)(**HPS[kind])
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _draws(gold, name):
    return [torch.from_numpy(gold[f"{name}_u{i}"]) for i in range(int(gold[f"{name}_ndraws"]))]


def _run(model, kind, inp, cfg, gt, noise, **kw):
    """a golden's recipe through the HIP model"""
    if kind == "s2a":
        return model.reverse_diffusion(model.cond_emb(inp["codes"].to(DEV)), inp["prompt"].to(DEV), temp=M.S2A_TEMP, filter_thres=M.S2A_THRES,
                                       gt_code=inp["gt"].to(DEV) if gt else None, n_timesteps=M.S2A_STEPS, cfg=cfg, rescale_cfg=M.RESCALE,
                                       noise=noise, **kw)
    return model.reverse_diffusion(inp["prompt"].to(DEV), M.TT, inp["phones"].to(DEV), temp=M.T2S_TEMP, filter_thres=M.T2S_THRES,
                                   n_timesteps=M.T2S_STEPS, cfg=cfg, rescale_cfg=M.RESCALE, noise=noise, **kw)


def test_estimator_forwards_vs_fp64(conv_precision, gold, sds):
    """DiffLlama at T = 37 and 150 (dk 64), DiffLlamaPrefix with 9 phones and without (dk 96); item 1 masked beyond frame 29.  Bound: 4 x the
    measured distance of the fp32 CPU restatement from fp64 at the same shape x max(1, |ref|max)"""
    valid, fails = int(gold["valid"]), []
    cast = lambda sd, dt: {k: v.to(dt) for k, v in sd.items()}
    s2a, t2s = _model("s2a", sds["s2a"]), _model("t2s", sds["t2s"])
    cases = []
    for T in (37, 150):
        x, t, cond, mask = M.diffllama_inputs(HPS["s2a"], T, valid)
        ref = M.diffllama_forward(cast(sds["s2a"], torch.float64), HPS["s2a"], x.double(), t.double(), cond.double(), mask.double())
        cpu = torch.from_numpy(gold[f"dl_y_{T}"])
        cases.append((f"DiffLlama T={T}", s2a.diff_estimator(x.to(DEV), t.to(DEV), cond.to(DEV), mask.to(DEV)), cpu, ref))
    x, t, ph, mask, pmask = M.prefix_inputs(HPS["t2s"], valid)
    sd64 = cast(sds["t2s"], torch.float64)
    ref = M.prefix_forward(sd64, HPS["t2s"], x.double(), t.double(), mask.double(), ph.double(), pmask.double())
    cases.append(("DiffLlamaPrefix 9 phones", t2s.diff_estimator(x.to(DEV), t.to(DEV), mask.to(DEV), phone_embedding=ph.to(DEV), phone_mask=pmask.to(DEV)),
                  torch.from_numpy(gold["px_y_phones"]), ref))
    ref = M.prefix_forward(sd64, HPS["t2s"], x.double(), t.double(), mask.double())
    cases.append(("DiffLlamaPrefix plain", t2s.diff_estimator(x.to(DEV), t.to(DEV), mask.to(DEV)), torch.from_numpy(gold["px_y_plain"]), ref))
    cases.append(("DiffLlamaPrefix zero phones", t2s.diff_estimator(x.to(DEV), t.to(DEV), mask.to(DEV), phone_embedding=ph[:, :0].to(DEV),
                                                                    phone_mask=pmask[:, :0].to(DEV)), torch.from_numpy(gold["px_y_plain"]), ref))
    for name, got, cpu, ref in cases:
        e32, bound = _bound(cpu, ref)
        e = _err(got, ref)
        print(f"{name} {conv_precision}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
        assert got.shape == ref.shape
        if not e <= bound:
            fails.append((name, e, bound))
    assert not fails, fails


@pytest.mark.parametrize("name", list(M.RUNS))
def test_reverse_diffusion_replays_the_golden(gold, sds, name):
    """on the golden's own draws the tokens are the golden's (every stored run is decided, tests/test_oracle_maskgct.py); where every step's
    embeds are stored, each of them meets the estimator bound against the fp64 restatement on the same trajectory"""
    kind, cfg, gt = M.RUNS[name]
    hp, sd = HPS[kind], sds[kind]
    inp = M.sampler_inputs(kind, hp, int(gold[f"{name}_seed"]))
    draws, rec = _draws(gold, name), []
    replay = M.Replay(draws)
    y = _run(_model(kind, sd), kind, inp, cfg, gt, replay, record=rec)
    want = torch.from_numpy(gold[f"{name}_y"])
    print(f"{name}: {int((y.cpu() != want).sum())} of {want.numel()} tokens differ from the golden; {replay.i} of {len(draws)} draws taken")
    assert y.dtype == torch.int64 and y.shape == want.shape and replay.i == len(draws)
    assert torch.equal(y.cpu(), want)
    if f"{name}_embeds" in gold:
        rec64 = []
        M.golden_run(kind, sd, hp, inp, cfg, gt, M.Replay(draws), torch.float64, record=rec64)
        fails = []
        for i, (got, cpu, ref) in enumerate(zip(rec, torch.from_numpy(gold[f"{name}_embeds"]), rec64)):
            e32, bound = _bound(cpu, ref)
            e = _err(got, ref)
            print(f"  step {i}: embeds gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
            if not e <= bound:
                fails.append((i, e, bound))
        assert len(rec) == len(rec64) and not fails, fails


def test_reverse_diffusion_draws_its_own_noise(sds):
    s2a, t2s = _model("s2a", sds["s2a"]), _model("t2s", sds["t2s"])
    inp = M.sampler_inputs("t2s", HPS["t2s"], 5)
    y = _run(t2s, "t2s", inp, 2.5, False, None)
    assert y.shape == (2, M.TT) and y.dtype == torch.int64 and int(y.min()) >= 0 and int(y.max()) < HPS["t2s"]["cond_codebook_size"]
    inp = M.sampler_inputs("s2a", HPS["s2a"], 5)
    y = _run(s2a, "s2a", inp, 2.5, False, None)
    assert y.shape == (2, M.TT, 3) and y.dtype == torch.int64 and int(y.min()) >= 0 and int(y.max()) < HPS["s2a"]["codebook_size"]
    y = _run(s2a, "s2a", inp, 0.0, False, None, max_layer=2)
    assert y.shape == (2, M.TT, 2)


def test_t2s_more_phones_than_prompt_is_refused(sds):
    """the reference's unconditional branch fails with a shape error when P > prompt_len; P <= prompt_len and cfg = 0 run"""
    t2s = _model("t2s", sds["t2s"])
    prompt = torch.randint(0, 128, (2, 5), generator=_gen("quirk")).to(DEV)
    phones = torch.randint(0, 1023, (2, 6), generator=_gen("quirk", 2)).to(DEV)
    with pytest.raises(ValueError, match="prompt_len"):
        t2s.reverse_diffusion(prompt, 7, phones, n_timesteps=2, cfg=2.5)
    assert t2s.reverse_diffusion(prompt, 7, phones, n_timesteps=2, cfg=0.0).shape == (2, 7)
    assert t2s.reverse_diffusion(prompt, 7, phones[:, :5], n_timesteps=2, cfg=2.5).shape == (2, 7)


def test_hoisted_quantities_equal_the_per_step_form(sds):
    """what the samplers compute once per call or per layer is bit for bit what the reference computes in every step"""
    from amphion_amd.modules import hip_ops

    s2a, t2s = _model("s2a", sds["s2a"]), _model("t2s", sds["t2s"])
    inp = M.sampler_inputs("s2a", HPS["s2a"], 9)
    est = s2a.diff_estimator
    cond = s2a.cond_emb(inp["codes"].to(DEV))
    prompt = inp["prompt"].to(DEV)
    for layer in (0, 2):
        temp_cond = cond + s2a.layer_emb(torch.tensor([layer], device=DEV)).unsqueeze(1)
        hoisted = s2a.layer_cond_cf(cond, layer)
        assert torch.equal(hoisted, est.cond_embedding_cf(temp_cond))
        assert torch.equal(hoisted[:, :, M.TP:], est.cond_embedding_cf(temp_cond[:, M.TP:, :]))          # the unconditional branch's slice
        x = torch.randn(2, M.TP + M.TT, 128, generator=_gen("hoist", layer)).to(DEV)
        t = torch.full((2,), 0.75, device=DEV)
        assert torch.equal(est(x, t, temp_cond, None), est(x, t, None, None, cond_embedding_cf=hoisted))
    cur_prompt = 0
    for idx, emb in enumerate(s2a.token_emb):
        cur_prompt = cur_prompt + emb(prompt[:, :, idx])
    assert torch.equal(s2a.prompt_embedding_cf(prompt), cur_prompt.transpose(1, 2))
    # the step's input through the extended table: cum + mask * mask_token + ~mask * token_emb(seq)
    g = _gen("input")
    cum = torch.randn(2, M.TT, 128, generator=g).to(DEV)
    seq = torch.randint(0, 64, (2, M.TT), generator=g).to(DEV)
    mask = (torch.rand(2, M.TT, generator=g) < 0.5).to(DEV)
    mask_token = s2a.mask_emb(torch.zeros(1, dtype=torch.long, device=DEV))
    want = cum + mask[..., None] * mask_token[:, None, :] + (~mask[..., None]) * s2a.token_emb[1](seq)
    table = s2a._ext[1].get(s2a.token_emb[1], s2a.mask_emb)
    got = hip_ops.embed_sum_c(torch.where(mask, 64, seq)[None], [table], cum.transpose(1, 2).contiguous())
    assert torch.equal(got, want.transpose(1, 2))
    inp = M.sampler_inputs("t2s", HPS["t2s"], 9)
    phones, prompt = inp["phones"].to(DEV), inp["prompt"].to(DEV)
    assert torch.equal(t2s.phone_embedding_cf(phones), t2s.diff_estimator.cond_embedding_cf(t2s.phone_emb(phones)))
    assert torch.equal(t2s.prompt_embedding_cf(prompt), (0 + t2s.cond_emb(prompt)).transpose(1, 2))


def test_handles_follow_their_parameters(gold, sds):
    """a parameter changed in place rebuilds what was packed from it: to_logit, a token table (the extended table) and phone_emb"""
    for kind, name, keys in (("t2s", "t2s_cfg25", ("to_logit.weight", "cond_emb.weight", "phone_emb.weight", "mask_emb.weight")),
                             ("s2a", "s2a_cfg0", ("to_logits.1.weight", "token_emb.0.weight"))):
        _, cfg, gt = M.RUNS[name]
        inp = M.sampler_inputs(kind, HPS[kind], int(gold[f"{name}_seed"]))
        draws = _draws(gold, name)
        model = _model(kind, sds[kind])
        before = _run(model, kind, inp, cfg, gt, M.Replay(draws))
        for key in keys:
            sd = {k: v.clone() for k, v in model.state_dict().items()}
            with torch.no_grad():
                p = dict(model.named_parameters())[key]
                p.mul_(-1.5)                                                   # in place: same address, another version
            sd[key] = sd[key] * -1.5
            after = _run(model, kind, inp, cfg, gt, M.Replay(draws))
            fresh = _run(_model(kind, sd), kind, inp, cfg, gt, M.Replay(draws))
            print(f"{kind} {key}: {int((after != before).sum())} tokens moved")
            assert torch.equal(after, fresh), key
            assert not torch.equal(after, before), key
            before = after


def test_end_to_end_phones_to_wave(sds):
    """T2S tokens -> S2A codes -> CodecDecoder.vq2emb -> decoder: a finite wave of T x hop samples, entirely on this library"""
    import codec_ref as C
    from amphion_amd.models.codec.amphion_codec.codec import CodecDecoder

    t2s, s2a = _model("t2s", sds["t2s"]), _model("s2a", sds["s2a"])
    fhp = C.small_fvq_hp()                                                     # three quantizers of 64 codes, as the small S2A
    dec = CodecDecoder(**C.decoder_kwargs(fhp))
    dec.load_state_dict(C.decoder_state_dict(fhp, 11))
    dec = dec.to(DEV).eval()
    inp = M.sampler_inputs("t2s", HPS["t2s"], 21)
    prompt_sem = inp["prompt"].to(DEV) % HPS["s2a"]["cond_codebook_size"]                   # the small S2A's semantic codebook has 97 entries
    target_sem = t2s.reverse_diffusion(inp["prompt"].to(DEV), M.TT, inp["phones"].to(DEV), n_timesteps=5, cfg=2.5, rescale_cfg=0.75, filter_thres=0.9)
    sem = torch.cat([prompt_sem, target_sem % HPS["s2a"]["cond_codebook_size"]], dim=1)
    prompt_ac = M.sampler_inputs("s2a", HPS["s2a"], 21)["prompt"].to(DEV)
    codes = s2a.reverse_diffusion(s2a.cond_emb(sem), prompt_ac, n_timesteps=[4, 2, 1], cfg=2.5, rescale_cfg=0.75, filter_thres=0.9)
    assert codes.shape == (2, M.TT, 3)
    wav = dec(dec.vq2emb(codes.permute(2, 0, 1).contiguous()))
    print(f"end to end: wave {tuple(wav.shape)}, max |wav| {float(wav.abs().max()):.3f}")
    assert wav.shape[0] == 2 and wav.shape[-1] == M.TT * C.SMALL_VOCOS_HP["hop_size"] and bool(torch.isfinite(wav).all())
