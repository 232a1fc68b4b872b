"""VALL-E on the GPU, through module -> ctypes -> C ABI: the prefix-LM prefill attention, the LayerNorm-folded T = 1 Linear, the embedding plus
position kernel, then ``VALLE.inference`` / ``continual`` against the golden outputs of the real class (tests/golden/make_golden_valle.py) and
the fp64 restatement (tests/valle_ref.py).

Bounds.  A kernel is allowed what tests/test_gpu_ar.py::_bound allows: 4 x the error of THE SAME FORMULA evaluated by torch in fp32 on the CPU
at the same inputs, scaled by max(1, |ref64|max).  Discrete results (codes) must be EQUAL: the goldens are decided, every decision at least
4 tau from its boundary (valle_ref.decidedness; tests/test_oracle_valle.py asserts it).  Every test prints its figures before it asserts."""
import ctypes
import math
import os
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import valle_ref as V
from valle_ref import CONTINUAL_FRAMES, CONTINUAL_HP, CONTINUAL_TEXT, IN_SEED, RUNS, SD_SEED

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, H, DK = 2, 2, 64
C = H * DK


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _err(got, ref64):
    return float((got.double().cpu() - ref64).abs().max())


def _bound(cpu32, ref64):
    """4 x the fp32 CPU evaluation's error, scaled by max(1, |ref|max)"""
    e32 = float((cpu32.double() - ref64).abs().max())
    return e32, 4.0 * e32 * max(1.0, float(ref64.abs().max()))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_valle.npz"))


# ---- amp_prefix_attention -------------------------------------------------------------------------------------------------------------
def _masks(T):
    out = [("none", None)]
    if T >= 3:
        m = torch.ones(B, T, dtype=torch.bool)
        m[:, T // 2] = False
        m[0, 1:max(2, T // 3)] = False
        out.append(("hole", m))
    return out


def _prefix_ref(q, k, v, prefix, mask=None):
    """q, k, v [B, H dk, T] -> [B, H dk, T]: key j is visible to query i iff (j < prefix or j <= i) and the key mask admits it"""
    Bq, Cq, T = q.shape
    sp = lambda t: t.reshape(Bq, H, DK, T).transpose(2, 3)
    j = torch.arange(T)
    hidden = ~((j[None, :] < prefix) | (j[None, :] <= j[:, None]))[None, None]
    if mask is not None:
        hidden = hidden | (~mask)[:, None, None, :]
    s = torch.matmul(sp(q), sp(k).transpose(2, 3)) / math.sqrt(DK)
    o = torch.matmul(torch.softmax(s.masked_fill(hidden, float("-inf")), dim=-1), sp(v))
    return o.transpose(2, 3).reshape(Bq, Cq, T)


def _prefix_gpu(qkv_dev, prefix, mask=None):
    from amphion_amd.modules import hip_ops

    return hip_ops.prefix_attention(qkv_dev[:, :C], qkv_dev[:, C:2 * C], qkv_dev[:, 2 * C:], H, prefix, None if mask is None else mask.cuda())


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 128, 129, 200])
def test_prefix_attention_vs_fp64(T):
    """q | k | v are strided views of one [B, 3 H dk, T] tensor; masked K / V columns hold 1e30.  T = 1 is the copy of v: bound 0."""
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    fails = []
    for prefix in sorted({p for p in (0, 1, 31, 64, 65, T) if p <= T}):
        for name, mask in _masks(T):
            qkv = torch.randn(B, 3 * C, T, generator=_gen("prefix", T, prefix))
            q64, k64, v64 = (t.double() for t in qkv.split(C, 1))
            if mask is not None:
                qkv[:, C:][(~mask)[:, None, :].expand(B, 2 * C, T)] = 1e30
            ref = _prefix_ref(q64, k64, v64, prefix, mask)
            cpu = _prefix_ref(q64.float(), k64.float(), v64.float(), prefix, mask)
            got = _prefix_gpu(qkv.cuda(), prefix, mask)
            e32, bound = _bound(cpu, ref)
            e = _err(got, ref)
            print(f"prefix attention T={T} prefix={prefix} mask={name}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
            assert got.shape == (B, C, T) and bool(torch.isfinite(got).all())
            if not e <= bound:
                fails.append((prefix, name, e, bound))
            _lib.range_check()
    assert not fails, fails


@pytest.mark.parametrize("T", [2, 64, 65, 129, 200])
def test_prefix_equal_to_T_is_cross_attention_bit_for_bit(T):
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    _lib.set_precision("f16x3")
    for name, mask in _masks(T):
        qkv = torch.randn(B, 3 * C, T, generator=_gen("full", T)).cuda()
        m = None if mask is None else mask.cuda()
        full = hip_ops.cross_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], H, m)
        assert torch.equal(_prefix_gpu(qkv, T, mask), full), (T, name)


def test_prefix_attention_ignores_the_hidden_region_bit_for_bit():
    """prefix 31 of 200: q, k and v in columns > i (i >= prefix - 1: all of them hidden from columns <= i) replaced by other finite values --
    output columns <= i keep their bits; and with prefix 0 the kernel is the causal rule from column 0"""
    T = 200
    qkv = torch.randn(B, 3 * C, T, generator=_gen("hidden"))
    other = 3.0 * torch.randn(B, 3 * C, T, generator=_gen("hidden2")) + 1.0
    for prefix in (31, 0):
        base = _prefix_gpu(qkv.cuda(), prefix).cpu()
        for i in (max(prefix - 1, 0), 31, 32, 64, 127, T - 2):
            x = qkv.clone()
            x[:, :, i + 1:] = other[:, :, i + 1:]
            got = _prefix_gpu(x.cuda(), prefix).cpu()
            assert torch.equal(got[:, :, :i + 1], base[:, :, :i + 1]), (prefix, i)
            assert not torch.equal(got[:, :, i + 1:], base[:, :, i + 1:]), (prefix, i)
    # a text column sees the whole prefix: changing a LATER text column changes an earlier one
    x = qkv.clone()
    x[:, :, 20] = other[:, :, 20]
    assert not torch.equal(_prefix_gpu(x.cuda(), 31).cpu()[:, :, :10], _prefix_gpu(qkv.cuda(), 31).cpu()[:, :, :10])


def test_prefix_attention_refuses():
    from amphion_amd.modules import hip_ops

    qkv = torch.randn(B, 3 * C, 8, generator=_gen("refuse")).cuda()
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    for prefix in (-1, 9):
        with pytest.raises(ValueError, match="prefix"):
            hip_ops.prefix_attention(q, k, v, H, prefix)
    with pytest.raises(ValueError, match="head dimension"):
        hip_ops.prefix_attention(q, k, v, 1, 0)
    with pytest.raises(ValueError, match="key_mask"):
        hip_ops.prefix_attention(q, k, v, H, 0, torch.ones(B, 7, dtype=torch.bool).cuda())
    with pytest.raises(TypeError):
        hip_ops.prefix_attention(q.cpu(), k, v, H, 0)


# ---- amp_pw_forward_vec_ln ------------------------------------------------------------------------------------------------------------
_handles = {}


def _pw_handle(cin, cout, precision):
    from amphion_amd import _lib

    key = (cin, cout, precision)
    if key not in _handles:
        g = _gen("pwln", cin, cout)
        w = (torch.randn(cout, cin, generator=g) / math.sqrt(cin)).contiguous()
        b = torch.randn(cout, generator=g).contiguous()
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().amp_pw_create(cin, cout, _lib.ptr(w), _lib.ptr(b), ctypes.byref(h)))
        _handles[key] = (h, w, b)
    return _handles[key]


# (cin, cout, epilogue): the q | k | v, linear1 and linear2 shapes of the recipe, a row count that is no multiple of 32, a small odd pair
LN_SHAPES = [(1024, 3072, "bias"), (1024, 4096, "relu"), (4096, 1024, "res"), (1024, 1025, "bias"), (72, 40, "relu")]


@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}{s[2]}")
def test_pw_forward_vec_ln_vs_fp64(shape, conv_precision):
    from amphion_amd.modules import hip_ops

    cin, cout, epi = shape
    h, w, b = _pw_handle(cin, cout, conv_precision)
    fails = []
    for nb in (1, 3, 8):
        g = _gen("pwlnx", cin, cout, nb)
        x = 1.5 * torch.randn(nb, cin, 1, generator=g) + 0.3
        lg, lb = 1.0 + 0.2 * torch.randn(cin, generator=g), 0.2 * torch.randn(cin, generator=g)
        res = torch.randn(nb, cout, 1, generator=g) if epi == "res" else None
        gamma = (1.0 + 0.5 * torch.randn(cout, generator=g)) if epi == "res" else None

        def f(dt):
            y = F.linear(F.layer_norm(x[:, :, 0].to(dt), (cin,), lg.to(dt), lb.to(dt), 1e-5), w.to(dt), b.to(dt))
            if epi == "relu":
                y = F.relu(y)
            return (res[:, :, 0].to(dt) + gamma.to(dt) * y) if epi == "res" else y
        ref, cpu = f(torch.float64), f(torch.float32)
        rd, gd = (res.cuda(), gamma.cuda()) if epi == "res" else (None, None)
        got = hip_ops.pw_forward_vec_ln(h, cout, x.cuda(), lg.cuda(), lb.cuda(), 1e-5, relu=epi == "relu", gamma=gd, res=rd)
        again = hip_ops.pw_forward_vec_ln(h, cout, x.cuda(), lg.cuda(), lb.cuda(), 1e-5, relu=epi == "relu", gamma=gd, res=rd)
        e32, bound = _bound(cpu, ref)
        e = _err(got[:, :, 0], ref)
        print(f"pw_forward_vec_ln {cin}->{cout} {epi} B={nb} {conv_precision}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
        assert got.shape == (nb, cout, 1) and torch.equal(got, again)
        if epi == "relu":
            assert float(got.min()) >= 0.0
        if not e <= bound:
            fails.append((nb, e, bound))
    assert not fails, fails


@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}{s[2]}")
def test_pw_forward_vec_ln_without_the_norm_is_pw_forward_vec(shape, conv_precision):
    """ln_gamma = NULL, relu = 0: the bits of amp_pw_forward_vec, with and without the residual epilogue"""
    from amphion_amd.modules import hip_ops

    cin, cout, epi = shape
    h, w, b = _pw_handle(cin, cout, conv_precision)
    for nb in (1, 3, 8):
        g = _gen("pwlnid", cin, cout, nb)
        x = torch.randn(nb, cin, 1, generator=g).cuda()
        res, gamma = torch.randn(nb, cout, 1, generator=g).cuda(), (1.0 + 0.5 * torch.randn(cout, generator=g)).cuda()
        assert torch.equal(hip_ops.pw_forward_vec_ln(h, cout, x), hip_ops.pw_forward_vec(h, cout, x)), nb
        assert torch.equal(hip_ops.pw_forward_vec_ln(h, cout, x, gamma=gamma, res=res), hip_ops.pw_forward_vec(h, cout, x, gamma=gamma, res=res)), nb
        # a row block of a wider tensor, read in place
        wide = torch.randn(nb, 2 * cin, 1, generator=g).cuda()
        assert torch.equal(hip_ops.pw_forward_vec_ln(h, cout, wide[:, cin:]), hip_ops.pw_forward_vec(h, cout, wide[:, cin:].contiguous())), nb


def test_pw_forward_vec_ln_constant_row_and_refusals():
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    _lib.set_precision("f16x3")
    cin, cout = 1024, 1025
    h, w, b = _pw_handle(cin, cout, "f16x3")
    g = _gen("const")
    x = torch.randn(3, cin, 1, generator=g)
    x[1] = 0.7                                                   # variance 0
    lg, lb = (1.0 + 0.2 * torch.randn(cin, generator=g)).cuda(), (0.2 * torch.randn(cin, generator=g)).cuda()
    y = hip_ops.pw_forward_vec_ln(h, cout, x.cuda(), lg, lb, 1e-5)
    assert bool(torch.isfinite(y).all())
    big, _, _ = _pw_handle(4160, 64, "f16x3")
    L, INV = _lib.lib(), _lib.AMP_ERR_INVALID
    xd, yd = x.cuda(), torch.empty(3, cout, 1, device="cuda")
    nbytes = L.amp_pw_forward_vec_ln_workspace_bytes(h, 3)
    assert nbytes == L.amp_pw_forward_vec_workspace_bytes(h, 3) > 0 and L.amp_pw_forward_vec_ln_workspace_bytes(h, 9) == 0
    ws = torch.empty(nbytes // 4, device="cuda")
    p, st = _lib.ptr, _lib.current_stream_ptr(xd.device)
    ones = torch.ones(cout, device="cuda")
    xb = torch.randn(1, 4160, 1, generator=g).cuda()
    ok = dict(h=h, x=p(xd), xbs=0, B=3, lg=p(lg), lb=p(lb), eps=1e-5, relu=0, gamma=None, res=None, y=p(yd), ws=p(ws), wsb=nbytes)
    for kw in (dict(B=0), dict(B=9), dict(lb=None), dict(lg=None), dict(eps=-1.0), dict(eps=float("nan")), dict(gamma=p(ones)), dict(res=p(yd)),
               dict(gamma=p(ones), res=p(yd), relu=1), dict(xbs=100), dict(wsb=nbytes - 4), dict(ws=None), dict(y=p(xd)), dict(ws=p(yd)), dict(x=None),
               dict(h=big, x=p(xb), B=1, wsb=1 << 20)):
        a = dict(ok)
        a.update(kw)
        rc = L.amp_pw_forward_vec_ln(a["h"], a["x"], a["xbs"], a["B"], a["lg"], a["lb"], a["eps"], a["relu"], a["gamma"], a["res"], a["y"], a["ws"],
                                     a["wsb"], st)
        assert rc == INV, kw
        assert b"amp_pw_forward_vec_ln" in L.amp_last_error(), kw
    with pytest.raises(ValueError, match="come together"):
        hip_ops.pw_forward_vec_ln(h, cout, xd, lg)
    with pytest.raises(ValueError, match="residual"):
        hip_ops.pw_forward_vec_ln(h, cout, xd, res=yd)
    torch.cuda.synchronize()


# ---- amp_embed_pos --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [72, 128])
def test_embed_pos_is_torch_bit_for_bit(D):
    from amphion_amd.modules import hip_ops
    from amphion_amd.modules.transformer.position_embedding import sine_table

    rows = 40
    g = _gen("embed", D)
    w = torch.randn(rows, D, generator=g)
    pe = sine_table(64, D)
    assert torch.equal(pe, V.sine_pe(64, D, torch.float32, "cpu"))
    for T in (1, 7, 45):
        for pos0 in (0, 5):
            for alpha, x_scale in ((0.8125, 1.0), (1.37, math.sqrt(D))):
                tok = torch.randint(0, rows, (B, T), generator=g)
                a = torch.tensor([alpha])
                want = (w[tok] * x_scale + a * pe[None, pos0:pos0 + T]).transpose(1, 2)
                got = hip_ops.embed_pos(tok.cuda(), w.cuda(), pe.cuda(), pos0, a.cuda(), x_scale)
                assert got.shape == (B, D, T) and got.is_contiguous() and torch.equal(got.cpu(), want), (T, pos0, alpha)


def test_embed_pos_flags_a_bad_id_and_refuses():
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    g = _gen("embedbad")
    w, pe, a = torch.randn(10, 64, generator=g).cuda(), torch.randn(20, 64, generator=g).cuda(), torch.tensor([0.5]).cuda()
    for bad in (10, -1):
        tok = torch.randint(0, 10, (B, 6), generator=g)
        tok[1, 3] = bad
        with pytest.raises(_lib.AmpError):
            hip_ops.embed_pos(tok.cuda(), w, pe, 0, a)
        y = hip_ops.embed_pos(tok.cuda(), w, pe, 0, a, check=False)            # the flagged column reads row 0: in bounds
        with pytest.raises(_lib.AmpError):
            hip_ops.embed_sum_check(y.device)
        assert torch.equal(y[1, :, 3], w[0] * 1.0 + a * pe[3])
    tok = torch.randint(0, 10, (B, 6), generator=g).cuda()
    hip_ops.embed_pos(tok, w, pe, 14, a)                                      # the last rows of the table
    for pos0 in (15, -1):
        with pytest.raises(ValueError, match="positions"):
            hip_ops.embed_pos(tok, w, pe, pos0, a)
    with pytest.raises(ValueError, match="tokens"):
        hip_ops.embed_pos(tok.float(), w, pe, 0, a)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
_models = {}


def _model(name):
    """(hp, sd, model on the device, inputs, keywords) of a golden run, or of the continual model"""
    from amphion_amd.models.tts.valle import VALLE

    if name not in _models:
        if name == "continual":
            hp = V.make_hp(**CONTINUAL_HP)
            sd = V.synth_state_dict(hp, int(np.load(os.path.join(GOLDEN, "golden_valle.npz"))["continual_sd_seed"]))
            inputs, kw = V.synth_inputs(hp, IN_SEED, CONTINUAL_TEXT, CONTINUAL_FRAMES), {}
        else:
            over, text_len, kw, _ = RUNS[name]
            hp = V.make_hp(**over)
            sd = V.synth_state_dict(hp, SD_SEED)
            inputs = V.synth_inputs(hp, IN_SEED, text_len)
        model = VALLE(SimpleNamespace(**hp))
        missing, unexpected = model.load_state_dict(sd)
        assert not missing and not unexpected
        _models[name] = (hp, sd, model.cuda(), inputs, kw)
    return _models[name]


@pytest.mark.parametrize("name", sorted(RUNS))
def test_inference_reproduces_the_golden(name, gold, conv_precision):
    """every stored run, token for token on all quantizer levels, with the stored draws as the noise; the two stopping modes return the
    golden's lengths"""
    hp, sd, model, (x, x_lens, y, enroll), kw = _model(name)
    q, want = torch.from_numpy(gold[f"inf_{name}_q"]), gold[f"inf_{name}_codes"]
    codes = model.inference(x.cuda(), x_lens, y.cuda(), enroll, noise=V.Replay(q), **kw)
    print(f"inference {name} {conv_precision}: {codes.shape[1]} frames, golden {want.shape[1]}")
    assert codes.dtype == torch.int64 and codes.shape == want.shape and codes.cpu().tolist() == want.tolist()
    n = want.shape[1] + int(hp["prepend_bos"])
    assert (n == 16 * x.shape[1] + 1) if RUNS[name][3] == "cap" else (n <= 16 * x.shape[1])


def test_inference_from_the_existing_launches_reproduces_the_golden(gold):
    """the AR stage with the decode step composed of amp_layer_norm_c at T = 1, amp_pw_forward_vec and a separate ReLU (the comparison route
    of tools/valle_bench.py) returns the golden's level-0 tokens"""
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    hp, sd, model, (x, x_lens, y, enroll), kw = _model("eos")
    q, want = torch.from_numpy(gold["inf_eos_q"]), torch.from_numpy(gold["inf_eos_codes"])
    y0 = y.cuda()[..., 0]
    with torch.no_grad():
        out = model._ar_generate(x.cuda(), y0, y0.shape[1], kw["top_k"], kw["temperature"], noise=V.Replay(q), fused=False)
    assert torch.equal(out.cpu(), torch.cat([y[..., 0], want[..., 0]], dim=1))


@pytest.mark.parametrize("name", ["eos", "bos", "cap"])
def test_inference_step_logits(name, gold, conv_precision):
    """teacher-forced on the golden's tokens, every step's logits are within the bound of the fp64 RECOMPUTING restatement's"""
    hp, sd, model, (x, x_lens, y, enroll), kw = _model(name)
    q, teacher = torch.from_numpy(gold[f"inf_{name}_q"]), torch.from_numpy(gold[f"inf_{name}_codes"])
    r32, r64 = [], []
    V.inference(sd, hp, x, x_lens, y, enroll, V.Replay(q), path="recompute", teacher=teacher, record=r32, **kw)
    V.inference(V.cast(sd, torch.float64), hp, x, x_lens, y, enroll, V.Replay(q), path="recompute", teacher=teacher, record=r64, **kw)
    ref = torch.stack([r["logits"] for r in r64 if "logits" in r])
    steps = []
    model.inference(x.cuda(), x_lens, y.cuda(), enroll, noise=V.Replay(q), step_logits=steps, teacher=teacher[0, :, 0].tolist(), **kw)
    assert len(steps) == ref.shape[0] == teacher.shape[1] + 1
    e32, bound = _bound(torch.stack([r["logits"] for r in r32 if "logits" in r]), ref)
    per_step = (torch.stack(steps).double().cpu() - ref).abs().amax(1)
    print(f"step logits {name} {conv_precision}: {len(steps)} steps, gpu max {float(per_step.max()):.3e} (step {int(per_step.argmax())}), first "
          f"{float(per_step[0]):.3e}, cpu32 {e32:.3e} bound {bound:.3e}")
    assert float(per_step.max()) <= bound


def test_continual_reproduces_the_golden(gold, conv_precision):
    hp, sd, model, (x, x_lens, y, _), _ = _model("continual")
    codes = model.continual(x.cuda(), x_lens, y.cuda())
    assert codes.shape == (1, CONTINUAL_FRAMES - CONTINUAL_FRAMES // 2, 8) and codes.cpu().tolist() == gold["continual_codes"].tolist()


def test_inference_draws_its_noise_and_checks_arguments(gold):
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    hp, sd, model, (x, x_lens, y, enroll), kw = _model("eos")
    for seed in range(5, 15):                                        # (a draw of EOS at the very first step is the reference's SyntaxError)
        try:
            torch.manual_seed(seed)
            a = model.inference(x.cuda(), x_lens, y.cuda(), enroll, top_k=10, temperature=0.9)
            break
        except SyntaxError:
            continue
    torch.manual_seed(seed)
    b = model.inference(x.cuda(), x_lens, y.cuda(), enroll, top_k=10, temperature=0.9)
    assert torch.equal(a, b) and 1 <= a.shape[1] <= 16 * x.shape[1] + 1 and a.shape[2] == 4 and int(a.max()) < hp["audio_token_num"]
    # the very first step stops: the sample is EOS because its noise is next to nothing
    V_, EOS = hp["audio_token_num"] + 1, hp["audio_token_num"]

    def eos_wins(shape):
        n = torch.ones(shape)
        n[..., EOS] = 1e-30
        return n
    with pytest.raises(SyntaxError):
        model.inference(x.cuda(), x_lens, y.cuda(), enroll, noise=eos_wins)
    with pytest.raises(RuntimeError, match="is on cpu"):
        model.inference(x, x_lens, y.cuda(), enroll)
    with pytest.raises(ValueError, match="unpadded"):
        model.inference(x.cuda(), x_lens - 1, y.cuda(), enroll)
    with pytest.raises(ValueError, match="temperature"):
        model.inference(x.cuda(), x_lens, y.cuda(), enroll, temperature=0.0)
    with open(os.path.join(GOLDEN, "keys_valle.json")) as f:
        assert list(model.state_dict().keys()) == V.state_dict_keys(hp) and list(sd.keys()) == V.state_dict_keys(hp) == __import__("json").load(f)
    bad = x.clone()
    bad[0, 2] = hp["text_token_num"]
    with pytest.raises(_lib.AmpError):
        model.inference(bad.cuda(), x_lens, y.cuda(), enroll, **kw)                # reported behind the prefill, before any draw
