"""Vevo's autoregressive transformer on the GPU, through module -> ctypes -> C ABI: the causal prefill attention, the KV cache and the decode
attention, the T = 1 Linear, the sampler, then ``AutoregressiveTransformer.forward`` / ``generate`` against the golden outputs of the real
class (tests/golden/make_golden_ar.py) and the fp64 restatement (tests/ar_ref.py).

Bounds.  A kernel is allowed what tests/test_gpu_fmt.py::_bound allows: 4 x the error of THE SAME FORMULA evaluated by torch in fp32 on the
CPU at the same inputs, scaled by max(1, |ref|max).  Against the golden, that bound plus the golden's own distance from fp64.  Discrete
results (token ids) must be EQUAL: their inputs are decided, every decision at least 4 tau from its boundary (ar_ref.decidedness), which the
CPU side of each test asserts.  Every test prints its figures before it asserts; DESIGN.md section 22 records them."""
import ctypes
import math
import os
import zlib

import numpy as np
import pytest
import torch

import ar_ref as A
import fmt_ref as R
from ar_ref import FWD_SEED, GEN_SEED, MAX_LENGTH, MIN_NEW, RUNS, SD_SEED

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, H = 2, 2
LMAX = 2048


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _err(got, ref64):
    return float((got.double().cpu() - ref64).abs().max())


def _bound(cpu32, ref64):
    """4 x the fp32 CPU evaluation's error, scaled by max(1, |ref|max)"""
    e32 = float((cpu32.double() - ref64).abs().max())
    return e32, 4.0 * e32 * max(1.0, float(ref64.abs().max()))


# ---- amp_rope_attention_causal ------------------------------------------------------------------------------------------------------
def _causal_masks(T):
    out = [("none", None)]
    if T > 29:
        m = torch.ones(B, T, dtype=torch.bool)
        m[1, 29:] = False
        out.append(("tail29", m))
    if T >= 3:
        m = torch.ones(B, T, dtype=torch.bool)
        m[:, T // 2] = False
        m[0, 1:max(2, T // 3)] = False
        out.append(("hole", m))
    return out


def _causal_gpu(qkv_dev, dk, cos, sin, mask):
    from amphion_amd.modules import hip_ops

    C = H * dk
    return hip_ops.rope_attention(qkv_dev[:, :C], qkv_dev[:, C:2 * C], qkv_dev[:, 2 * C:], H, cos.cuda(), sin.cuda(),
                                  None if mask is None else mask.cuda(), causal=True)


@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200])
@pytest.mark.parametrize("dk", [64, 96])
def test_causal_attention_vs_fp64(dk, T):
    """q | k | v are strided views of one [B, 3 H dk, T] tensor; masked K / V columns hold 1e30.  T = 1 is the copy of v: bound 0."""
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    C = H * dk
    cos, sin = R.rope_cos_sin(T, dk)
    fails = []
    for name, mask in _causal_masks(T):
        qkv = torch.randn(B, 3 * C, T, generator=_gen("causal", dk, T))
        q64, k64, v64 = (t.double() for t in qkv.split(C, 1))
        if mask is not None:
            bad = (~mask)[:, None, :].expand(B, 2 * C, T)
            qkv[:, C:][bad] = 1e30
        ref = A.causal_attention_cf(q64, k64, v64, H, cos.double(), sin.double(), mask)
        cpu = A.causal_attention_cf(q64.float(), k64.float(), v64.float(), H, cos, sin, mask)
        got = _causal_gpu(qkv.cuda(), dk, cos, sin, mask)
        e32, bound = _bound(cpu, ref)
        e = _err(got, ref)
        print(f"causal attention dk={dk} T={T} mask={name}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
        assert got.shape == (B, C, T) and bool(torch.isfinite(got).all())
        if not e <= bound:
            fails.append((name, e, bound))
        _lib.range_check()
    assert not fails, fails


@pytest.mark.parametrize("dk", [64, 96])
def test_causal_attention_ignores_the_future_bit_for_bit(dk):
    """q, k and v in columns > i replaced by other finite values: output columns <= i keep their bits"""
    T, C = 200, H * dk
    cos, sin = R.rope_cos_sin(T, dk)
    qkv = torch.randn(B, 3 * C, T, generator=_gen("future", dk))
    base = _causal_gpu(qkv.cuda(), dk, cos, sin, None).cpu()
    other = 3.0 * torch.randn(B, 3 * C, T, generator=_gen("future2", dk)) + 1.0
    for i in (0, 31, 32, 64, T - 2):
        x = qkv.clone()
        x[:, :, i + 1:] = other[:, :, i + 1:]
        got = _causal_gpu(x.cuda(), dk, cos, sin, None).cpu()
        assert torch.equal(got[:, :, :i + 1], base[:, :, :i + 1]), i
        assert not torch.equal(got[:, :, i + 1:], base[:, :, i + 1:]), i


# ---- amp_kv_append, amp_attention_decode ----------------------------------------------------------------------------------------------
def _rope_cf(k, cos, sin, pos0):
    """k [B, H dk, T] at positions pos0 .. -> rotated, same layout"""
    Bk, C, T = k.shape
    dk = C // H
    x = k.reshape(Bk, H, dk, T).transpose(2, 3)
    return R.apply_rope(x, cos[pos0:pos0 + T].to(k.dtype), sin[pos0:pos0 + T].to(k.dtype)).transpose(2, 3).reshape(Bk, C, T)


@pytest.mark.parametrize("dk", [64, 96])
def test_kv_append(dk):
    from amphion_amd.modules import hip_ops

    C, Lmax = H * dk, 160
    cos, sin = R.rope_cos_sin(Lmax, dk)
    fails = []
    for pos0 in (0, 1, 63, 64):
        for T in (1, 5, 64, 65):
            qkv = torch.randn(B, 3 * C, T, generator=_gen("append", dk, pos0, T))
            k, v = qkv[:, C:2 * C], qkv[:, 2 * C:]
            kc, vc = hip_ops.kv_cache(B, H, dk, Lmax, "cuda")
            kc.fill_(7.0)
            vc.fill_(-7.0)
            d = qkv.cuda()
            hip_ops.kv_append(d[:, C:2 * C], d[:, 2 * C:], H, cos.cuda(), sin.cuda(), pos0, kc, vc)
            kc, vc = kc.cpu(), vc.cpu()
            assert torch.equal(vc[:, :, pos0:pos0 + T], v), (pos0, T)
            keep = torch.ones(Lmax, dtype=torch.bool)
            keep[pos0:pos0 + T] = False
            assert bool((kc[:, :, keep] == 7.0).all()) and bool((vc[:, :, keep] == -7.0).all()), (pos0, T)
            ref = _rope_cf(k.double(), cos.double(), sin.double(), pos0)
            e32, bound = _bound(_rope_cf(k, cos, sin, pos0), ref)
            e = _err(kc[:, :, pos0:pos0 + T], ref)
            print(f"kv_append dk={dk} pos0={pos0} T={T}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
            if not e <= bound:
                fails.append((pos0, T, e, bound))
    assert not fails, fails


def _decode_ref(q, kc, vc, cos, sin, L, dk):
    """q [B, C] un-rotated at position L - 1, caches [B, C, >= L] (K rotated) -> [B, C]"""
    Bq, C = q.shape
    qr = _rope_cf(q[:, :, None], cos, sin, L - 1).reshape(Bq, H, dk)
    k = kc[:, :, :L].reshape(Bq, H, dk, L)
    v = vc[:, :, :L].reshape(Bq, H, dk, L)
    p = torch.softmax(torch.einsum("bhd,bhdl->bhl", qr, k) / math.sqrt(dk), -1)
    return torch.einsum("bhl,bhdl->bhd", p, v).reshape(Bq, C)


@pytest.mark.parametrize("dk", [64, 96])
def test_attention_decode(dk):
    """every L around the key split; the cache beyond L holds NaN, then 1e30: finite and the same bits"""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    S = _lib.lib().amp_attention_decode_split()
    C = H * dk
    cos, sin = R.rope_cos_sin(LMAX, dk)
    g = _gen("decode", dk)
    kfull, vfull = torch.randn(B, C, LMAX, generator=g), torch.randn(B, C, LMAX, generator=g)
    fails = []
    for L in (1, 2, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1, 2047):
        q = 2.0 * torch.randn(B, 3 * C, 1, generator=g)
        outs = []
        for fill in (float("nan"), 1e30):
            kc, vc = kfull.clone(), vfull.clone()
            kc[:, :, L:] = fill
            vc[:, :, L:] = fill
            outs.append(hip_ops.attention_decode(q.cuda()[:, :C], H, cos.cuda(), sin.cuda(), L, kc.cuda(), vc.cuda()).cpu())
        assert outs[0].shape == (B, C, 1) and bool(torch.isfinite(outs[0]).all()), L
        assert torch.equal(outs[0], outs[1]), L
        q1 = q[:, :C, 0]
        ref = _decode_ref(q1.double(), kfull.double(), vfull.double(), cos.double(), sin.double(), L, dk)
        e32, bound = _bound(_decode_ref(q1, kfull, vfull, cos, sin, L, dk), ref)
        e = _err(outs[0][:, :, 0], ref)
        print(f"attention_decode dk={dk} L={L}: gpu {e:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
        if not e <= bound:
            fails.append((L, e, bound))
    assert not fails, fails


@pytest.mark.parametrize("dk", [64, 96])
def test_prefill_plus_decode_is_one_causal_prefill(dk):
    """70 tokens: a causal prefill of 40 that fills the cache, then 30 decode steps, against the fp64 causal attention over all 70"""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    _lib.set_precision("f16x3")
    T, T0, C = 70, 40, H * dk
    cos, sin = R.rope_cos_sin(T, dk)
    qkv = torch.randn(B, 3 * C, T, generator=_gen("consistency", dk))
    q64, k64, v64 = (t.double() for t in qkv.split(C, 1))
    ref = A.causal_attention_cf(q64, k64, v64, H, cos.double(), sin.double())
    cpu = A.causal_attention_cf(q64.float(), k64.float(), v64.float(), H, cos, sin)
    d, cd, sd_ = qkv.cuda(), cos.cuda(), sin.cuda()
    kc, vc = hip_ops.kv_cache(B, H, dk, T + 3, "cuda")
    kc.fill_(float("nan"))
    vc.fill_(float("nan"))
    head = d[:, :, :T0].contiguous()
    cols = [_causal_gpu(head, dk, cos[:T0], sin[:T0], None)]
    hip_ops.kv_append(head[:, C:2 * C], head[:, 2 * C:], H, cd, sd_, 0, kc, vc)
    for t in range(T0, T):
        col = d[:, :, t:t + 1].contiguous()
        hip_ops.kv_append(col[:, C:2 * C], col[:, 2 * C:], H, cd, sd_, t, kc, vc)
        cols.append(hip_ops.attention_decode(col[:, :C], H, cd, sd_, t + 1, kc, vc))
    got = torch.cat(cols, 2)
    e32, bound = _bound(cpu, ref)
    e_pre, e_dec = _err(got[:, :, :T0], ref[:, :, :T0]), _err(got[:, :, T0:], ref[:, :, T0:])
    print(f"prefill {T0} + {T - T0} steps dk={dk}: prefill {e_pre:.3e} decode {e_dec:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
    assert e_pre <= bound and e_dec <= bound


# ---- amp_pw_forward_vec ---------------------------------------------------------------------------------------------------------------
_handles = {}


def _pw_handle(cin, cout, precision):
    from amphion_amd import _lib

    key = (cin, cout, precision)
    if key not in _handles:
        g = _gen("pw", cin, cout)
        w = (torch.randn(cout, cin, generator=g) / math.sqrt(cin)).contiguous()
        b = torch.randn(cout, generator=g).contiguous()
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().amp_pw_create(cin, cout, _lib.ptr(w), _lib.ptr(b), ctypes.byref(h)))
        _handles[key] = (h, w, b)
    return _handles[key]


@pytest.mark.parametrize("shape", [(192, 192, False), (192, 576, False), (192, 512, False), (256, 192, True), (192, 150, False), (1536, 9268, False),
                                   (1, 40, True)], ids=lambda s: f"{s[0]}x{s[1]}{'res' if s[2] else ''}")
def test_pw_forward_vec(shape, conv_precision):
    """within the bound of fp64, and within the same bound of amp_pw_forward at T = 1 on the same handle; Cin = 1 is the smallest
    amp_pw_create accepts"""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    cin, cout, with_res = shape
    h, w, b = _pw_handle(cin, cout, conv_precision)
    L = _lib.lib()
    assert L.amp_pw_precision(h) == _lib.PRECISIONS[conv_precision]
    fails = []
    for nb in (1, 3):
        g = _gen("pwx", cin, cout, nb)
        x = torch.randn(nb, cin, 1, generator=g)
        res = torch.randn(nb, cout, 1, generator=g) if with_res else None
        gamma = (1.0 + 0.5 * torch.randn(cout, generator=g)) if with_res else None

        def f(dt):
            y = torch.nn.functional.linear(x[:, :, 0].to(dt), w.to(dt), b.to(dt))
            return (res[:, :, 0].to(dt) + gamma.to(dt) * y) if with_res else y
        ref, cpu = f(torch.float64), f(torch.float32)
        xd = x.cuda()
        rd, gd = (res.cuda(), gamma.cuda()) if with_res else (None, None)
        got = hip_ops.pw_forward_vec(h, cout, xd, gamma=gd, res=rd)
        gemm = torch.empty((nb, cout, 1), dtype=torch.float32, device="cuda")
        _lib.check(L.amp_pw_forward(h, _lib.ptr(xd), 0, nb, 1, 2 if with_res else 0, _lib.ptr(gd), _lib.ptr(rd), _lib.ptr(gemm),
                                    _lib.current_stream_ptr(xd.device)))
        e32, bound = _bound(cpu, ref)
        e, eg = _err(got[:, :, 0], ref), _err(gemm[:, :, 0], ref)
        d = float((got - gemm).abs().max())
        print(f"pw_forward_vec {cin}->{cout} B={nb} {conv_precision}: vec {e:.3e} gemm {eg:.3e} vec-gemm {d:.3e} cpu32 {e32:.3e} bound {bound:.3e}")
        assert got.shape == (nb, cout, 1)
        if not (e <= bound and d <= bound):
            fails.append((nb, e, d, bound))
        # y aliasing res
        if with_res:
            y = rd.clone()
            hip_ops.pw_forward_vec(h, cout, xd, gamma=gd, res=y, out=y)
            assert torch.equal(y, got)
    assert not fails, fails


def test_pw_forward_vec_is_deterministic_and_refuses():
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    _lib.set_precision("f16x3")
    h, w, b = _pw_handle(192, 576, "f16x3")
    x = torch.randn(3, 192, 1, generator=_gen("det")).cuda()
    a = hip_ops.pw_forward_vec(h, 576, x)
    assert all(torch.equal(a, hip_ops.pw_forward_vec(h, 576, x)) for _ in range(3))
    L, INV = _lib.lib(), _lib.AMP_ERR_INVALID
    y = torch.empty(3, 576, 1, device="cuda")
    nbytes = L.amp_pw_forward_vec_workspace_bytes(h, 3)
    ws = torch.empty(nbytes // 4, device="cuda")
    p, st = _lib.ptr, _lib.current_stream_ptr(x.device)
    assert nbytes > 0 and L.amp_pw_forward_vec_workspace_bytes(h, 9) == 0
    for args in ((h, p(x), 0, 0, 0, None, None, p(y), p(ws), nbytes, st), (h, p(x), 0, 9, 0, None, None, p(y), p(ws), nbytes, st),
                 (h, p(x), 0, 3, 1, None, None, p(y), p(ws), nbytes, st), (h, p(x), 0, 3, 2, None, None, p(y), p(ws), nbytes, st),
                 (h, p(x), 100, 3, 0, None, None, p(y), p(ws), nbytes, st), (h, p(x), 0, 3, 0, None, None, p(y), p(ws), nbytes - 4, st),
                 (h, p(x), 0, 3, 0, None, None, p(y), None, nbytes, st), (h, p(x), 0, 3, 0, None, None, p(x), p(ws), nbytes, st),
                 (h, p(x), 0, 3, 0, None, None, p(y), p(y), nbytes, st)):
        assert L.amp_pw_forward_vec(*args) == INV, args[2:6]
        assert b"amp_pw_forward_vec" in L.amp_last_error()
    torch.cuda.synchronize()


# ---- amp_ar_sample --------------------------------------------------------------------------------------------------------------------
def _sample_case(V, k, top_p, temperature, penalty, suppress, seed=0, eos=None):
    """Decided inputs: by rank r from the top the logits are 1.525 - 0.05 r for r < 64 (no logit within 0.025 of zero or of another: the
    top-k boundary at k = 50 and the penalty's sign test are far from their edges, and the mass sits there) and -20 - 0.001 (r - 64) below
    (a tail of up to 16320 values whose whole mass is below 1e-5), at permuted positions; the race and the top-p cut are checked like the
    rest.  -> (logits [V], q [V], history [n], eos, expected id, tau, gap)"""
    g = _gen("sample", V, seed)
    rank = torch.randperm(V, generator=g).float()
    logits = torch.where(rank < 64, 1.525 - 0.05 * rank, -20.0 - 0.001 * (rank - 64)).contiguous()
    q = torch.empty(V).exponential_(generator=g)
    top = torch.argsort(logits, descending=True)
    eos = int(top[0]) if eos is None else eos                    # suppressing the largest changes the winner's field
    pool = torch.cat((top[:6], top[-4:], top[V // 2:V // 2 + 2]))[:max(2, min(12, V))]     # logits of both signs
    hist = torch.cat((pool, pool[:3], pool[:1]))                 # ids repeat
    kw = dict(repetition_penalty=penalty, eos=eos, suppress_eos=suppress, temperature=temperature, top_k=k, top_p=top_p)
    gaps = {}
    l64 = A.process(logits.double(), hist, gaps=gaps, **kw)
    l32 = A.process(logits, hist, **kw)
    assert torch.equal(torch.isfinite(l32), torch.isfinite(l64))
    fin = torch.isfinite(l64)
    tau = float((l32.double()[fin] - l64[fin]).abs().max())
    want = A.race(l64, q.double(), gaps)
    assert want == A.race(l32, q)
    return logits, q, hist, eos, want, tau, min(gaps.values())


@pytest.mark.parametrize("V", [2, 64, 65, 150, 9268, 16384])
def test_ar_sample(V):
    """k in {1, 50, V, V + 7} x top_p in {1e-6, 0.9, 1.0} x temperature in {0.8, 1.0} x penalty in {1.0, 1.1} x EOS suppressed or not: the
    ids equal the restatement's; every case is decided (gap >= 4 tau), asserted here on the CPU side"""
    from amphion_amd.modules import hip_ops

    worst, n, bad = float("inf"), 0, []
    for k in (1, 50, V, V + 7):
        for top_p in (1e-6, 0.9, 1.0):
            for temperature in (0.8, 1.0):
                for penalty in (1.0, 1.1):
                    for suppress in (False, True):
                        rows = [_sample_case(V, k, top_p, temperature, penalty, suppress, 0)]
                        rows.append(_sample_case(V, k, top_p, temperature, penalty, suppress, 1, eos=rows[0][3]))
                        for logits, q, hist, eos, want, tau, gap in rows:
                            assert gap >= 4 * tau and gap > 0, (k, top_p, temperature, penalty, suppress, gap, tau)
                            worst = min(worst, gap / tau if tau else float("inf"))
                        # two rows in one launch: row 1's logits, noise and history differ; they share n, eos and the settings
                        eos = rows[0][3]
                        nh = len(rows[0][2])
                        ids = torch.full((len(rows), nh + 2), -1, dtype=torch.int64)
                        for r, row in enumerate(rows):
                            ids[r, :nh] = row[2]
                        lg = torch.stack([row[0] for row in rows])[:, :, None].cuda()
                        qd = torch.stack([row[1] for row in rows]).cuda()
                        out = hip_ops.ar_sample(lg, qd, ids.cuda(), nh, eos, suppress, temperature, k, top_p, penalty).cpu()
                        assert torch.equal(out[:, :nh], ids[:, :nh]) and bool((out[:, nh + 1] == -1).all())
                        for r, row in enumerate(rows):
                            n += 1
                            if int(out[r, nh]) != row[4]:
                                bad.append((k, top_p, temperature, penalty, suppress, r, int(out[r, nh]), row[4]))
    print(f"ar_sample V={V}: {n} rows, smallest gap {worst:.1f} tau, {len(bad)} differ")
    assert not bad, bad[:8]


def test_ar_sample_ties():
    from amphion_amd.modules import hip_ops

    V = 64
    # four equal logits straddle the k-th place (k = 3: ranks 3 .. 6 are equal): HF removes l < the k-th value, so all four stay -- the
    # noise makes the LAST of them win, which a sampler that keeps k entries would have dropped
    logits = torch.linspace(-3.0, -1.0, V)
    logits[[5, 50]] = torch.tensor([4.0, 3.5])
    tied = [7, 20, 33, 61]
    logits[tied] = 3.0
    q = torch.ones(V)
    q[61] = 1e-3
    ids = torch.zeros((1, 4), dtype=torch.int64)
    want = A.race(A.process(logits.double(), ids[0, :0], top_k=3, top_p=1.0), q.double())
    assert want == 61
    out = hip_ops.ar_sample(logits[None, :, None].cuda(), q[None].cuda(), ids.cuda(), 0, 0, False, 1.0, 3, 1.0, 1.0)
    assert int(out[0, 0]) == 61
    # the same with top_p: the four tied and the two above hold all the mass
    out = hip_ops.ar_sample(logits[None, :, None].cuda(), q[None].cuda(), ids.cuda(), 0, 0, False, 1.0, 3, 0.999, 1.0)
    assert int(out[0, 0]) == A.race(A.process(logits.double(), ids[0, :0], top_k=3, top_p=0.999), q.double()) == 61
    # equal race values: the lower index wins
    logits = torch.linspace(-3.0, -1.0, V)
    logits[[40, 10]] = 2.0
    q = torch.full((V,), 5.0)
    q[[40, 10]] = 0.5
    assert A.race(A.process(logits, ids[0, :0], top_k=50, top_p=1.0), q) == 10
    out = hip_ops.ar_sample(logits[None, :, None].cuda(), q[None].cuda(), ids.cuda(), 1, 0, False, 1.0, 50, 1.0, 1.0)
    assert int(out[0, 1]) == 10


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_ar.npz"))


_models = {}


def _model(dk):
    """one module per head dimension; its handles follow the precision"""
    from amphion_amd.models.vc.autoregressive_transformer import AutoregressiveTransformer

    if dk not in _models:
        hp = A.small_hp(dk)
        sd = A.synth_state_dict(hp, SD_SEED)
        m = AutoregressiveTransformer(**hp).eval()
        old = dict(sd)
        for i in range(hp["num_hidden_layers"]):                 # a checkpoint that carries the rotary buffers
            old[f"model.model.layers.{i}.self_attn.rotary_emb.inv_freq"] = torch.zeros(dk // 2)
        m.load_state_dict(old)
        _models[dk] = (hp, sd, A.cast(sd, torch.float64), m.cuda())
    return _models[dk]


_fwd_refs = {}


def _forward_refs(dk):
    if dk not in _fwd_refs:
        hp, sd, sd64, _ = _model(dk)
        inputs = A.synth_forward_inputs(hp, FWD_SEED)
        _fwd_refs[dk] = (inputs, A.forward(sd, hp, *inputs), A.forward(sd64, hp, *inputs))
    return _fwd_refs[dk]


@pytest.mark.parametrize("dk", [96, 64])
def test_forward(dk, gold, conv_precision):
    hp, sd, sd64, model = _model(dk)
    inputs, (l32, loss32), (l64, loss64) = _forward_refs(dk)
    out = model(*(t.cuda() for t in inputs))
    g = torch.from_numpy(gold[f"fwd_logits_{dk}"])
    e32, bound = _bound(l32, l64)
    eg = float((g.double() - l64).abs().max())
    e, e_gold = _err(out.logits, l64), _err(out.logits, g.double())
    print(f"forward dk={dk} {conv_precision}: gpu {e:.3e} from fp64, {e_gold:.3e} from the golden; cpu32 {e32:.3e} golden {eg:.3e} bound {bound:.3e}")
    assert out.logits.shape == g.shape
    assert e <= bound and e_gold <= bound + eg
    el32 = max(abs(float(loss32) - float(loss64)), float(np.spacing(np.float32(loss64))))
    lb = 4 * el32 * max(1.0, abs(float(loss64)))
    el, elg = abs(float(out.loss) - float(loss64)), abs(float(out.loss) - float(gold[f"fwd_loss_{dk}"]))
    print(f"loss {float(out.loss):.6f}: gpu {el:.3e} from fp64, {elg:.3e} from the golden; bound {lb:.3e}")
    assert el <= lb and elg <= lb + abs(float(gold[f"fwd_loss_{dk}"]) - float(loss64))


@pytest.mark.parametrize("name", sorted(RUNS))
def test_generate_reproduces_the_golden(name, gold, conv_precision):
    """every stored run, token for token, with the stored draws as the noise; the two stopping modes return the golden's lengths"""
    dk, kw, end = RUNS[name]
    hp, sd, sd64, model = _model(dk)
    ii, po = A.synth_generate_inputs(hp, GEN_SEED)
    q = torch.from_numpy(gold[f"gen_{name}_q"])
    gen = model.generate(ii.cuda(), prompt_output_ids=po.cuda(), max_length=MAX_LENGTH, min_new_tokens=MIN_NEW, noise=A.Replay(q), **kw)
    want = gold[f"gen_{name}_tokens"]
    print(f"generate {name} {conv_precision}: {gen.shape[1]} tokens, golden {want.shape[1]}")
    assert gen.dtype == torch.int64 and gen.cpu().tolist() == want.tolist()
    raw = gold[f"gen_{name}_raw"]
    if end == "eos":
        assert gen.shape[1] == len(raw) - 1 and ii.shape[1] + po.shape[1] + 3 + len(raw) < MAX_LENGTH
    if end == "max":
        assert gen.shape[1] == len(raw) == MAX_LENGTH - (ii.shape[1] + po.shape[1] + 3)


@pytest.mark.parametrize("name", ["eos96", "pen64"])
def test_generate_step_logits(name, gold, conv_precision):
    """teacher-forced on the golden's tokens, every step's logits are within the bound of the fp64 restatement's"""
    dk, kw, end = RUNS[name]
    hp, sd, sd64, model = _model(dk)
    ii, po = A.synth_generate_inputs(hp, GEN_SEED)
    q = torch.from_numpy(gold[f"gen_{name}_q"])
    raw = gold[f"gen_{name}_raw"].tolist()
    r32, r64 = [], []
    A.generate(sd, hp, ii, po, A.Replay(q), max_length=MAX_LENGTH, min_new_tokens=MIN_NEW, teacher=raw, record=r32, **kw)
    A.generate(sd64, hp, ii, po, A.Replay(q), max_length=MAX_LENGTH, min_new_tokens=MIN_NEW, teacher=raw, record=r64, **kw)
    steps = []
    model.generate(ii.cuda(), prompt_output_ids=po.cuda(), max_length=MAX_LENGTH, min_new_tokens=MIN_NEW, noise=A.Replay(q), step_logits=steps,
                   teacher=raw, **kw)
    assert len(steps) == len(r64) == len(raw)
    ref = torch.stack([r["logits"] for r in r64])
    e32, bound = _bound(torch.stack([r["logits"] for r in r32]), ref)
    per_step = (torch.stack(steps).double().cpu() - ref).abs().amax(1)
    print(f"step logits {name} {conv_precision}: {len(steps)} steps, gpu max {float(per_step.max()):.3e} (step {int(per_step.argmax())}), first "
          f"{float(per_step[0]):.3e}, cpu32 {e32:.3e} bound {bound:.3e}")
    assert float(per_step.max()) <= bound


def test_generate_draws_its_noise_and_checks_arguments():
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    hp, sd, sd64, model = _model(64)
    ii, po = A.synth_generate_inputs(hp, GEN_SEED)
    torch.manual_seed(5)
    a = model.generate(ii.cuda(), prompt_output_ids=po.cuda(), max_length=40, min_new_tokens=3)
    torch.manual_seed(5)
    b = model.generate(ii.cuda(), prompt_output_ids=po.cuda(), max_length=40, min_new_tokens=3)
    n0 = ii.shape[1] + po.shape[1] + 3
    assert torch.equal(a, b) and 3 <= a.shape[1] <= 40 - n0 and int(a.max()) < A.special(hp)["vocab"]
    with pytest.raises(ValueError, match="max_length"):
        model.generate(ii.cuda(), prompt_output_ids=po.cuda(), max_length=n0)
    with pytest.raises(ValueError, match="prompt_output_ids"):
        model.generate(ii.cuda())
    with pytest.raises(RuntimeError, match="is on cpu"):
        model.generate(ii, prompt_output_ids=po.cuda())
    keys = list(model.state_dict().keys())
    assert keys == A.state_dict_keys(hp) and all(torch.equal(model.state_dict()[k].cpu(), sd[k]) for k in keys)
