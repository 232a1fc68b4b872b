"""The semantic tokenizers on the MI355X (csrc/dsconv_f16x3.hip and the drop-ins of amphion_amd/models/codec/{kmeans,coco,vevo}) against the fp64
restatement of tests/tokenizer_ref.py and the golden outputs of the real reference classes.

Bounds, with e32 the fp32 restatement's own error against fp64 on the same inputs:
    amp_dsconv, per element                       2e-6 (|w| * |x| + |b|) + 3e-7 |ref|; behind the GELU 1.2 x the first term and |lin| in the second
    exact-fp32 tensors (amp_gelu, quantizers)     max(4 e32, 1e-6 max|ref64|)
    anything through an f16x3 GEMM                max(4 e32, 1e-4 max|ref64|)
Every stage is compared with fp64 run from the DEVICE's stage before it.  Quantizer codes: identical to fp64 on every DECIDED (level, frame) pair
of the margin rule computed from the device's latent; at most 2 % of the pairs may be undecided, which is asserted on the fp64 reference before
the device's codes are looked at; tensors are compared with the references FOLLOWING the kernel's codes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import codec_ref as C  # noqa: E402
import speechtokenizer_ref as S  # noqa: E402
import tokenizer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(ROOT, "tests", "golden")
UNDECIDED_CAP = 0.02


def _L():
    from amphion_amd import _lib

    return _lib


def bound(ref64, ref32, floor):
    return max(4.0 * float((ref32.double() - ref64).abs().max()), floor * float(ref64.abs().max()))


def check(name, got, ref64, ref32, floor):
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    err, tol = float((got - ref64).abs().max()), bound(ref64, ref32, floor)
    print(f"    {name}: error {err:.3g}, bound {tol:.3g} ({err / tol if tol else 0:.3f})")
    assert err <= tol, (name, err, tol)


def near_gold(name, got, g, ref64, ref32, floor):
    """the golden tensor is the reference's own fp32 evaluation: it may sit its own rounding away from fp64"""
    got, g = got.detach().cpu().double(), torch.from_numpy(g).double()
    assert got.shape == g.shape, (name, got.shape, g.shape)
    tol = bound(ref64, ref32, floor) + float((g - ref64).abs().max())
    err = float((got - g).abs().max())
    print(f"    {name} against the golden file: {err:.3g}, bound {tol:.3g}")
    assert err <= tol, (name, err, tol)


def decided_or_fail(name, decided):
    """the cap on undecided pairs, on the fp64 reference alone"""
    und = 1.0 - float(decided.double().mean())
    assert und <= UNDECIDED_CAP, (name, und)
    return und


# ---- amp_dsconv ------------------------------------------------------------------------------------------------------------------------
class DsConv:
    def __init__(self, w, b):
        _lib = _L()
        self.cout, self.cin, _ = w.shape
        self.h = ctypes.c_void_p()
        w, b = w.contiguous(), (b.contiguous() if b is not None else None)
        _lib.check(_lib.lib().amp_dsconv_create(self.cin, self.cout, _lib.ptr(w), _lib.ptr(b), ctypes.byref(self.h)))

    def __call__(self, x, gelu):
        _lib = _L()
        L = _lib.lib()
        B, _, T = x.shape
        y = torch.full((B, self.cout, L.amp_dsconv_out_len(self.h, T)), float("nan"), device=DEV)
        need = L.amp_dsconv_workspace_bytes(self.h, B, T)
        ws = torch.empty(max(1, need // 4), device=DEV)
        _lib.check(L.amp_dsconv_forward(self.h, _lib.ptr(x), B, T, int(gelu), _lib.ptr(ws) if need else None, need, _lib.ptr(y), None))
        return y

    def __del__(self):
        _L().lib().amp_dsconv_destroy(self.h)


def three_step_route(w, b, x, gelu):
    """the route available before the kernel, by hand through the public entries: zero-column copy, amp_sconv (stride 2, padding 1) with the
    weight extended by a zero fourth tap, amp_gelu"""
    _lib = _L()
    L = _lib.lib()
    cout, cin, _ = w.shape
    B, _, T = x.shape
    w4 = Fn.pad(w, (0, 1)).contiguous()
    h = ctypes.c_void_p()
    _lib.check(L.amp_sconv_create(cin, cout, 2, 1, _lib.ptr(w4), _lib.ptr(b), ctypes.byref(h)))
    xp = Fn.pad(x, (0, 1)).contiguous()
    Tout = L.amp_sconv_out_len(h, T + 1)
    need = L.amp_sconv_workspace_bytes(h, B, T + 1)
    ws = torch.empty(need // 4, device=DEV)
    y = torch.empty((B, cout, Tout), device=DEV)
    _lib.check(L.amp_sconv_forward(h, _lib.ptr(xp), B, T + 1, None, _lib.ptr(ws), need, _lib.ptr(y), None))
    if gelu:
        _lib.check(L.amp_gelu(_lib.ptr(y), y.numel(), _lib.ptr(y), None))
    torch.cuda.synchronize()
    L.amp_sconv_destroy(h)
    return y


# a .. c: 64-column tiles (T_out either side of one and of two tiles, both parities of T); d: the 128-column tile, which the launcher takes from
# 256 workgroups on (16 items x 8 column tiles x 2 row tiles), with a ragged last column tile, channel step and row tile
DS_CASES = {"a": (3, 24, 24, (1, 2, 3, 4)), "b": (2, 64, 160, (127, 128, 129, 130)), "c": (1, 100, 64, (257, 258)),
            "d": (16, 40, 130, (1793, 1794))}


@pytest.mark.parametrize("case", sorted(DS_CASES))
def test_dsconv_against_fp64(conv_precision, case):
    """random data, B >= 2 in two cases: a clamp in place of the zero select at input column -1 or T would read the neighbouring row or repeat
    the edge sample, and misses the bound"""
    _lib = _L()
    B, cin, cout, lengths = DS_CASES[case]
    g = torch.Generator().manual_seed(ord(case))
    w = torch.randn(cout, cin, 3, generator=g) / (3 * cin) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    conv = DsConv(w, b)
    nobias = DsConv(w, None)
    worst = 0.0
    for T in lengths:
        x = torch.randn(B, cin, T, generator=g)
        xd = x.to(DEV)
        for gelu in (False, True):
            ref, tol = R.dsconv_bound(w.double(), b.double(), x.double(), gelu)
            y = conv(xd, gelu)
            torch.cuda.synchronize()
            assert tuple(y.shape) == tuple(ref.shape) == (B, cout, (T - 1) // 2 + 1) and torch.isfinite(y).all()
            ratio = float(((y.cpu().double() - ref).abs() / tol.clamp_min(1e-30)).max())
            print(f"    dsconv {cin}->{cout} B={B} T={T} gelu={gelu} [{conv_precision}]: worst error / bound = {ratio:.3f}")
            worst = max(worst, ratio)
            assert ratio <= 1.0, (case, T, gelu, ratio)
            if conv_precision == "f32":
                assert torch.equal(y, three_step_route(w, b, xd, gelu)), (case, T, gelu)
        ref, tol = R.dsconv_bound(w.double(), None, x.double(), False)
        assert float(((nobias(xd, False).cpu().double() - ref).abs() / tol.clamp_min(1e-30)).max()) <= 1.0
        for i in sorted({0, 1 % B, B - 1}):               # an item's bits depend neither on what it is batched with nor on the tile width
            assert torch.equal(conv(xd[i:i + 1].contiguous(), True)[0], conv(xd, True)[i]), (case, T, i)
    _lib.range_check()
    print(f"dsconv case {case} [{conv_precision}]: worst error / bound = {worst:.3f}")


def test_dsconv_forward_refusals():
    _lib = _L()
    L, p = _lib.lib(), _lib.ptr
    conv = DsConv(torch.zeros(4, 4, 3), None)
    x = torch.zeros(2, 4, 8, device=DEV)
    y = torch.zeros(2, 4, 4, device=DEV)
    for args in ((conv.h, None, 2, 8, 0, None, 0, p(y), None), (conv.h, p(x), 2, 8, 0, None, 0, None, None), (conv.h, p(x), 0, 8, 0, None, 0, p(y), None),
                 (conv.h, p(x), 2, 0, 0, None, 0, p(y), None), (conv.h, p(x), 2, 8, 2, None, 0, p(y), None), (conv.h, p(x), 2, 8, 0, None, 0, p(x), None)):
        assert L.amp_dsconv_forward(*args) == _lib.AMP_ERR_INVALID, L.amp_last_error()
        assert b"amp_dsconv_forward" in L.amp_last_error()
    assert L.amp_dsconv_workspace_bytes(conv.h, 2, 8) == 0                 # f16x3 needs none
    _lib.set_precision("f32")
    try:
        exact = DsConv(torch.zeros(4, 4, 3), None)
    finally:
        _lib.set_precision("f16x3")
    need = L.amp_dsconv_workspace_bytes(exact.h, 2, 8)
    assert need > 0
    ws = torch.zeros(need // 4 + 8, device=DEV)
    assert L.amp_dsconv_forward(exact.h, p(x), 2, 8, 1, p(ws), need - 4, p(y), None) == _lib.AMP_ERR_INVALID
    assert L.amp_dsconv_forward(exact.h, p(x), 2, 8, 1, None, need, p(y), None) == _lib.AMP_ERR_INVALID
    assert L.amp_dsconv_forward(exact.h, p(x), 2, 8, 1, p(ws[1:]), need, p(y), None) == _lib.AMP_ERR_INVALID and b"16-byte" in L.amp_last_error()
    assert L.amp_dsconv_forward(exact.h, p(x), 2, 8, 1, p(ws), need, p(y), None) == 0
    torch.cuda.synchronize()


# ---- amp_gelu --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_gelu(n):
    _lib = _L()
    L, p = _lib.lib(), _lib.ptr
    g = torch.Generator().manual_seed(n)
    x = 3.0 * torch.randn(n, generator=g)
    ref64, ref32 = Fn.gelu(x.double()), Fn.gelu(x)
    for off in (0, 1, 3):                                 # the base 0, 4 and 12 bytes off a 16-byte boundary
        bx = torch.zeros(off + n, device=DEV)
        by = torch.full((off + n + 4,), float("nan"), device=DEV)
        xv, yv = bx[off:], by[off:off + n]
        xv.copy_(x)
        assert xv.data_ptr() % 16 == 4 * off
        _lib.check(L.amp_gelu(p(xv), n, p(yv), None))
        torch.cuda.synchronize()
        check(f"gelu n={n} off={off}", yv, ref64, ref32, 1e-6)
        assert bool(torch.isnan(by[off + n:]).all()) and bool(torch.isnan(by[:off]).all())
        out_of_place = yv.clone()
        _lib.check(L.amp_gelu(p(xv), n, p(xv), None))      # in place
        torch.cuda.synchronize()
        assert torch.equal(xv, out_of_place)
    # aligned input, unaligned output
    bx = x.to(DEV)
    by = torch.zeros(n + 1, device=DEV)
    _lib.check(L.amp_gelu(p(bx), n, p(by[1:]), None))
    torch.cuda.synchronize()
    check(f"gelu n={n} y off", by[1:], ref64, ref32, 1e-6)


# ---- the models ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_tokenizers.npz"))


@pytest.fixture(scope="module")
def nets(gold):
    return R.golden_models(int(gold["seed"]))


def build_repcodec(hp, sd):
    from amphion_amd.models.codec.kmeans.repcodec_model import RepCodec

    m = RepCodec(**hp)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def build_coco(hp, sd, cls=None, **kw):
    from amphion_amd.models.codec.coco.rep_coco_model import CocoContentStyle

    m = (cls or CocoContentStyle)(cfg=R.coco_cfg(hp), **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def build_vevo(hp, sd):
    from amphion_amd.models.codec.vevo.vevo_repcodec import VevoRepCodec

    m = VevoRepCodec(**hp)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def fvq_sure_pairs(sd, hp, z_gold, z_dev, tau):
    """the level-0 pairs on which the device must give the GOLDEN code: the fp64 margin on the golden latent covers tau and the latent's distance
    from the reference's.  The distance is taken between unit vectors enc = z_e / |z_e|, z_e = in_project(z): a difference of two distances,
    -2 enc . (c_k - c_j) with |c| = 1, moves by at most 4 |d enc| <= 8 |d z_e| / |z_e| <= 8 ||W_in||_2 |d z| / |z_e|."""
    P = {k: v.double() for k, v in sd.items()}
    W = C.folded(P, R.QP + "0.in_project.")[:, :, 0]
    z_e = torch.einsum("oc,bct->bot", W, z_gold.double()) + P[R.QP + "0.in_project.bias"][None, :, None]
    delta = (z_dev.double() - z_gold.double()).norm(dim=1)
    slack = tau + 8.0 * float(torch.linalg.matrix_norm(W, 2)) * delta / z_e.norm(dim=1)
    g64 = R.fvq(sd, hp, z_gold, torch.float64)
    return g64["margin"][0] > slack


def check_fvq_codes(name, sd, hp, z_dev, codes_dev, gold_z, gold_codes):
    """codes [N, B, T'] of the device against fp64 on the decided pairs and against the golden codes on the sure ones -> (codes on the host,
    whether they are the golden codes)"""
    zh = z_dev.detach().cpu()
    r64, _, tau, decided = R.fvq_margin_rule(sd, hp, zh)
    und = decided_or_fail(name, decided)
    ch = codes_dev.cpu()
    assert int(ch.min()) >= 0 and int(ch.max()) < hp["codebook_size"]
    assert bool((ch == r64["codes"])[decided].all()), (name, int(((ch != r64["codes"]) & decided).sum()))
    sure = fvq_sure_pairs(sd, hp, gold_z, zh, tau)
    assert bool((ch[0] == gold_codes)[sure].all()), name
    print(f"    {name}: tau = {tau:.3g}, undecided {100 * und:.2f} %, {int(sure.sum())} of {sure.numel()} pairs compared with the golden codes, "
          f"{int((ch[0] != gold_codes).sum())} differ")
    return ch, torch.equal(ch[0], gold_codes), bool(sure.all())


def golden_walk(name, same, all_sure):
    """the golden tensors behind the quantizer can be compared only where the device walked the golden codes -- and it must have, where every
    pair is sure"""
    if all_sure:
        assert same, name
    if not same:
        pytest.fail(f"{name}: codes off the golden ones on pairs the margin leaves open: the golden comparison cannot be made for this input")


@pytest.mark.parametrize("T", R.GOLDEN_LENGTHS)
@pytest.mark.parametrize("K", [64, 8192])
def test_repcodec_vs_fp64_and_golden(conv_precision, gold, nets, K, T):
    hp, sd = nets[f"rep{K}"]
    m = build_repcodec(hp, sd)
    x = R.golden_inputs(T)["rep"]
    xd = x.to(DEV)
    tag = f"repcodec K={K} T={T} [{conv_precision}]"
    gz = torch.from_numpy(gold[f"rep_z_{T}"])
    gcodes = torch.from_numpy(gold[f"rep{K}_codes_{T}"]).long()
    # encoder
    z = m.encoder(xd.transpose(1, 2)).transpose(1, 2)
    z64, z32 = R.repcodec_encoder(sd, hp, x, torch.float64), R.repcodec_encoder(sd, hp, x, torch.float32)
    check(f"encoder {tag}", z, z64, z32, 1e-4)
    near_gold("latent", z, gold[f"rep_z_{T}"], z64, z32, 1e-4)
    # quantize
    codes, q = m.quantize(xd)
    assert tuple(codes.shape) == (2, T) and codes.dtype == torch.int64 and tuple(q.shape) == (2, T, 64)
    ch, same, all_sure = check_fvq_codes(tag, sd, hp, z.contiguous(), codes[None], gz, gcodes)
    zh = z.detach().cpu().contiguous()
    f64, f32 = R.fvq(sd, hp, zh, torch.float64, codes=ch), R.fvq(sd, hp, zh, torch.float32, codes=ch)
    check(f"quantized {tag}", q.transpose(1, 2), f64["zq"], f32["zq"], 1e-6)
    # forward: the decoder from the device's quantized
    x_rec, loss, idx = m(xd)
    assert float(loss) == 0.0 and tuple(idx.shape) == (1, 2, T) and torch.equal(idx[0], codes)
    qh = q.transpose(1, 2).cpu()
    check(f"decoder {tag}", x_rec, R.repcodec_decoder(sd, hp, qh, torch.float64), R.repcodec_decoder(sd, hp, qh, torch.float32), 1e-4)
    if K == 64:
        golden_walk(tag, same, all_sure)
        e64, e32 = R.repcodec_forward(sd, hp, x, torch.float64, codes=gcodes[None]), R.repcodec_forward(sd, hp, x, torch.float32, codes=gcodes[None])
        near_gold("x_rec", x_rec, gold[f"rep_rec_{T}"], e64["x_rec"], e32["x_rec"], 1e-4)
    _L().range_check(DEV)


@pytest.mark.parametrize("T", R.GOLDEN_LENGTHS)
def test_coco_vs_fp64_and_golden(conv_precision, gold, nets, T):
    hp, sd = nets["coco"]
    m = build_coco(hp, sd)
    x = R.golden_inputs(T)
    feats = dict(whisper=x["whisper"], chroma=x["chroma"])
    wd, cd = x["whisper"].to(DEV), x["chroma"].to(DEV)
    tag = f"coco T={T} [{conv_precision}]"
    Tq = ((T - 1) // 2 + 1 - 1) // 2 + 1
    gcodes = torch.from_numpy(gold[f"coco_codes_{T}"]).long()
    # the input layers, the down-sampling convs, the encoder: each from the device's stage before it
    x0 = m.input_projection(wd, cd)
    check(f"input layers {tag}", x0, R.coco_input(sd, hp, feats, torch.float64), R.coco_input(sd, hp, feats, torch.float32), 1e-4)
    down = m.downsample_layers(x0)
    assert tuple(down.shape) == (2, 64, Tq)
    check(f"downsample {tag}", down, R.coco_down(sd, hp, x0.cpu(), torch.float64), R.coco_down(sd, hp, x0.cpu(), torch.float32), 1e-4)
    z = m.encoder(down).transpose(1, 2).contiguous()
    check(f"encoder {tag}", z, R.coco_encoder(sd, hp, down.cpu(), torch.float64), R.coco_encoder(sd, hp, down.cpu(), torch.float32), 1e-4)
    # quantize
    codes, q = m.quantize(wd, cd)
    assert tuple(codes.shape) == (2, Tq) and tuple(q.shape) == (2, Tq, 64)
    e64, e32 = (R.coco_forward(sd, hp, feats, dt, codes=gcodes[None]) for dt in (torch.float64, torch.float32))
    near_gold("latent", z, gold[f"coco_z_{T}"], e64["z"], e32["z"], 1e-4)
    ch, same, all_sure = check_fvq_codes(tag, sd, hp, z, codes[None], torch.from_numpy(gold[f"coco_z_{T}"]), gcodes)
    zh = z.cpu()
    f64, f32 = R.fvq(sd, hp, zh, torch.float64, codes=ch), R.fvq(sd, hp, zh, torch.float32, codes=ch)
    check(f"quantized {tag}", q.transpose(1, 2), f64["zq"], f32["zq"], 1e-6)
    # forward: decoder, up-sampling, output layers
    w_rec, c_rec, loss, idx = m(wd, cd)
    assert float(loss) == 0.0 and tuple(idx.shape) == (1, 2, Tq) and torch.equal(idx[0], codes)
    assert tuple(w_rec.shape) == (2, T, 64) and tuple(c_rec.shape) == (2, T, 24)
    qd = q.transpose(1, 2).contiguous()
    dec = m.decoder(qd).transpose(1, 2).contiguous()
    check(f"decoder {tag}", dec, R.coco_decoder(sd, hp, qd.cpu(), torch.float64), R.coco_decoder(sd, hp, qd.cpu(), torch.float32), 1e-4)
    up = m.upsample_layers(dec)
    assert up.shape[2] == 4 * Tq >= T
    check(f"upsample {tag}", up, R.coco_up(sd, hp, dec.cpu(), 4 * Tq, torch.float64), R.coco_up(sd, hp, dec.cpu(), 4 * Tq, torch.float32), 1e-4)
    uh = up[:, :, :T].cpu()
    o64, o32 = R.coco_outputs(sd, hp, uh, torch.float64), R.coco_outputs(sd, hp, uh, torch.float32)
    check(f"whisper output {tag}", w_rec, o64["whisper"], o32["whisper"], 1e-4)
    check(f"chromagram output {tag}", c_rec, o64["chroma"], o32["chroma"], 1e-4)
    golden_walk(tag, same, all_sure)
    near_gold("quantized", q, gold[f"coco_zq_{T}"], e64["zq"].transpose(1, 2), e32["zq"].transpose(1, 2), 1e-4)
    near_gold("whisper_rec", w_rec, gold[f"coco_whisper_{T}"], e64["whisper"], e32["whisper"], 1e-4)
    near_gold("chromagram_rec", c_rec, gold[f"coco_chroma_{T}"], e64["chroma"], e32["chroma"], 1e-4)
    _L().range_check(DEV)


def test_coco_output_length_where_the_upsampled_length_falls_short(nets):
    """the reference repeats the last frame when the up-sampled length is short of T; with these layers 4 T' >= T always, so the rule is driven
    through the decoder half directly"""
    hp, sd = nets["coco"]
    m = build_coco(hp, sd)
    zq = torch.randn(2, 64, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    full = m._decode(12, zq)
    longer = m._decode(15, zq)
    shorter = m._decode(10, zq)
    for a, b, c in zip(full, longer, shorter):
        assert a.shape[1] == 12 and b.shape[1] == 15 and c.shape[1] == 10
        assert torch.equal(b[:, :12], a) and torch.equal(c, a[:, :10])
        assert all(torch.equal(b[:, 12 + i], a[:, 11]) for i in range(3))


@pytest.mark.parametrize("T", R.GOLDEN_LENGTHS)
def test_vevo_repcodec_vs_fp64_and_golden(conv_precision, gold, nets, T):
    _lib = _L()
    hp, sd = nets["vevo"]
    m = build_vevo(hp, sd)
    cbs = R.vevo_codebooks(sd, hp)
    x = R.golden_inputs(T)["vevo"]
    xd = x.to(DEV)
    tag = f"vevo T={T} [{conv_precision}]"
    gz = torch.from_numpy(gold[f"vevo_z_{T}"])
    gcodes = torch.from_numpy(gold[f"vevo_codes_{T}"]).long()
    # the submodules one by one, as vevo_utils calls them
    e = m.encoder(xd)
    check(f"encoder {tag}", e, R.vevo_encoder(sd, hp, x, torch.float64), R.vevo_encoder(sd, hp, x, torch.float32), 1e-4)
    z = m.projector(e)
    z64, z32 = R.vevo_projector(sd, hp, e.cpu(), torch.float64), R.vevo_projector(sd, hp, e.cpu(), torch.float32)
    check(f"projector {tag}", z, z64, z32, 1e-4)
    e2e64, e2e32 = (R.vevo_forward(sd, hp, x, dt, codes=gcodes) for dt in (torch.float64, torch.float32))
    near_gold("latent", z, gold[f"vevo_z_{T}"], e2e64["z"], e2e32["z"], 1e-4)
    zh = z.cpu()
    r64, _, tau, decided = S.margin_rule(cbs, zh)
    und = decided_or_fail(tag, decided)
    zq, idx = m.quantizer.codebook.forward_index(z.transpose(2, 1))
    assert tuple(idx.shape) == (1, 2, T) and tuple(zq.shape) == (2, T, 64)
    ch = idx.cpu()
    assert bool((ch == r64["codes"])[decided].all())
    # the golden codes: a pair counts when its fp64 margin also covers the latent's distance from the reference's (4 |delta|_2 max_k |e_k|_2)
    delta = (zh.double() - gz.double()).norm(dim=1)
    slack = tau + 4.0 * delta * max(float(c.double().norm(dim=1).max()) for c in cbs)
    sure = S.evq_forward(cbs, gz, torch.float64)["margin"] > slack[None]
    assert bool((ch == gcodes)[sure].all())
    print(f"    codes {tag}: tau = {tau:.3g}, undecided {100 * und:.2f} %, {int(sure.sum())} of {sure.numel()} pairs compared with the golden codes")
    f64, f32 = S.evq_forward(cbs, zh, torch.float64, codes=ch), S.evq_forward(cbs, zh, torch.float32, codes=ch)
    check(f"quantized {tag}", zq.transpose(1, 2), f64["zq"], f32["zq"], 1e-6)
    # inference / encode / decode
    zq_i, idx_i = m.quantizer.inference(z)
    assert torch.equal(idx_i, idx) and torch.equal(zq_i, zq.transpose(1, 2))
    m.quantizer.initial()
    zq_e, flat = m.quantizer.encode(z)
    assert torch.equal(flat, idx) and torch.equal(zq_e, zq)                   # one level: the flattened index is the index
    assert torch.equal(m.quantizer.decode(flat), zq[None])
    # forward
    y, zq_f, z_f, vqloss, perplexity = m(xd)
    assert torch.equal(z_f, z) and torch.equal(zq_f, zq.transpose(1, 2)) and tuple(vqloss.shape) == tuple(perplexity.shape) == (1,)
    check(f"decoder {tag}", y, R.vevo_decoder(sd, hp, zq_f.cpu(), torch.float64), R.vevo_decoder(sd, hp, zq_f.cpu(), torch.float32), 1e-4)
    q64, q32 = R.vevo_quantize(sd, hp, zh, torch.float64, codes=ch), R.vevo_quantize(sd, hp, zh, torch.float32, codes=ch)
    check(f"vqloss {tag}", vqloss, q64["loss"], q32["loss"], 1e-6)
    check(f"perplexity {tag}", perplexity, q64["perplexity"], q32["perplexity"], 1e-6)
    golden_walk(tag, torch.equal(ch, gcodes), bool(sure.all()))
    near_gold("y", y, gold[f"vevo_y_{T}"], e2e64["y"], e2e32["y"], 1e-4)
    _lib.range_check(DEV)


def test_quantize_shapes_for_one_and_two_levels(nets):
    """all_indices [N, B, T] is squeezed to [B, T] for N = 1 alone"""
    from amphion_amd.models.codec.coco.rep_coco_model import CocoContent, CocoStyle

    x = R.golden_inputs(5)
    for N in (1, 2):
        hp = R.small_repcodec_hp(64, N)
        sd = R.synth_repcodec_state_dict(hp, 7)
        m = build_repcodec(hp, sd)
        codes, q = m.quantize(x["rep"].to(DEV))
        assert tuple(codes.shape) == ((2, 5) if N == 1 else (2, 2, 5)) and tuple(q.shape) == (2, 5, 64)
        x_rec, _, idx = m(x["rep"].to(DEV))
        assert tuple(idx.shape) == (N, 2, 5) and tuple(x_rec.shape) == (2, 5, 64)
        hp_c = R.small_coco_hp(64, N)
        sd_c = R.synth_coco_state_dict(hp_c, 9)
        mc = build_coco(hp_c, sd_c)
        codes, q = mc.quantize(x["whisper"].to(DEV), x["chroma"].to(DEV))
        assert tuple(codes.shape) == ((2, 2) if N == 1 else (2, 2, 2)) and tuple(q.shape) == (2, 2, 64)
        assert torch.equal(mc(x["whisper"].to(DEV), x["chroma"].to(DEV), return_for_quantizer=True)[0], codes)
    # the one-input classes, the quantizer-only construction and rate 8
    hp = R.small_coco_hp(rate=8)
    for cls, kw, feat in ((CocoContent, dict(chroma=False), "whisper"), (CocoStyle, dict(whisper=False), "chroma")):
        sd = R.synth_coco_state_dict(hp, 11, **kw)
        m = build_coco(hp, sd, cls=lambda cfg: cls(cfg))
        f = x[feat].to(DEV)
        rec, loss, idx = m(f)
        assert tuple(rec.shape) == tuple(f.shape) and tuple(idx.shape) == (1, 2, 1) and float(loss) == 0.0
        codes, q = m.quantize(f)
        assert tuple(codes.shape) == (2, 1) and tuple(q.shape) == (2, 1, 64)
        r64, r32 = (R.coco_forward(sd, hp, {feat: x[feat]}, dt, codes=idx.cpu()) for dt in (torch.float64, torch.float32))
        check(f"{cls.__name__} rate 8", rec, r64[feat], r32[feat], 1e-4)
        only = build_coco(hp, R.synth_coco_state_dict(hp, 11, only_quantizer=True, **kw), cls=lambda cfg: cls(cfg, construct_only_for_quantizer=True))
        assert torch.equal(only.quantize(f)[0], codes)
        with pytest.raises(RuntimeError):
            only(f)


def test_state_dict_round_trip_and_refusals(nets):
    _lib = _L()
    x = R.golden_inputs(5)
    xr, xw, xc, xv = (x[k].to(DEV) for k in ("rep", "whisper", "chroma", "vevo"))
    rep, coco, vevo = build_repcodec(*nets["rep64"]), build_coco(*nets["coco"]), build_vevo(*nets["vevo"])
    for m, (hp, sd), build in ((rep, nets["rep64"], build_repcodec), (coco, nets["coco"], build_coco), (vevo, nets["vevo"], build_vevo)):
        back = m.state_dict()
        assert list(back) == list(sd) and all(torch.equal(back[k].cpu(), sd[k]) for k in sd)
        m2 = build(hp, {k: v.cpu() for k, v in back.items()})
        if m is rep:
            assert torch.equal(m2.quantize(xr)[0], m.quantize(xr)[0])
        elif m is coco:
            assert torch.equal(m2.quantize(xw, xc)[0], m.quantize(xw, xc)[0])
        else:
            assert torch.equal(m2(xv)[0], m(xv)[0])
    calls = (lambda: rep(xr), lambda: rep.quantize(xr), lambda: coco(xw, xc), lambda: coco.quantize(xw, xc), lambda: vevo(xv),
             lambda: vevo.encoder(xv), lambda: vevo.quantizer.inference(xv))
    for m in (rep, coco, vevo):
        m.train()
    for call in calls:
        with pytest.raises(NotImplementedError):
            call()
    for m in (rep, coco, vevo):
        m.eval()
    # a tensor off the module's device, a wrong channel count, a non-fp32 input: refused before any launch
    for call in (lambda: rep.quantize(xr.cpu()), lambda: coco.quantize(xw.cpu(), xc.cpu()), lambda: vevo(xv.cpu()), lambda: vevo.projector(xv.cpu())):
        with pytest.raises(RuntimeError):
            call()
    for call in (lambda: rep.quantize(xc), lambda: coco.quantize(xc, xw), lambda: coco.quantize(xw, xc[:, :3]), lambda: vevo(xc.transpose(1, 2)),
                 lambda: vevo.decoder(xc.transpose(1, 2)), lambda: vevo.quantizer.codebook.forward_index(xc)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: rep.quantize(xr.double()), lambda: coco.quantize(xw.half(), xc), lambda: vevo(xv.double())):
        with pytest.raises(TypeError):
            call()
    # initial() then decode; an index outside its level's codebook raises through amp_evq_check
    vevo.quantizer.initial()
    zq, flat = vevo.quantizer.encode(vevo.projector(vevo.encoder(xv)))
    assert tuple(vevo.quantizer.decode(flat).shape) == (1, 2, 5, 64) and torch.equal(vevo.quantizer.decode(flat)[0], zq)
    assert tuple(vevo.quantizer.decode(flat[:, 0]).shape) == (1, 5, 64)
    bad = flat.clone()
    bad[0, 1, 2] = 32
    with pytest.raises(_lib.AmpError):
        vevo.quantizer.decode(bad)
    assert torch.equal(vevo.quantizer.decode(flat)[0], zq)                   # the check cleared the flag
    _lib.range_check(DEV)
