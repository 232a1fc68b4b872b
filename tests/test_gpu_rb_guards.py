"""Real x in the guard columns of the whole-ResBlock kernel (csrc/rb_f16x3.hip, RbArgs::gx; amp_set_rb_guards) and the launch plan of a
resblock (conv_host.hip rb_geometry / rb_plan; amp_set_rb_split_plan, amp_rb_launch_plan).  With the guards holding the staged x, the first
conv of a launch keeps all W columns and a tile loses that conv's reach less either side: other tile cuts, the same bits.  Every comparison
is torch.equal against the chain of fused pairs (resblock_forward(..., fused=False)) with the guards forced on; the plan arithmetic needs
no device."""
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

DILS = (1, 3, 5)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _weights(C, k, n):
    ws1 = [_rand(C, C, k, seed=10 + p, scale=(C * k) ** -0.5) for p in range(n)]
    bs1 = [_rand(C, seed=20 + p, scale=0.1) for p in range(n)]
    ws2 = [_rand(C, C, k, seed=30 + p, scale=(C * k) ** -0.5) for p in range(n)]
    bs2 = [_rand(C, seed=40 + p, scale=0.1) for p in range(n)]
    return ws1, bs1, ws2, bs2


@pytest.fixture
def sw():
    """the three switches for one call sequence; all back to the policy afterwards"""
    from amphion_amd import _lib

    L = _lib.lib()

    def use(fusion=None, guards=None, plan=None):
        if fusion is not None:
            _lib.check(L.amp_set_resblock_fusion(fusion))
        if guards is not None:
            _lib.check(L.amp_set_rb_guards(guards))
        if plan is not None:
            _lib.check(L.amp_set_rb_split_plan(len(plan), (ctypes.c_int * 3)(*(list(plan) + [0] * (3 - len(plan))))))
    yield use
    _lib.check(L.amp_set_resblock_fusion(-1))
    _lib.check(L.amp_set_rb_guards(-1))
    _lib.check(L.amp_set_rb_split_plan(0, None))


def _plan(C, k, dils, B, T, ragged=False):
    """[(pairs, gx, output columns per tile, tiles per item)] of the launches of one resblock under the current switches"""
    from amphion_amd import _lib

    n = ctypes.c_int()
    v = [(ctypes.c_int * 3)() for _ in range(4)]
    _lib.check(_lib.lib().amp_rb_launch_plan(C, k, (ctypes.c_int * len(dils))(*dils), len(dils), B, T, int(ragged), ctypes.byref(n), *v))
    return [tuple(a[i] for a in v) for i in range(n.value)]


_PAIRS = {}


def _pairs(C, k, dils, B, T):
    """the reference, computed once per shape: the chain of fused pairs (guards play no part in it)"""
    from hip_helpers import resblock_forward

    key = (C, k, dils, B, T)
    if key not in _PAIRS:
        ws1, bs1, ws2, bs2 = _weights(C, k, len(dils))
        _PAIRS[key] = resblock_forward(ws1, bs1, ws2, bs2, _rand(B, C, T, seed=5), dilations=dils, fused=False)
    return _PAIRS[key]


def _guard_columns(C, k, mode):
    return 16 if (C == 128 or (C == 64 and k <= 5 and mode == 3)) else 32


FORMS = [(32, 3), (32, 7), (32, 11), (64, 3), (64, 7), (64, 11), (128, 3)]


@pytest.mark.parametrize("C,k", FORMS)
@pytest.mark.parametrize("mode", [2, 3])
def test_guards_equal_pairs_at_every_tile_cut(C, k, mode, sw):
    """T = 1, the first conv's reach, one tile, one tile + 1 column, two tiles + 1 and two tiles + a guard + 1: the smallest shapes at which
    a guard reads across an item's end (B = 2: into the next item's rows, which the select must keep out), a tile seam, or serves a
    one-column last tile.  Mode 2: the eight-wave tiles, mode 3: the four-wave ones (16 guard columns at C = 64, k = 3)."""
    from amphion_amd import _lib
    from hip_helpers import resblock_forward

    _lib.set_precision("f16x3")
    sw(fusion=mode, guards=1, plan=(3,))
    B = 2
    (pairs, gx, nt, _), = _plan(C, k, DILS, B, 4096)
    reach, rh0 = (k - 1) // 2 * DILS[0], sum((k - 1) // 2 * (d + 1) for d in DILS)
    assert pairs == 3 and gx == 1
    sw(guards=0)
    (_, gx0, nt0, _), = _plan(C, k, DILS, B, 4096)
    assert gx0 == 0 and nt == nt0 + 2 * reach and (nt + 2 * (rh0 - reach)) % 256 == 0
    sw(guards=1)
    ws1, bs1, ws2, bs2 = _weights(C, k, 3)
    for T in (1, reach, nt, nt + 1, 2 * nt + 1, 2 * nt + _guard_columns(C, k, mode) + 1):
        y = resblock_forward(ws1, bs1, ws2, bs2, _rand(B, C, T, seed=5), dilations=DILS, fused=True)
        assert torch.equal(y, _pairs(C, k, DILS, B, T)), (C, k, mode, T)


def _forward_ex(ws1, bs1, ws2, bs2, x, dils, mode, div, y0):
    """amp_resblock_forward_ex: the resblock in the launches of the current plan, the last one with the MRF mode"""
    from amphion_amd import _lib

    L = _lib.lib()
    C, _, k = ws1[0].shape
    n = len(dils)
    h1, h2 = [], []
    try:
        for ws, bs, hs, ds in ((ws1, bs1, h1, dils), (ws2, bs2, h2, [1] * n)):
            for w, b, d in zip(ws, bs, ds):
                h = ctypes.c_void_p()
                w, b = w.contiguous().float(), b.contiguous().float()
                _lib.check(L.amp_conv_create(0, C, C, k, 1, d, (k * d - d) // 2, ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(b.data_ptr()), ctypes.byref(h)))
                hs.append(h)
        xd, y = x.contiguous().float().cuda(), y0.contiguous().float().cuda()
        tmp = torch.full((2,) + tuple(xd.shape), float("nan"), device="cuda")
        B, _, T = xd.shape
        a1, a2 = (ctypes.c_void_p * n)(*[h.value for h in h1]), (ctypes.c_void_p * n)(*[h.value for h in h2])
        _lib.check(L.amp_resblock_forward_ex(a1, a2, n, ctypes.c_void_p(xd.data_ptr()), B, T, 0.1, ctypes.c_void_p(y.data_ptr()), mode, div,
                                             ctypes.c_void_p(tmp.data_ptr()), _lib.current_stream_ptr(xd.device)))
        torch.cuda.synchronize()
        return y.cpu()
    finally:
        for h in h1 + h2:
            L.amp_conv_destroy(h)


@pytest.mark.parametrize("plan", [(3,), (2, 1), (1, 2), (1, 1, 1)])
@pytest.mark.parametrize("C,k", [(64, 11), (32, 7)])
def test_every_forced_plan_has_the_bits_of_one_launch_and_of_the_pairs(C, k, plan, sw):
    """Each launch of a plan sheds its own first conv's reach (other cuts in every launch), x goes through HBM in between and only the last
    launch applies the MRF mode: mode 0 == the fused pairs, modes 1 / 2 == today's single launch with zero guards."""
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    B = 2
    sw(fusion=2, guards=1, plan=plan)
    launches = _plan(C, k, DILS, B, 4096)
    assert [l[0] for l in launches] == list(plan) and all(l[1] == 1 for l in launches)
    T = 2 * launches[0][2] + 1
    ws1, bs1, ws2, bs2 = _weights(C, k, 3)
    x, y0 = _rand(B, C, T, seed=5), _rand(B, C, T, seed=6)
    got = [_forward_ex(ws1, bs1, ws2, bs2, x, DILS, m, 3.0, y0) for m in (0, 1, 2)]
    assert torch.equal(got[0], _pairs(C, k, DILS, B, T))
    sw(guards=0, plan=(3,))
    for m in (1, 2):
        assert torch.equal(got[m], _forward_ex(ws1, bs1, ws2, bs2, x, DILS, m, 3.0, y0)), m
    assert torch.equal(got[1], y0 + got[0])           # one fp32 add per element


def test_first_conv_reach_against_the_guard_width(sw):
    """k = 5, dilations (9, 1) at C = 64: a reach of 18.  The 32-guard tile takes it into the guards; the 16-guard tile (four waves) is
    not built for it at all -- the same guard bounds every read of the tile, so no launch ever has a first conv wider than its guard
    (rb_geometry's zero-guard fallback stays behind that).  Dilations (7, 1), reach 14, fit the 16 columns."""
    from amphion_amd import _lib
    from hip_helpers import resblock_forward

    _lib.set_precision("f16x3")
    C, k, B, T = 64, 5, 2, 700
    x = _rand(B, C, T, seed=5)
    ws1, bs1, ws2, bs2 = _weights(C, k, 2)
    for dils, mode, want_gx in (((9, 1), 2, 1), ((7, 1), 3, 1), ((9, 1), 3, None)):
        sw(fusion=mode, guards=1)
        if want_gx is None:
            with pytest.raises(_lib.AmpError) as e:
                _plan(C, k, dils, B, T)
            assert e.value.status == _lib.AMP_ERR_UNSUPPORTED
            with pytest.raises(_lib.AmpError) as e:
                resblock_forward(ws1, bs1, ws2, bs2, x, dilations=dils, fused=True)
            assert e.value.status == _lib.AMP_ERR_UNSUPPORTED
            continue
        (pairs, gx, nt, _), = _plan(C, k, dils, B, T)
        rh0 = sum(2 * (d + 1) for d in dils)
        assert (pairs, gx) == (2, want_gx) and nt == (512 if mode == 2 else 256) - 2 * (rh0 - 2 * dils[0])
        y = resblock_forward(ws1, bs1, ws2, bs2, x, dilations=dils, fused=True)
        assert torch.equal(y, resblock_forward(ws1, bs1, ws2, bs2, x, dilations=dils, fused=False)), (dils, mode)


def test_ragged_generator_with_guards_equals_without(sw):
    """One up-sampling stage of 64 channels with k = 3 and k = 11 resblocks, lens (40, 17, 1) frames: the guards of a tile at an
    utterance's end cover columns beyond it (zero by select, whatever the workspace holds there) and the next item's rows are never read."""
    from amphion_amd.models.vocoders.gan.generator.hifigan import HiFiGAN
    from amphion_amd.utils.synthetic import randomize_, synthetic_mel

    hp = dict(resblock="1", upsample_rates=[4], upsample_kernel_sizes=[8], upsample_initial_channel=128, resblock_kernel_sizes=[3, 11],
              resblock_dilation_sizes=[[1, 3, 5]] * 2)
    m = randomize_(HiFiGAN(NS(preprocess=NS(n_mel=80, hop_size=4), model=NS(hifigan=NS(**hp)))), 1234).cuda().eval()
    mel = synthetic_mel(3, 80, 40, seed=3).cuda()
    lens = [40, 17, 1]
    out = {}
    with torch.no_grad():
        for g in (0, 1):
            sw(fusion=2, guards=g)
            out[g] = (m(mel).cpu(), m.forward_ragged(mel, lens).cpu())
        sw(fusion=0)
        pairs = m(mel).cpu()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[1][0], pairs)
    for i, n in enumerate(lens):
        assert torch.equal(out[0][1][i, :, : n * 4], out[1][1][i, :, : n * 4])
        assert not torch.isnan(out[1][1][i, :, : n * 4]).any()


def test_range_guard_reports_as_with_zero_guards(sw):
    """C = 32, k = 3, eight-wave tiles: with guards a tile keeps 1 002 columns, tile 1 stages columns 959 .. 990 into its left guard and
    tile 0 keeps them.  An element of 1e6 there is a real operand of both tiles: the report is the one zero guards give, and an in-range
    input reports nothing either way."""
    from amphion_amd import _lib
    from hip_helpers import resblock_forward

    def flag():
        try:
            _lib.range_check()
        except _lib.AmpError as e:
            assert e.status == _lib.AMP_ERR_RANGE, e
            return True
        return False

    _lib.set_precision("f16x3")
    C, k, B, T = 32, 3, 1, 3000
    ws1, bs1, ws2, bs2 = _weights(C, k, 3)
    x = _rand(B, C, T, seed=5)
    big = x.clone()
    big[0, 5, 975] = 1e6
    flag()
    seen = {}
    for g in (0, 1):
        sw(fusion=2, guards=g, plan=(3,))
        (_, gx, nt, _), = _plan(C, k, DILS, B, T)
        assert (gx, nt) == (g, 1000 + 2 * g)
        y = resblock_forward(ws1, bs1, ws2, bs2, x, dilations=DILS, fused=True)
        seen[g] = [flag()]
        assert torch.equal(y, _pairs(C, k, DILS, B, T))
        resblock_forward(ws1, bs1, ws2, bs2, big, dilations=DILS, fused=True)
        seen[g].append(flag())
    assert seen[0] == [False, True] and seen[1] == seen[0]
