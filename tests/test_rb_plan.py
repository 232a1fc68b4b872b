"""CPU: the geometry and the launch plan of the whole-ResBlock kernel (conv_host.hip rb_geometry / rb_plan, through amp_rb_launch_plan):
with real x in the guard columns every launch sheds its first conv's reach; the plan cuts a resblock where that saves rounds of
workgroups and keeps the round-5 plan everywhere else."""
import ctypes

import pytest

DILS = (1, 3, 5)


def _plan(C, k, B, T, ragged=False, dils=DILS):
    """[(pairs, gx, output columns per tile, tiles per item)] per launch"""
    from amphion_amd import _lib

    n = ctypes.c_int()
    v = [(ctypes.c_int * 3)() for _ in range(4)]
    _lib.check(_lib.lib().amp_rb_launch_plan(C, k, (ctypes.c_int * len(dils))(*dils), len(dils), B, T, int(ragged), ctypes.byref(n), *v))
    return [tuple(a[i] for a in v) for i in range(n.value)]


@pytest.fixture
def sw():
    from amphion_amd import _lib

    L = _lib.lib()

    def use(guards=None, plan=None):
        if guards is not None:
            _lib.check(L.amp_set_rb_guards(guards))
        if plan is not None:
            _lib.check(L.amp_set_rb_split_plan(len(plan), (ctypes.c_int * 3)(*(list(plan) + [0] * (3 - len(plan))))))
    yield use
    _lib.check(L.amp_set_rb_guards(-1))
    _lib.check(L.amp_set_rb_split_plan(0, None))


def _rounds(B, launches, slots):
    return [-(-B * tiles // slots) for _, _, _, tiles in launches]


def test_zero_guards_give_the_round_5_geometry(sw):
    """the benchmark's launches at B = 64 as they were: 19 rounds of workgroups each"""
    sw(guards=0)
    assert _plan(64, 11, 64, 32768) == [(2, 0, 452, 73), (1, 0, 452, 73)]
    assert _plan(32, 11, 64, 65536) == [(3, 0, 904, 73)]
    assert _plan(64, 7, 64, 32768) == [(3, 0, 440, 75)]
    assert _plan(32, 7, 64, 65536) == [(3, 0, 440, 149)]          # four-wave tiles: 512 slots
    for C, k, T, slots in ((64, 11, 32768, 256), (32, 11, 65536, 256), (64, 7, 32768, 256), (32, 7, 65536, 512)):
        assert set(_rounds(64, _plan(C, k, 64, T), slots)) == {19}


def test_guards_shed_the_first_reach_of_every_launch(sw):
    """RH' = RH - (k-1)/2 * d_first per launch: the tiles and workgroups of the benchmark's rows with the guards on, plans forced"""
    sw(guards=1, plan=(2, 1))
    assert _plan(64, 11, 64, 32768) == [(2, 1, 462, 71), (1, 1, 502, 66)]          # 4 544 / 4 224 workgroups: 18 / 17 rounds
    assert _plan(64, 7, 64, 32768) == [(2, 1, 482, 68), (1, 1, 506, 65)]           # 4 352 = 17.0 rounds / 4 160
    assert _plan(32, 7, 64, 65536) == [(2, 1, 482, 136), (1, 1, 506, 130)]         # 8 704 = 17.0 rounds of 512
    assert _rounds(64, _plan(64, 11, 64, 32768), 256) == [18, 17]
    assert _rounds(64, _plan(64, 7, 64, 32768), 256) == [17, 17]
    assert _rounds(64, _plan(32, 7, 64, 65536), 512) == [17, 17]
    sw(plan=(3,))
    assert _plan(32, 11, 64, 65536) == [(3, 1, 914, 72)]                           # 4 608 workgroups = exactly 18 rounds
    assert _plan(64, 7, 64, 32768) == [(3, 1, 446, 74)]                            # whole: still 19 rounds
    assert _plan(64, 3, 64, 32768) == [(3, 1, 234, 141)] and _plan(32, 3, 64, 65536) == [(3, 1, 490, 134)]   # RH 12 -> 11: no round saved
    sw(plan=(1, 1, 1))
    assert _plan(64, 11, 64, 32768) == [(1, 1, 502, 66)] * 3                       # every pair sheds its own dilated conv: 17 rounds each
    sw(plan=(1, 2))
    assert _plan(64, 11, 64, 32768) == [(1, 1, 502, 66), (2, 1, 442, 75)]


def test_policy_at_the_benchmark_shapes():
    """nothing set: the guards where they were measured to pay (k = 11, and C = 64 k = 7 with the cut the model then finds), the round-5
    launches everywhere else"""
    assert _plan(64, 11, 64, 32768) == [(2, 1, 462, 71), (1, 1, 502, 66)]
    assert _plan(64, 7, 64, 32768) == [(2, 1, 482, 68), (1, 1, 506, 65)]
    assert _plan(32, 11, 64, 65536) == [(3, 1, 914, 72)]
    assert _plan(32, 7, 64, 65536) == [(3, 0, 440, 149)]
    assert _plan(64, 3, 64, 32768) == [(3, 0, 232, 142)] and _plan(32, 3, 64, 65536) == [(3, 0, 488, 135)]
    assert _plan(64, 7, 64, 32768, ragged=True) == [(3, 1, 446, 74)]          # ragged: the guards, not the new cut


@pytest.mark.parametrize("guards", [-1, 0, 1])
def test_small_grids_keep_the_round_5_plan(guards, sw):
    """the one-stage generator of tests/test_gpu_resblock.py (C = 64, k = 11, T = 6 400): 4 + 2 convs at B = 64 (1 088 workgroups on the
    zero-guard count), one launch of 6 at B = 32 -- never three launches below 2 048 workgroups, never fewer launches than round 5 chose"""
    sw(guards=guards)
    assert [l[0] for l in _plan(64, 11, 64, 6400)] == [2, 1]
    assert [l[0] for l in _plan(64, 11, 32, 6400)] == [3]
    assert [l[0] for l in _plan(64, 11, 64, 32768, ragged=True)] == [2, 1]
    assert [l[0] for l in _plan(64, 7, 64, 32768, ragged=True)] == [3]


def test_switches_refuse_what_they_do_not_know():
    from amphion_amd import _lib

    L = _lib.lib()
    for call in (lambda: L.amp_set_rb_guards(2), lambda: L.amp_set_rb_guards(-2), lambda: L.amp_set_rb_split_plan(2, (ctypes.c_int * 3)(2, 2, 0)),
                 lambda: L.amp_set_rb_split_plan(2, (ctypes.c_int * 3)(3, 0, 0)), lambda: L.amp_set_rb_split_plan(4, (ctypes.c_int * 3)(1, 1, 1))):
        with pytest.raises(_lib.AmpError):
            _lib.check(call())
    assert _plan(64, 11, 64, 32768)[0][0] in (1, 2, 3)          # nothing stuck
