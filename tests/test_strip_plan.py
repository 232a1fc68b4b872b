"""CPU: the strip plan of the fused C = 128 pairs (conv_host.hip strip_geometry, through amp_pair_strip_plan): fitted strips where they
save a round of workgroups, today's shifted strips everywhere else."""
import ctypes

import pytest


def _plan(B, T, k, ragged=False):
    from amphion_amd import _lib

    v = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.lib().amp_pair_strip_plan(B, T, k, int(ragged), *[ctypes.byref(c) for c in v]))
    return tuple(c.value for c in v)      # form, strip_len, strips per item, steps per full strip


def _steps_per_item(T, k, plan):
    form, strip_len, spi, steps = plan
    last = T - (spi - 1) * strip_len
    return (spi - 1) * steps + (last + (0 if form else k - 1) + 255) // 256


@pytest.fixture
def fit():
    from amphion_amd import _lib

    def use(mode):
        _lib.check(_lib.lib().amp_set_strip_fit(mode))
    yield use
    _lib.check(_lib.lib().amp_set_strip_fit(-1))


@pytest.mark.parametrize("k", [7, 11])
def test_headline_shape_is_64_steps_in_16_rounds(k, fit):
    B, T = 64, 16384
    fit(0)
    shifted = _plan(B, T, k)
    assert shifted == (0, 4 * 256 - (k - 1), 17, 4)
    assert _steps_per_item(T, k, shifted) == 65                       # the 17th strip is one more step: ceil(65 * 64 / 256) = 17 rounds
    fit(-1)
    plan = _plan(B, T, k)
    form, strip_len, spi, steps = plan
    assert form == 1 and strip_len == steps * 256 and steps in (4, 8)
    assert _steps_per_item(T, k, plan) == 64
    assert B * spi % 256 == 0 and B * spi // 256 * steps == 16        # whole rounds of workgroups, 16 rounds of steps
    fit(1)
    assert _plan(B, T, k) == (1, 1024, 16, 4)                         # every launch fitted: the shifted plan's four steps


@pytest.mark.parametrize("B,T", [(64, 16385), (70, 15000), (64, 16000), (64, 4100), (8, 16384), (200, 16384 + 10)])
def test_no_round_saved_keeps_todays_plan(B, T, fit):
    for k in (7, 11):
        fit(0)
        today = _plan(B, T, k)
        fit(-1)
        assert _plan(B, T, k) == today and today[0] == 0


def test_ragged_batches_are_untouched(fit):
    for k in (7, 11):
        fit(0)
        today = _plan(64, 16384, k, ragged=True)
        assert today == (0, 256 - (k - 1), (16384 + 245 - (k - 11)) // (256 - (k - 1)), 1)
        fit(-1)
        assert _plan(64, 16384, k, ragged=True) == today


def test_switch_and_plan_arguments_are_checked():
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 151
    for bad in (-2, 2):
        with pytest.raises(_lib.AmpError) as ei:
            _lib.check(L.amp_set_strip_fit(bad))
        assert "amp_set_strip_fit" in str(ei.value)
    with pytest.raises(_lib.AmpError):
        _plan(64, 16384, 3)                                           # k = 3 pairs have no strip kernel
