"""Fitted strips of the fused-pair strip kernel (pair_strip_f16x3.hip, PairArgs::fit; amp_set_strip_fit): a strip's outputs start at its
first column and a halo prologue computes the k - 1 carried xt columns, instead of the strip starting k - 1 columns early.  Every case runs
C = 128 with amp_set_strip_fit(1) -- every strip launch fitted -- and must give the bits of the per-tile kernel (amp_set_pair_strips(0)).

Strips run on launches of 512+ of them, so B = 8 at T near 16 384 is the small shape: 64 one-step fitted strips per item.  One (64, 16 384)
case runs the plan's own choice for the benchmarked shape."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C, B_SMALL, T0 = 128, 8, 16384


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _params(k):
    w1 = _rand(C, C, k, seed=1, scale=(C * k) ** -0.5)
    b1 = _rand(C, seed=2, scale=0.1)
    w2 = _rand(C, C, k, seed=3, scale=(C * k) ** -0.5)
    b2 = _rand(C, seed=4, scale=0.1)
    return w1, b1, w2, b2


_X = {}


def _x(B, T):
    """one input per shape, shared by the cases (never modified: the range case clones)"""
    if (B, T) not in _X:
        _X[(B, T)] = _rand(B, C, T, seed=5)
    return _X[(B, T)]


def _ref(w1, b1, w2, b2, x, d, slope=0.1):
    k = w1.shape[2]
    xt = F.conv1d(F.leaky_relu(x, slope), w1, b1, dilation=d, padding=(k * d - d) // 2)
    xt = F.conv1d(F.leaky_relu(xt, slope), w2, b2, padding=(k - 1) // 2)
    return xt + x


@pytest.fixture
def switches():
    """(pair_strips, strip_fit) for one call sequence; both back to the policy afterwards"""
    from amphion_amd import _lib

    def use(strips, fit):
        _lib.check(_lib.lib().amp_set_pair_strips(strips))
        _lib.check(_lib.lib().amp_set_strip_fit(fit))
    yield use
    _lib.check(_lib.lib().amp_set_pair_strips(-1))
    _lib.check(_lib.lib().amp_set_strip_fit(-1))


def _plan(B, T, k):
    """(form, strip_len, strips per item, steps per strip) under the current switches"""
    import ctypes
    from amphion_amd import _lib

    v = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.lib().amp_pair_strip_plan(B, T, k, 0, *[ctypes.byref(c) for c in v]))
    return tuple(c.value for c in v)


def _fit_equals_tile(k, d, B, T, switches, fit=1):
    from amphion_amd import _lib
    from hip_helpers import pair_forward

    _lib.set_precision("f16x3")
    w1, b1, w2, b2 = _params(k)
    x = _x(B, T)
    switches(0, -1)
    y_tile = pair_forward(w1, b1, w2, b2, x, dilation=d)
    switches(-1, fit)
    form, strip_len, spi, _ = _plan(B, T, k)
    assert form == 1 and B * spi >= 512, (form, strip_len, spi)      # the launch below is a fitted strip launch
    y_fit = pair_forward(w1, b1, w2, b2, x, dilation=d)
    assert not torch.isnan(y_fit).any()
    assert torch.equal(y_fit, y_tile), (k, d, B, T)
    return y_fit


@pytest.mark.parametrize("k", [7, 11])
@pytest.mark.parametrize("d", [1, 3, 5])
def test_exact_multiples_of_a_step(k, d, switches):
    """T = 64 steps: every strip starts on a step boundary; the first and last k - 1 columns of an item are the zero-padding cases (strip 0's
    prologue lies half outside the item, the last step's seam ends at the item's end)."""
    _fit_equals_tile(k, d, B_SMALL, T0, switches)


@pytest.mark.parametrize("k,dT", [(11, -1), (11, 1), (11, -10), (11, 10), (11, 255), (7, -6), (7, 6), (7, 1), (7, 255)])
def test_off_by_a_few(k, dT, switches):
    """The last strip is one column (+1), exactly the halo (+(k - 1)), one column short of a step (+255), or the item ends just inside the last
    full strip (-1, -(k - 1))."""
    _fit_equals_tile(k, 3, B_SMALL, T0 + dT, switches)


def test_headline_shape_runs_the_plan(switches):
    """(64, 16 384): the benchmarked stage-1 shape under the plan itself (amp_set_strip_fit(-1)), and with every launch fitted at the shifted
    plan's four steps per strip"""
    for fit in (-1, 1):
        _fit_equals_tile(11, 3, 64, T0, switches, fit=fit)


@pytest.mark.parametrize("k,d", [(11, 5), (7, 1)])
def test_partition_batch_invariance_and_oracle(k, d, switches):
    """Items 0 and B - 1 of the fitted launch equal that item run alone (a single item runs the per-tile kernel: another plan, the same
    bits), and one probed item matches the fp64 oracle within the 5e-6 of tests/test_gpu_pair.py."""
    from hip_helpers import pair_forward

    y = _fit_equals_tile(k, d, B_SMALL, T0, switches)
    w1, b1, w2, b2 = _params(k)
    x = _x(B_SMALL, T0)
    for b in (0, B_SMALL - 1):
        y1 = pair_forward(w1, b1, w2, b2, x[b:b + 1], dilation=d)
        assert torch.equal(y[b:b + 1], y1), f"item {b}"
    Tp = 6000                       # oracle on a prefix: exact for the first Tp - receptive field columns (23 strip starts among them)
    ref = _ref(w1.double(), b1.double(), w2.double(), b2.double(), x[-1:, :, :Tp].double(), d)
    keep = Tp - (k - 1) * (d + 1)
    err = (y[-1:, :, :keep].double() - ref[..., :keep]).abs().max().item()
    print(f"k={k} d={d}: |fitted strips - f64| = {err:.2e}")
    assert err <= 5e-6


def test_range_guard_sees_the_prologue(switches):
    """An operand beyond 4 094 in the columns a halo prologue stages (just in front of a strip's first output) raises the flag, as it does
    for the per-tile kernel; the in-range input does not.  (Every prologue operand is also an operand of the neighbouring strip's last step:
    the case checks that the fitted launch decides like the other forms, not the prologue in isolation.)"""
    from amphion_amd import _lib
    from hip_helpers import pair_forward

    _lib.set_precision("f16x3")
    k, d = 11, 3
    w1, b1, w2, b2 = _params(k)
    x = _x(B_SMALL, T0).clone()
    try:
        _lib.range_check()
    except _lib.AmpError:
        pass
    switches(-1, 1)
    assert _plan(B_SMALL, T0, k)[0] == 1
    pair_forward(w1, b1, w2, b2, x, dilation=d)
    _lib.range_check()                                   # in range: no flag
    x[3, 17, 37 * 256 - 3] = 5e3                         # item 3, three columns in front of strip 37's first output
    for strips, fit in ((-1, 1), (0, -1)):
        switches(strips, fit)
        pair_forward(w1, b1, w2, b2, x, dilation=d)
        with pytest.raises(_lib.AmpError) as e:
            _lib.range_check()
        assert e.value.status == _lib.AMP_ERR_RANGE
        _lib.range_check()                               # the check cleared the flag


def _child(out):
    """default switches, one process (the manifest is opened once per process): the two shapes, their manifest lines"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from amphion_amd import _lib
    from hip_helpers import pair_forward

    _lib.set_precision("f16x3")
    man = os.environ["AMP_LAUNCH_MANIFEST"]
    w1, b1, w2, b2 = _params(11)
    res = {}
    for B, T in ((64, 16384), (70, 15000)):
        n0 = sum(1 for _ in open(man)) if os.path.exists(man) else 0
        y = pair_forward(w1, b1, w2, b2, _rand(B, C, T, seed=5), dilation=1)
        assert torch.isfinite(y).all()
        res[f"{B}x{T}"] = open(man).read().splitlines()[n0:]
        with open(out, "w") as fh:
            json.dump(res, fh)


def test_the_plan_reaches_the_fitted_form_by_itself(tmp_path):
    """amp_set_strip_fit(-1), nothing set: at (64, 16 384) the launch's manifest line names the fitted form, at (70, 15 000) -- no round of
    workgroups to save -- the shifted one.  The plan makes the choice, not the switch."""
    out, man = tmp_path / "lines.json", tmp_path / "manifest.tsv"
    env = dict(os.environ, AMP_LAUNCH_MANIFEST=str(man), AMP_PRECISION="f16x3")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and out.exists(), f"child exit {r.returncode}\n{r.stderr[-2000:]}"
    res = json.load(open(out))
    for shape, form in (("64x16384", "fitted"), ("70x15000", "shifted")):
        lines = res[shape]
        assert len(lines) == 1 and lines[0].startswith("pair_strip_kernel<11, 2, 2, 4, 320, 2, 4, 1>\t"), lines
        assert f" {form} strips of " in lines[0], lines


if __name__ == "__main__":
    _child(sys.argv[1])
