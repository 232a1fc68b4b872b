"""CPU side of the recipe-shape tests (tests/test_gpu_recipe_shapes.py, tests/test_gpu_recipe_generators.py): the recipe
hyper-parameters against the drop-in classes and the oracle, the windowed fp64 conv reference against full convolutions, the
derivation of the op-level bound from the split-f16 emulation, and the coverage of the kernel forms by the GPU cases."""
import os
import sys
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import f16x3_emulation as emu  # noqa: E402
from conv_window_ref import conv_window, error_ratio, pick, probe_rows, probe_windows  # noqa: E402
from recipe_shapes import N_MEL, Op, recipe_hps, recipe_ops  # noqa: E402

from oracle import synth  # noqa: E402
from oracle import vocoder_oracle as vo  # noqa: E402


# ---- 1. the recipes ------------------------------------------------------------------------------------------------------------
def _net_and_shapes(name, hp):
    n_mel = N_MEL[name]
    cfg = NS(preprocess=NS(n_mel=n_mel, hop_size=256, sample_rate=24000, extract_amplitude_phase=False))
    if name == "bigvgan_large":
        from amphion_amd.models.vocoders.gan.generator.bigvgan import BigVGAN

        return BigVGAN(NS(preprocess=cfg.preprocess, model=NS(bigvgan=NS(**hp)))), synth.bigvgan_param_shapes(n_mel, hp)
    if name == "nsf":
        from amphion_amd.models.vocoders.gan.generator.nsfhifigan import NSFHiFiGAN

        return NSFHiFiGAN(NS(preprocess=cfg.preprocess, model=NS(nsfhifigan=NS(**hp)))), synth.nsfhifigan_param_shapes(n_mel, hp)
    from amphion_amd.models.vocoders.gan.generator.hifigan import HiFiGAN

    return HiFiGAN(NS(preprocess=cfg.preprocess, model=NS(hifigan=NS(**hp)))), synth.hifigan_param_shapes(n_mel, hp)


@pytest.mark.parametrize("name", ["bigvgan_large", "tfr", "nsf", "hifigan_rb2"])
def test_recipe_hp_matches_the_drop_in_class_and_runs_the_oracle(name):
    """the drop-in class built from the recipe has exactly the synthetic state_dict's keys and shapes, the stage widths of the issue
    table, and the fp64 oracle runs it (B = 1, 4 frames -> 1024 samples)"""
    hp = recipe_hps()[name]
    net, shapes = _net_and_shapes(name, hp)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == {k: tuple(v) for k, v in shapes.items()}
    c0 = hp["upsample_initial_channel"]
    widths = [c0 // 2 ** (i + 1) for i in range(len(hp["upsample_rates"]))]
    assert widths == {"bigvgan_large": [768, 384, 192, 96, 48, 24], "tfr": [384, 192, 96, 48, 24], "nsf": [384, 192, 96, 48, 24],
                      "hifigan_rb2": [128, 64, 32]}[name]
    assert torch.tensor(hp["upsample_rates"]).prod().item() == 256
    sd = synth.synth_state_dict(shapes, 4321, g_gain=0.7)
    mel = synth.synth_mel(1, N_MEL[name], 4, seed=3)
    if name == "bigvgan_large":
        y = vo.bigvgan_forward(sd, hp, mel, dtype=torch.float64)
    elif name == "nsf":
        y = vo.nsfhifigan_forward(sd, hp, mel, dtype=torch.float64)
    else:
        y = vo.hifigan_forward(sd, hp, mel, dtype=torch.float64)
    assert y.shape == (1, 1, 1024) and torch.isfinite(y).all()


# ---- 2. the windowed reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k,d,u,T", [
    (5, 7, 3, 1, 0, 40), (6, 4, 7, 3, 0, 50), (3, 9, 11, 5, 0, 64), (4, 3, 5, 12, 0, 70), (2, 1, 7, 1, 0, 9),
    (6, 5, 4, 1, 2, 17), (3, 4, 8, 1, 4, 11), (5, 3, 16, 1, 8, 9), (4, 2, 5, 1, 2, 13), (3, 3, 9, 1, 4, 6),
])
def test_conv_window_matches_full_conv(cin, cout, k, d, u, T):
    """every probed (item, row, column) of the windowed reference equals the full fp64 conv: dilation, u in {2, 4, 8}, odd k,
    lrelu on load, bias, residual, out slope; windows at both ends, across an 8-column tile seam and overlapping ones"""
    g = torch.Generator().manual_seed(cin * 100 + k * 10 + u + d)
    B = 3
    x = torch.randn(B, cin, T, generator=g)
    b = torch.randn(cout, generator=g)
    if u:
        w = torch.randn(cin, cout, k, generator=g)
        pad = (k - u) // 2
        kw = dict(transposed=True, stride=u, padding=pad)
        full = lambda xx, ww, bb: F.conv_transpose1d(xx, ww, bb, stride=u, padding=pad)
    else:
        w = torch.randn(cout, cin, k, generator=g)
        pad = (k * d - d) // 2
        kw = dict(dilation=d, padding=pad)
        full = lambda xx, ww, bb: F.conv1d(xx, ww, bb, dilation=d, padding=pad)
    for slope_in, slope_out, with_res in ((1.0, 1.0, False), (0.1, 1.0, True), (0.2, 0.3, False)):
        xl = F.leaky_relu(x.double(), slope_in)
        y = full(xl, w.double(), b.double())
        Tout = y.shape[-1]
        res = torch.randn(B, cout, Tout, generator=g) if with_res else None
        cond = full(xl.abs(), w.double().abs(), b.double().abs())
        if res is not None:
            y, cond = y + res.double(), cond + res.double().abs()
        y = F.leaky_relu(y, slope_out)
        wins = probe_windows(Tout, 8, width=4) + [(Tout // 3, Tout // 3 + 5), (-3, 2), (Tout - 1, Tout + 6)]
        rows = probe_rows(cout, 2, up=u or 1, n_random=1)
        ref, rc, cols = conv_window(x, w, b, rows=rows, windows=wins, items=[0, 2], res=res, slope_in=slope_in, slope_out=slope_out,
                                    **kw)
        assert cols.min() >= 0 and cols.max() < Tout and 0 in cols.tolist() and Tout - 1 in cols.tolist()
        torch.testing.assert_close(ref, pick(y, [0, 2], rows, cols), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(rc, pick(cond, [0, 2], rows, cols), rtol=1e-12, atol=1e-12)
        # the error measure: 0 on itself, and a perturbation of one ulp-scale relative to the condition reads back as such
        assert error_ratio(ref, ref, rc) == 0.0
        assert abs(error_ratio(ref + 1e-6 * rc, ref, rc) - 1e-6) < 1e-12


def test_probe_sets():
    """rows: both ends of every row group that holds real rows (polyphase rows for a ConvT), the last real row; windows: both ends
    and the tile seams"""
    rows = probe_rows(192, 128, n_random=0)
    assert rows == [0, 127, 128, 191]
    assert probe_rows(24, 32, n_random=0) == [0, 23]
    # ConvT 384 -> 192, u = 4: 768 GEMM rows in 256-row groups = channels 0..63, 64..127, 128..191
    assert probe_rows(192, 256, up=4, n_random=0) == [0, 63, 64, 127, 128, 191]
    w = probe_windows(1000, 128, width=8, seed=0)
    cols = {c for a, b in w for c in range(a, b)}
    assert {0, 7, 992, 999, 124, 131, 892, 899}.issubset(cols)
    assert all(b0 < a1 for (_, b0), (a1, _) in zip(w, w[1:]))


# ---- 3. the bound: calibration and sensitivity ---------------------------------------------------------------------------------
# The GPU bound on |hip - fp64| / cond (tests/test_gpu_recipe_shapes.py: BOUND).  Derivation, from the emulation below at every
# recipe layer (T = 256, probe rows, lrelu on load, bias):
#   * the kernels' three-product arithmetic errs by at most 4.0e-7 of cond (C = 48, k = 7, K = 336; it does not shrink with K: the
#     fp32 roundings of the running sum and the epilogue dominate, the dropped W_lo X_lo is 2^-22 per product);
#   * dropping W_hi X_lo or W_lo X_hi leaves one f16 rounding (2^-12 relative) per product: over K products of random sign that is
#     ~2^-12 / sqrt(K) of cond per output and, taken over the probes, at least 1.8e-5 of cond at the longest contraction
#     (BigVGAN-large stage 0, K = 768 x 11 = 8448) and up to 1.9e-4 at the shortest.
# BOUND = 2e-6 is 5x above the first (4x is the required margin; the rest is room for the MFMA's own summation order) and 9x below
# the smallest of the second, so a kernel that lost a correction term fails at every layer, whatever its contraction length.
BOUND = 2e-6


def _emulated_ratios(op, T=256):
    g = torch.Generator().manual_seed(op.cin * 7 + op.k * 3 + op.d + op.u)
    if op.u:
        w = torch.randn(op.cin, op.cout, op.k, generator=g) * (op.cin * op.k / op.u) ** -0.5
    else:
        w = torch.randn(op.cout, op.cin, op.k, generator=g) * (op.cin * op.k) ** -0.5
    b = torch.randn(op.cout, generator=g) * 0.1
    x = torch.randn(1, op.cin, T, generator=g)
    rows = sorted(set(probe_rows(op.cout, op.group_rows, up=op.u or 1, n_random=8)))
    wr = w[:, rows] if op.transposed else w[rows]
    ref, cond, _ = conv_window(x, w, b, rows=rows, windows=[(0, op.out_len(T))], slope_in=0.1, **op.kwargs())
    return {t: error_ratio(emu.conv(x, wr, b[rows], slope_in=0.1, terms=t, **op.kwargs()), ref, cond) for t in emu.TERMS}


def test_bound_separates_three_from_two_terms():
    """at every recipe layer: the three-term emulation stays 4x under BOUND, and each two-term emulation exceeds it"""
    from test_gpu_recipe_shapes import BOUND as GPU_BOUND

    assert GPU_BOUND == BOUND
    bad = []
    for op in recipe_ops():
        r = _emulated_ratios(op)
        if not (4 * r[3] <= BOUND and r["no_wh_xlo"] > BOUND and r["no_wlo_xhi"] > BOUND):
            bad.append(f"{op.name} (K = {op.K}): three terms {r[3]:.2e}, no W_hi X_lo {r['no_wh_xlo']:.2e}, no W_lo X_hi {r['no_wlo_xhi']:.2e}")
    assert not bad, "\n".join(bad)


def test_emulation_weight_scale_matches_the_packing():
    """amp_host.h pow2_weight_scale: max|w| * 2^s in (2^12, 2^13], a power of two max|w| lands on 2^13 exactly"""
    for m in (1.0, 0.75, 3.0, 2.0 ** -7, 1e-3):
        s = emu.weight_scale(torch.tensor([m, -m / 3]))
        assert 2.0 ** 12 < m * s <= 2.0 ** 13, m
    hi, lo = emu.split(torch.tensor([1.0 + 2.0 ** -20, 3.0]))
    assert hi.tolist() == [1.0, 3.0] and lo.tolist() == [2.0 ** -20, 0.0]


# ---- 4. coverage of the kernel forms -------------------------------------------------------------------------------------------
def test_recipe_cases_reach_every_form():
    """the GPU op cases (as Op.form() predicts them; the GPU test asserts the manifest against the same prediction) include every
    form the issue lists"""
    from test_gpu_recipe_shapes import cases, large_grid, small_grid

    seen = {}
    for name, op, _ in cases():
        for grid in (small_grid(op), large_grid(op)):
            f = op.form(*grid)[0]
            seen.setdefault(f, []).append((op, grid))
            assert op.form(*grid, precision="f32")[0] == "conv_mfma_kernel"
    blk2d_multi = [op for f, v in seen.items() if f.startswith("conv_blk") and f.endswith("/2d") for op, _ in v if op.M // 256 > 1]
    assert blk2d_multi, "conv_blk with several row groups in the 2-D grid"
    assert any(op.transposed for op in blk2d_multi), "the transposed conv_blk (kt2) in the 2-D grid"
    assert "conv_blk_kernel/k7/wn1/2d" in seen and "conv_blk_kernel/k11/wn1/2d" in seen, "the A-ring conv_blk at k = 7 / 11"
    assert any(f.startswith("conv_blk_kernel/k7/wn2") for f in seen) and any(f.startswith("conv_blk_kernel/k11/wn2") for f in seen)
    assert any(op.padded_rows for op, _ in seen["conv_f16x3_kernel"]), "conv_f16x3 with padded rows"
    assert {op.cout for op, _ in seen["conv_small_kernel"] if op.padded_rows} >= {192, 96}, "conv_small with padded rows"
    assert any(f.endswith("/1d") for f in seen), "the row-group-fastest order"
    assert all(op.padded_rows == 0 for f, v in seen.items() if f.startswith("conv_blk") for op, _ in v)
    # long contractions and odd / partly empty chunks
    assert max(op.K for op in recipe_ops()) == 8448
    assert {Op(100, 768, 7), Op(24, 24, 3), Op(48, 48, 3), Op(128, 128, 7, 12)} <= set(recipe_ops())
