"""CPU side of the inverse-STFT / mel-gradient geometry sweep (tests/stft_geometry.py; the kernels run in tests/test_gpu_stft_geometry.py):
  - the fp64 references agree with independent code: the oracle's conv-basis STFT.inverse and fold-based APNet ISTFT, and torch.istft;
  - every class a table claims is re-derived from the numbers, and every required class is reached: an edit that loses one fails here;
  - a float32 restatement of the kernels' arithmetic stays inside the bounds the GPU tests use at every table point, and each one-slip
    mutant of it leaves them on at least one -- the truncating frame count of the ragged rows among them;
  - no fp64 mel energy of a gradient case lies within 1e-3 (relative) of the log clamp, so fp32 decides the clamp's 0 / 1 gradient alike.
The ratios printed here (error / bound; run with -s) are the ones DESIGN.md quotes."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import stft_geometry as sg  # noqa: E402
from oracle import vocoder_oracle as vo  # noqa: E402

GUARD = 64


@functools.lru_cache(maxsize=None)
def _ist(name):
    c = sg.ist_by_id(name)
    inp = sg.ist_inputs(c)
    return c, inp, sg.ist_reference(c, inp)


@functools.lru_cache(maxsize=None)
def _grad(name):
    c = sg.grad_by_id(name)
    wav, g = sg.grad_inputs(c)
    return c, wav, g, sg.grad_reference(c, wav, g)


# ---- the references against independent code --------------------------------------------------------------------------------
def _no_tiny(c):
    return c.mode == "forward" and c.window == "hann" and "tiny_skip" not in sg.ist_labels(c)


@pytest.mark.parametrize("name", [c.id for c in sg.ISTFT if _no_tiny(c) and c.n_fft <= 1100])
def test_forward_reference_equals_the_conv_basis_inverse(name):
    """utils/stft.py:183-222 as the oracle restates it: conv_transpose1d with the pseudo-inverse basis (kept in float32 there: 6e-8 relative)"""
    c, inp, ref = _ist(name)
    out = vo.taco_stft_inverse(inp["mag"], inp["phase"], c.n_fft, c.hop, c.win, dtype=torch.float64)[:, 0]
    assert out.shape == ref["out"].shape
    assert sg.ist_excess(ref, out) <= 0.25


@pytest.mark.parametrize("name", [c.id for c in sg.ISTFT if _no_tiny(c)])
def test_forward_reference_equals_torch_istft(name):
    c, inp, ref = _ist(name)
    d = sg.ist_den32(c)[c.crop:c.crop + c.Lout]
    if d.min() <= 1e-11:
        pytest.fail("a case without a tiny stretch whose wss torch.istft would refuse: " + name)
    re, im = sg.ist_spectrum(c, inp)
    w = torch.from_numpy(sg.ist_window32(c)).double()
    out = torch.istft(torch.complex(re, im), c.n_fft, c.hop, c.n_fft, w, center=True, onesided=True, length=c.Lout)
    # torch divides by the fp64 envelope of the float32 window, the reference by its float32 rounding: 6e-8 relative
    assert (out - ref["out"]).abs().max() <= 1e-6 * max(1.0, float(ref["out"].abs().max()))


@pytest.mark.parametrize("name", [c.id for c in sg.ISTFT if c.mode == "same" and c.crop > 0])
def test_same_reference_equals_the_fold_based_istft(name):
    c, inp, ref = _ist(name)
    re, im = sg.ist_spectrum(c, inp)
    w = torch.from_numpy(sg.ist_window32(c)).double()
    out = vo.apnet_istft_same(torch.complex(re, im), c.n_fft, c.hop, c.win, w)
    assert out.shape == ref["out"].shape
    assert (out - ref["out"]).abs().max() <= 1e-6 * max(1.0, float(ref["out"].abs().max()))


def test_polar_reference_is_the_same_reference_on_the_formed_spectrum():
    for c in sg.ISTFT:
        if c.form != "head":
            continue
        _, inp, ref = _ist(c.id)
        h = inp["head"][:, :2 * c.bins * c.F].reshape(c.B, 2 * c.bins, c.F).double()
        mag = torch.exp(h[:, :c.bins]).clamp(max=inp["clip"])
        twin = sg.Ist("twin", "same", c.n_fft, c.hop, c.F, B=c.B)
        r2 = sg.ist_reference(twin, {"re": mag * torch.cos(h[:, c.bins:]), "im": mag * torch.sin(h[:, c.bins:])})
        assert torch.equal(r2["out"], ref["out"])
        assert float(inp["head"][:, 2 * c.bins * c.F:].nan_to_num(nan=1.0).sum()) == c.B * c.stride_extra      # the gap holds NaN only


def test_gradient_restatement_equals_the_oracle_at_its_own_configuration():
    c = sg.grad_by_id("g400_F32")
    wav, _ = sg.grad_inputs(c)
    y = wav[0].double()
    twin = sg.Grad("twin", c.n_fft, c.hop, c.n_mel, c.L, mag_eps=1e-9 + 1e-24)      # takes the restatement, not the oracle
    a, b = sg.mel64(y, c), sg.mel64(y, twin)
    assert a.shape == b.shape == (c.n_mel, c.F)
    assert (a - b).abs().max() <= 1e-6                                             # (the oracle's fp64 window against the float32 one)


# ---- class coverage -------------------------------------------------------------------------------------------------------
def test_istft_table_reaches_every_class_it_claims():
    ids = [c.id for c in sg.ISTFT]
    assert len(set(ids)) == len(ids)
    for c in sg.ISTFT:
        lab = sg.ist_labels(c)
        assert set(c.why) <= lab, (c.id, sorted(set(c.why) - lab))
        assert c.hop <= c.n_fft and 64 <= c.n_fft <= 4096
        if c.mode != "forward":
            assert c.win == c.n_fft and (c.win - c.hop) % 2 == 0, c.id
            assert sg.envelope_floor(c) >= 1e-3, (c.id, sg.envelope_floor(c))
        if "prime" in lab and c.n_fft > 1000:
            assert c.B * c.F <= 16, c.id                                            # a prime length is a direct DFT
        # DEVICE_TENSOR_CAP: the frame scratch and the head slab are the largest tensors of a case
        assert (c.B * c.F * c.n_fft + 2 * GUARD + c.offset) * 4 <= sg.DEVICE_TENSOR_CAP, c.id
        assert c.B * ((c.n_fft + 2) * c.F + c.stride_extra) * 4 <= sg.DEVICE_TENSOR_CAP, c.id
    missing = set(sg.ISTFT_REQUIRED) - sg.ist_required_reached()
    assert not missing, sorted(missing)
    for name in sg.POLAR_SPLIT_CASES:
        assert sg.ist_by_id(name).form == "head"
    assert {sg.frames_form(sg.ist_by_id(n).n_fft) for n in sg.POLAR_SPLIT_CASES} == {"radix2", "mixed", "wave15"}
    # the unaligned 1920 cases have an aligned twin with the same inputs
    for c in sg.ISTFT:
        if c.offset:
            twin = [t for t in sg.ISTFT if (t.mode, t.n_fft, t.hop, t.F, t.B, t.offset) == (c.mode, c.n_fft, c.hop, c.F, c.B, 0)]
            assert len(twin) == 1 and twin[0].seed == c.seed, c.id


def test_refusal_table_covers_every_documented_refusal():
    ids = [r[0] for r in sg.REFUSALS]
    assert len(set(ids)) == len(ids)
    kinds = {(e, tuple(sorted(k for k in ch))) for _, e, ch, _ in sg.REFUSALS}
    for want in (("forward", ("F",)), ("forward", ("hop",)), ("same", ("hop",)), ("same", ("win",)), ("same_polar", ("hop",)),
                 ("same_polar", ("win",)), ("same_polar", ("stride",)), ("same_polar", ("clip",)), ("forward", ("null",)), ("same", ("null",)),
                 ("same_polar", ("null",))):
        assert want in kinds, want
    nffts = {ch["n_fft"] for _, _, ch, _ in sg.REFUSALS if "n_fft" in ch}
    assert min(nffts) < 64 and max(nffts) > 4096
    b = sg.REFUSAL_BASE
    for _, e, ch, _ in sg.REFUSALS:                                                  # each odd-(win - hop) row really is odd, each hop row above n_fft
        if e != "forward" and set(ch) == {"hop"}:
            assert ch["hop"] > b["n_fft"] or (b["win"] - ch["hop"]) % 2 == 1


def test_gradient_table_reaches_every_class_it_claims():
    ids = [c.id for c in sg.GRAD]
    assert len(set(ids)) == len(ids)
    have = set()
    for c in sg.GRAD:
        lab = sg.grad_labels(c)
        have |= lab
        assert set(c.why) <= lab, (c.id, sorted(set(c.why) - lab))
        assert c.counts()[0] == c.F >= 1 and c.L > c.pad, c.id
        assert (c.B * c.F * c.n_fft + 2 * GUARD) * 4 <= sg.DEVICE_TENSOR_CAP, c.id       # frames_ws
        assert (2 * c.B * c.bins * c.F + 2 * GUARD) * 4 <= sg.DEVICE_TENSOR_CAP, c.id    # spec_ws
        assert (c.B * c.L + 2 * GUARD) * 4 <= sg.DEVICE_TENSOR_CAP, c.id
    assert not set(sg.GRAD_REQUIRED) - have, sorted(set(sg.GRAD_REQUIRED) - have)
    assert {(c.n_fft, c.hop, c.n_mel) for c in sg.GRAD} == set(sg.GRAD_CONFIGS)
    for n, h, m in sg.GRAD_CONFIGS:                                                  # every hop above n_fft / 3 has its ragged batch of four
        if 3 * h > n:
            rag = [c for c in sg.GRAD if (c.n_fft, c.hop) == (n, h) and c.lens]
            assert len(rag) == 1 and rag[0].B == 4 and {"zero_frame_short", "zero_frame_pad", "off_grid"} <= sg.grad_labels(rag[0]), (n, h)
            assert rag[0].counts()[0] > 0 and rag[0].lens[0] == rag[0].L
    assert any(c.n_mel % 8 == 0 for c in sg.GRAD)


def test_ragged_forward_table_takes_every_kernel_form():
    forms = {}
    for n, h, m, form in sg.RAGGED_FWD:
        assert sg.mel_forward_form(n, h, m) == form, (n, h)
        assert 3 * h > n
        forms.setdefault(form, set()).add(n)
        lens = sg.ragged_fwd_lens(n, h)
        pad = (n - h) // 2
        counts = [sg.row_frames(v, n, h) for v in lens]
        assert counts[0] > sg.WAVE_FRAMES and counts[2] == sg.WAVE_FRAMES + 1 and counts[1] == 0 and counts[3] == 0 and counts[4] >= 1
        assert pad < lens[1] < h and lens[3] <= pad and sg.truncating_row_frames(lens[1], n, h) == 1
        assert len(lens) * (n // 2 + 1) * counts[0] * 4 <= sg.DEVICE_TENSOR_CAP
    assert forms["mel1024"] == {1024} and forms["mel_wave"] == {2048, 512, 1920} and forms["mel_kernel"] == {256} and forms["mel_mixed"] >= {400, 1001, 1920}


def test_phantom_frame_lengths_of_the_issue():
    """the lengths at which C division gave a ragged row a frame 0 it does not have"""
    for n, h, lo, hi in ((400, 160, 121, 159), (512, 256, 129, 255), (1000, 400, 301, 399), (1001, 501, 251, 500), (646, 320, 164, 319)):
        bad = [v for v in range(1, 2 * n) if sg.truncating_row_frames(v, n, h) != sg.row_frames(v, n, h)]
        assert bad == list(range(lo, hi + 1)), (n, h, bad[:3], bad[-3:])
    for n, h in ((1024, 256), (2048, 512), (1920, 480), (64, 16)):                   # hop <= n_fft / 3: never
        assert all(sg.truncating_row_frames(v, n, h) == sg.row_frames(v, n, h) for v in range(1, 2 * n))


# ---- discrimination ---------------------------------------------------------------------------------------------------------
def test_istft_restatement_is_inside_the_bound_and_every_mutant_leaves_it():
    worst, best = ("", 0.0), {m: ("", 0.0) for m in sg.ISTFT_MUTANTS}
    for case in sg.ISTFT:
        c, inp, ref = _ist(case.id)
        r = sg.ist_excess(ref, sg.ist_model(c, inp))
        assert r <= 1.0, (c.id, r)
        if r > worst[1]:
            worst = (c.id, r)
        for m in sg.ISTFT_MUTANTS:
            if best[m][1] == math.inf:
                continue
            e = sg.ist_excess(ref, sg.ist_model(c, inp, m))
            if e > best[m][1]:
                best[m] = (c.id, e)
    print(f"\nistft restatement: worst error / bound {worst[1]:.3f} at {worst[0]}")
    for m, (cid, e) in best.items():
        print(f"  mutant {m}: {e:.3g} at {cid}")
        assert e > 1.0, (m, e)


def test_gradient_restatement_is_inside_the_bound_and_every_mutant_leaves_it():
    worst, best = ("", 0.0), {m: ("", 0.0) for m in sg.GRAD_MUTANTS}
    for case in sg.GRAD:
        c, wav, g, ref = _grad(case.id)
        r = sg.grad_excess(c, ref, sg.grad_model(c, wav, g))
        assert r <= 1.0, (c.id, r)
        if r > worst[1]:
            worst = (c.id, r)
        if c.n_fft > 1100 and not c.lens:
            continue                                                                  # (the mutants show at the short lengths already)
        for m in sg.GRAD_MUTANTS:
            e = sg.grad_excess(c, ref, sg.grad_model(c, wav, g, m))
            if m == "truncating_count":
                assert (e > 1.0) == bool(c.lens), (c.id, e)                           # every ragged batch shows it, no dense case does
            if e > best[m][1] or (e == math.inf and best[m][1] != math.inf):
                best[m] = (c.id, e)
    print(f"\ngradient restatement: worst error / bound {worst[1]:.3f} at {worst[0]}")
    for m, (cid, e) in best.items():
        print(f"  mutant {m}: {e:.3g} at {cid}")
        assert e > 1.0, (m, e)


def test_zero_row_case_has_no_autograd_counterpart():
    """mag_eps = 0 on an all-zero row: autograd of sqrt(0) is not finite, the kernel's mag > 0 guard gives exactly 0"""
    c, wav, g, ref = _grad("g512_zero_row")
    y = wav[c.zero_row].double().clone().requires_grad_(True)
    (g[c.zero_row].double() * sg.mel64(y, c)).sum().backward()
    assert not bool(torch.isfinite(y.grad).all())
    out = sg.grad_model(c, wav, g)
    assert np.isfinite(out).all() and not out[c.zero_row].any() and out[1 - c.zero_row].any()


def test_gradient_cases_stay_clear_of_the_log_clamp():
    for case in sg.GRAD:
        if case.log_clip > 0:
            c, wav, _, _ = _grad(case.id)
            margin = sg.grad_clip_margin(c, wav)
            assert margin >= 1e-3, (c.id, margin)
