"""amp_istft_forward / amp_istft_same / amp_istft_same_polar and amp_mel_backward (dense and ragged) over their documented geometry, and the
ragged forward on every kernel form, through the C ABI against fp64.  tests/stft_geometry.py holds the tables and references;
tests/test_stft_geometry_ref.py shows on the CPU what they reach and that the bounds below catch a kernel with one slip.

No new tolerance:
  inverse STFT     |err[m]| <= 2e-5 c max(1, max |num64|) / den[m]: num64 the fp64 overlap-add, c = n_fft / hop (forward) or 1 (same), den the
                   float32 wss / envelope value where the kernel divides and 1 where it does not (test_stft_inverse_any_smooth_nfft's 2e-5,
                   which this reduces to where den is flat)
  same_polar       also against amp_istft_same fed the torch-formed (re, im): 1e-5 x peak (test_gpu_vocos.py)
  dense gradient   max |err| <= 1e-4 max |ref| for a smooth upstream gradient (test_mel_gradient_of_a_plain_sum); the sign pattern of an L1
                   loss: max 2e-3 and mean 2e-5 of scale (test_mel_loss_value_and_gradient)
  ragged rows      bit-equal to the utterance run alone; frames at and beyond a row's own count untouched (forward) and unread (backward:
                   they hold NaN); zero-frame rows and columns beyond a length exactly 0
Every output lies between sentinels; frames_ws and spec_ws are exactly the documented size with a sentinel behind them.  The largest
error / bound of each case is printed."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import stft_geometry as sg  # noqa: E402

pytestmark = pytest.mark.gpu
FINITE_SENTINEL = -12345.5


def _H():
    import hip_helpers as H

    return H


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


# ---- inverse STFT -----------------------------------------------------------------------------------------------------------
def _run_istft(c, inp, mode=None, ab=None, offset=None):
    """one call of the case's entry point (or of `mode` on the (re, im) pair `ab`); -> wav [B, Lout] on the device, all fences checked"""
    H = _H()
    mode = mode or c.mode
    d = H.mel_desc(c.n_fft, c.win, c.hop, 0, 1)
    window = torch.from_numpy(sg.ist_window32(c)).cuda()
    den = torch.from_numpy(sg.ist_den32(c)).cuda()
    wav = H.Fenced((c.B, c.Lout))
    frames = H.Fenced((c.B * c.F * c.n_fft,), offset=c.offset if offset is None else offset)        # exactly the documented size
    assert frames.buf.numel() * 4 <= sg.DEVICE_TENSOR_CAP
    if ab is not None:
        a, b, kw = ab[0], ab[1], {}
    elif c.form == "polar":
        a, b, kw = inp["mag"].cuda(), inp["phase"].cuda(), {}
    elif c.form == "reim":
        a, b, kw = inp["re"].cuda(), inp["im"].cuda(), {}
    else:
        a, b, kw = inp["head"].cuda(), None, dict(stride=inp["stride"], clip=inp["clip"])
    st = H.istft_call(mode, d, a, b, c.B, c.F, window, den, frames, wav, **kw)
    assert st == sg.AMP_OK, (c.id, st, H.last_error())
    frames.check_written(f"{c.id}: frames_ws")
    return wav.check_written(f"{c.id}: wav")


@pytest.mark.parametrize("name", [c.id for c in sg.ISTFT])
def test_istft_geometry(conv_precision, name):
    c, inp, ref = _ist(name)
    out = _run_istft(c, inp)
    r = sg.ist_excess(ref, out)
    print(f"    {c.id} [{conv_precision}]: error / bound {r:.4f}")
    assert r <= 1.0, (c.id, r)
    if c.offset:
        # the documented fallback of unaligned scratch (the mixed-radix kernel) against the aligned run (the wave kernel), same bound
        twin = _run_istft(c, inp, offset=0)
        d = ((out.double() - twin.double()).abs().cpu() / sg.ist_bound(ref)[None, :]).max().item()
        print(f"    {c.id}: against the aligned run {d:.4f}")
        assert d <= 1.0, (c.id, d)
    if c.id in sg.POLAR_SPLIT_CASES:
        h = inp["head"].cuda()[:, :2 * c.bins * c.F].reshape(c.B, 2 * c.bins, c.F)
        mag = torch.clip(torch.exp(h[:, :c.bins]), max=inp["clip"])
        re, im = (mag * torch.cos(h[:, c.bins:])).contiguous(), (mag * torch.sin(h[:, c.bins:])).contiguous()
        split = _run_istft(c, inp, mode="same", ab=(re, im))
        peak = float(ref["out"].abs().max())
        diff = (out - split).abs().max().item()
        print(f"    {c.id}: against amp_istft_same on the torch-formed spectrum {diff:.2e} (peak {peak:.2f})")
        assert diff <= sg.POLAR_SPLIT * max(peak, 1.0), (c.id, diff, peak)


@pytest.mark.parametrize("rid", [r[0] for r in sg.REFUSALS])
def test_istft_refusals(rid):
    """status, a message naming the entry point, nothing launched: scratch and output keep their sentinels"""
    H = _H()
    _, mode, change, status = next(r for r in sg.REFUSALS if r[0] == rid)
    p = dict(sg.REFUSAL_BASE)
    p.update({k: v for k, v in change.items() if k in p})
    d = H.mel_desc(p["n_fft"], p["win"], p["hop"], 0, 1)
    room = 1 << 16
    t = {k: torch.ones(room, device="cuda") for k in ("a", "b", "window", "den")}
    t["frames"], t["wav"] = H.Fenced((room,)), H.Fenced((room,))
    if "null" in change:
        t[change["null"]] = None
    rows = 2 * (p["n_fft"] // 2 + 1)
    stride = rows * p["F"] + change.get("stride", 0)
    st = H.istft_call(mode, d, t["a"], t["b"], p["B"], p["F"], t["window"], t["den"], t["frames"], t["wav"], stride=stride,
                      clip=change.get("clip", 100.0))
    msg = H.last_error()
    assert st == status, (rid, st, msg)
    assert msg.strip() and "amp_istft_" + mode in msg, (rid, msg)
    torch.cuda.synchronize()
    for k in ("frames", "wav"):
        if t[k] is not None:
            t[k].check_fences(rid)
            assert bool(torch.isnan(t[k].t).all()), (rid, k)


# ---- ragged forward ---------------------------------------------------------------------------------------------------------
def _forward(d, wav, lens, F, n_mel, bins, fill):
    H = _H()
    B, Ln = wav.shape
    outs = {"mel": H.Fenced((B, n_mel, F), fill=fill), "mag": H.Fenced((B, bins, F), fill=fill), "re": H.Fenced((B, bins, F), fill=fill),
            "im": H.Fenced((B, bins, F), fill=fill)}
    return outs, (lambda window, basis: H.mel_forward_call(d, wav, lens, B, Ln, window, basis, outs["mel"], outs["mag"], outs["re"], outs["im"]))


@pytest.mark.parametrize("n_fft,hop,n_mel,form", sg.RAGGED_FWD)
def test_ragged_forward_every_kernel_form(n_fft, hop, n_mel, form):
    """zero-frame rows untouched, every row untouched from its own frame count on, the frames below bit-equal to the utterance alone"""
    from amphion_amd import _lib
    import ctypes

    H = _H()
    lens = sg.ragged_fwd_lens(n_fft, hop)
    B, Ln, bins = len(lens), lens[0], n_fft // 2 + 1
    gen = torch.Generator().manual_seed(n_fft + hop)
    wav = (torch.rand(B, Ln, generator=gen) * 2 - 1) * 0.7
    for b, n in enumerate(lens):
        wav[b, n:] = 0.0
    wav = wav.cuda()
    d = H.mel_desc(n_fft, n_fft, hop, n_mel, 0, 1e-9, 1e-5)
    window = torch.hann_window(n_fft).cuda()
    basis = torch.from_numpy(sg.vo.mel_filterbank(sg.SR, n_fft, n_mel, 0, None)).cuda()
    count = lambda n: _lib.lib().amp_mel_num_frames(ctypes.byref(d), n)  # noqa: E731
    F = count(Ln)
    outs, call = _forward(d, wav, torch.tensor(lens, dtype=torch.int32).cuda(), F, n_mel, bins, FINITE_SENTINEL)
    assert call(window, basis) == sg.AMP_OK, H.last_error()
    torch.cuda.synchronize()
    counts = [count(n) for n in lens]
    assert counts == [sg.row_frames(n, n_fft, hop) for n in lens] and counts[1] == 0 and counts[3] == 0 and counts[0] == F
    for b, (n, k) in enumerate(zip(lens, counts)):
        solo = None
        if k:
            solo, call1 = _forward(d, wav[b:b + 1, :n].contiguous(), None, k, n_mel, bins, FINITE_SENTINEL)
            assert call1(window, basis) == sg.AMP_OK, H.last_error()
        for name, o in outs.items():
            o.check_fences(f"{form} {n_fft}/{hop} {name}")
            tail = o.t[b, :, k:]
            assert bool((tail == FINITE_SENTINEL).all()), (f"{form} {n_fft}/{hop}: row {b} ({n} samples, {k} frames) of `{name}` was written at frame "
                                                           f"{k + int((tail != FINITE_SENTINEL).any(0).nonzero()[0])}")
            if k:
                got, want = o.t[b, :, :k], solo[name].check_written(f"{form} {n_fft}/{hop} {name} alone")[0]
                assert torch.equal(got, want), (form, n_fft, hop, name, b, (got - want).abs().max().item())


# ---- mel gradient -----------------------------------------------------------------------------------------------------------
def _backward(c, wav, g, lens=None, poison=True):
    """forward with log_clip <= 0 (what amp_mel_backward documents as its inputs), NaN into every frame at and beyond a row's own count, backward.
    -> grad_wav [B, L] on the device; workspaces exactly the documented size, all fences checked"""
    H = _H()
    B, Ln = wav.shape
    F = sg.num_frames(Ln, c.n_fft, c.hop, c.pad_mode)
    window, basis = sg.grad_window32(c).cuda(), torch.from_numpy(sg.grad_basis32(c)).cuda()
    dl = None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()
    outs, call = _forward(H.mel_desc(c.n_fft, c.n_fft, c.hop, c.n_mel, c.pad_mode, c.mag_eps, 0.0), wav, dl, F, c.n_mel, c.bins, float("nan"))
    assert call(window, basis) == sg.AMP_OK, H.last_error()
    torch.cuda.synchronize()
    g = g.clone()
    if lens is not None and poison:
        for b, n in enumerate(lens):
            k = sg.row_frames(n, c.n_fft, c.hop, c.pad_mode)
            g[b, :, k:] = float("nan")
            for o in outs.values():
                o.t[b, :, k:] = float("nan")
    spec_ws, frames_ws, gw = H.Fenced((2 * B * c.bins * F,)), H.Fenced((B * F * c.n_fft,)), H.Fenced((B, Ln))
    assert max(spec_ws.buf.numel(), frames_ws.buf.numel(), gw.buf.numel()) * 4 <= sg.DEVICE_TENSOR_CAP
    d = H.mel_desc(c.n_fft, c.n_fft, c.hop, c.n_mel, c.pad_mode, c.mag_eps, c.log_clip)
    st = H.mel_backward_call(d, dl, B, Ln, window, basis, outs["mel"], outs["mag"], outs["re"], outs["im"], g.cuda(), spec_ws, frames_ws, gw)
    assert st == sg.AMP_OK, (c.id, st, H.last_error())
    for o in list(outs.values()) + [spec_ws, frames_ws]:
        o.check_fences(c.id)
    gw.check_fences(c.id)
    assert not bool(torch.isnan(gw.t).any()), (c.id, "grad_wav holds NaN: unwritten, or a frame beyond a row's own count was read",
                                               torch.isnan(gw.t).any(1).nonzero().flatten().tolist())
    return gw.t


@pytest.mark.parametrize("name", [c.id for c in sg.GRAD if c.lens is None])
def test_mel_backward_dense(conv_precision, name):
    c, wav, g, ref = _grad(name)
    out = _backward(c, wav.cuda(), g)
    r = sg.grad_excess(c, ref, out)
    print(f"    {c.id} [{conv_precision}]: error / bound {r:.4f}")
    assert r <= 1.0, (c.id, r)
    if c.zero_row is not None:
        assert not bool(out[c.zero_row].any()) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("name", [c.id for c in sg.GRAD if c.lens is not None])
def test_mel_backward_ragged(conv_precision, name):
    c, wav, g, ref = _grad(name)
    out = _backward(c, wav.cuda(), g, lens=c.lens)
    for b, (n, k) in enumerate(zip(c.lens, c.counts())):
        assert not bool(out[b, n:].any()), (c.id, b, "columns beyond the length")
        if k == 0:
            assert not bool(out[b].any()), (c.id, b, "a zero-frame row")
            continue
        solo = _backward(c, wav[b:b + 1, :n].contiguous().cuda(), g[b:b + 1, :, :k].contiguous())
        assert torch.equal(out[b, :n], solo[0]), (c.id, b, (out[b, :n] - solo[0]).abs().max().item())
    r = sg.grad_excess(c, ref, out)
    print(f"    {c.id} [{conv_precision}]: error / bound {r:.4f}")
    assert r <= 1.0, (c.id, r)
