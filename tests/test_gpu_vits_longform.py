"""VITS at long-form lengths: no VITS kernel had run with a time axis above 400 columns, while a 12-second utterance at hop 256
has more than 1 024 frames -- the second row block of every element-wise kernel, expand_path over dozens of 64-frame blocks,
durations_kernel's running sum over long rows.

1. WN / PosteriorEncoder / ResidualCouplingBlock at the recipe's width, T = 1 100 and 2 500, against the oracle in fp64; every
   batch item against that item alone.
2. The same modules with every scratch tensor they allocate holding NaN beforehand: what lies beyond an utterance must not reach it.
3. ``SynthesizerTrn.infer`` on 420 tokens (up to 2 718 frames), compared stage by stage so that one flipped ceil can neither hide
   nor fake what follows it."""
import json
import math
import os
from functools import lru_cache

import pytest
import torch

from oracle import synth
from oracle import vits_infer_oracle as vio
from oracle import vocoder_oracle as vo

HERE = os.path.dirname(os.path.abspath(__file__))
gpu = pytest.mark.gpu
TOL = 1e-4                      # tests/test_gpu_vits.py
F64 = torch.float64
SHAPES = {"T1100": (1100, [1100, 1024]), "T2500": (2500, [2500, 1025, 7])}


def _mask(lens, T, dtype=torch.float32):
    return (torch.arange(T).view(1, 1, T) < torch.as_tensor(lens).view(-1, 1, 1)).to(dtype)


def _weights(gin):
    se = synth.synth_state_dict(synth.posterior_encoder_param_shapes(gin_channels=gin), 2468, g_gain=0.5)
    sf = synth.synth_state_dict(synth.coupling_block_param_shapes(gin_channels=gin), 1357, g_gain=0.5)
    return se, sf


def _modules(gin):
    from amphion_amd.models.tts.vits.vits import PosteriorEncoder, ResidualCouplingBlock

    se, sf = _weights(gin)
    enc = PosteriorEncoder(513, 192, 192, 5, 1, 16, gin_channels=gin)
    flow = ResidualCouplingBlock(192, 192, 5, 1, 4, gin_channels=gin)
    enc.load_state_dict(se)
    flow.load_state_dict(sf)
    return enc.cuda().eval(), flow.cuda().eval()


def _inputs(shape, gin):
    T, lens = SHAPES[shape]
    B = len(lens)
    gen = torch.Generator().manual_seed(T + gin)
    y = torch.rand(B, 513, T, generator=gen)
    noise = torch.randn(B, 192, T, generator=gen)
    g = torch.randn(B, gin, 1, generator=gen) if gin else None
    xw = torch.randn(B, 192, T, generator=gen) * _mask(lens, T)          # WN on its own
    return y, noise, g, xw, torch.tensor(lens)


@lru_cache(maxsize=None)
def _oracle(shape, gin):
    """fp64, once per (shape, gin): both arithmetic modes of the convs are held to the same reference"""
    y, noise, g, xw, lens = _inputs(shape, gin)
    se, sf = _weights(gin)
    g64 = g.double() if gin else None
    with torch.no_grad():
        z, m, logs, mask = vo.posterior_encoder_forward(se, "", y, lens, noise, dtype=F64, g=g64)
        z_p = vo.coupling_block_forward(sf, "", z, mask, dtype=F64, g=g64)
        z_hat = vo.coupling_block_forward(sf, "", z_p, mask, reverse=True, dtype=F64, g=g64)
        wn = vo.wn_forward(sf, "flows.0.enc", xw.double(), mask, 4, 192, 5, 1, F64, g=g64)
    return {"z": z, "m": m, "logs": logs, "z_p": z_p, "z_hat": z_hat, "wn": wn}


def _run(enc, flow, y, noise, g, lens):
    with torch.no_grad():
        z, m, logs, _ = enc(y, lens, g=g, noise=noise)
        z_p = flow(z, lens, g=g)
        z_hat = flow(z_p, lens, g=g, reverse=True)
    return {"z": z, "m": m, "logs": logs, "z_p": z_p, "z_hat": z_hat}


@gpu
@pytest.mark.parametrize("gin", [0, 256])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_posterior_side_long(shape, gin, conv_precision):
    T, lens_l = SHAPES[shape]
    y, noise, g, xw, lens = _inputs(shape, gin)
    enc, flow = _modules(gin)
    want = _oracle(shape, gin)
    gd = g.cuda() if gin else None
    valid = _mask(lens_l, T, torch.bool)
    # WN alone (the first coupling layer's, with its condition): fused and unfused, against fp64 and against each other
    wn = flow.flows[0].enc
    with torch.no_grad():
        y_f = wn(xw.cuda(), lens, g=gd)
        wn.fused = False
        y_u = wn(xw.cuda(), lens, g=gd)
        wn.fused = True
    e_f, e_u = ((t.cpu().double() - want["wn"]).abs().max().item() for t in (y_f, y_u))
    e_fu = (y_f - y_u).abs().max().item()
    print(f"\n[vits long] {shape} gin={gin} {conv_precision}: WN fused {e_f:.2e} unfused {e_u:.2e} fused-unfused {e_fu:.2e}")
    assert e_f <= TOL and e_u <= TOL and e_fu <= 2e-5
    assert (y_f.cpu()[~valid.expand_as(y_f)] == 0).all() and (y_u.cpu()[~valid.expand_as(y_u)] == 0).all()
    # posterior encoder -> flow -> flow reversed
    got = _run(enc, flow, y.cuda(), noise.cuda(), gd, lens)
    errs = {k: (got[k].cpu().double() - want[k]).abs().max().item() for k in got}
    print("[vits long] " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL, (k, v)
    assert ((got["z_hat"] - got["z"]).abs().cpu()[valid.expand_as(got["z"])]).max().item() <= TOL
    # every item is what it is alone (nothing beyond another utterance's end leaks into it) and zero beyond its own length
    for b, n in enumerate(lens_l):
        one = _run(enc, flow, y[b:b + 1, :, :n].cuda(), noise[b:b + 1, :, :n].cuda(), gd[b:b + 1] if gin else None, torch.tensor([n]))
        for k in got:
            assert (got[k][b, :, :n] - one[k][0]).abs().max().item() <= 2e-5, (k, b, n)
            assert (got[k][b, :, n:] == 0).all(), (k, b, n)


def _nan_pool(shapes, copies=48):
    """Fills what the caching allocator will hand out next with NaN: ``copies`` tensors of every shape the modules allocate are
    taken -- first the cached blocks the previous run freed (best fit), then fresh ones --, filled with NaN and freed again."""
    torch.cuda.synchronize()
    held = [torch.full(s, float("nan"), device="cuda") for s in shapes for _ in range(copies)]
    torch.cuda.synchronize()
    del held


@gpu
@pytest.mark.parametrize("gin", [0, 256])
def test_posterior_side_ignores_what_lies_beyond_an_utterance(gin, conv_precision):
    """The VITS counterpart of test_ragged_forward_ignores_what_lies_beyond_an_utterance: the scratch tensors of WN / the coupling
    layers are torch.empty, `pre` / `post` skip the tiles beyond an utterance and WN runs without its final mask, so beyond the
    lengths they hold whatever the memory held -- here NaN, on purpose.  The valid frames must stay finite and must not change."""
    T, lens_l = 1100, [1100, 1025, 7]
    gen = torch.Generator().manual_seed(31 + gin)
    B = len(lens_l)
    y = torch.rand(B, 513, T, generator=gen).cuda()
    noise = torch.randn(B, 192, T, generator=gen).cuda()
    g = torch.randn(B, gin, 1, generator=gen).cuda() if gin else None
    xw = (torch.randn(B, 192, T, generator=gen) * _mask(lens_l, T)).cuda()
    lens = torch.tensor(lens_l)
    enc, flow = _modules(gin)
    wn = flow.flows[0].enc

    def run():
        out = _run(enc, flow, y, noise, g, lens)
        with torch.no_grad():
            out["wn"] = wn(xw, lens, g=g)
            wn.fused = False
            out["wn_unfused"] = wn(xw, lens, g=g)
            wn.fused = True
        return {k: v.cpu() for k, v in out.items()}

    first = run()
    _nan_pool([(B, 192, T), (B, 384, T)])
    probes = [torch.empty(B, c, T, device="cuda") for c in (192, 384, 192, 384, 192, 192)]
    assert all(torch.isnan(p).all() for p in probes), "the allocator did not hand the poisoned memory back: this test would show nothing"
    del probes
    second = run()
    valid = _mask(lens_l, T, torch.bool).expand(B, 192, T)
    for k in first:
        assert torch.isfinite(second[k][valid]).all(), k
        assert torch.equal(second[k][valid], first[k][valid]), k
        assert (second[k][~valid] == 0).all(), k


# ---- SynthesizerTrn.infer on a long text ------------------------------------------------------------------------------------------
SMALL = dict(inter_channels=16, hidden_channels=32, filter_channels=64, n_heads=2, n_layers=2, kernel_size=3, p_dropout=0.1,
             resblock="1", resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]], upsample_rates=[4, 2],
             upsample_initial_channel=32, upsample_kernel_sizes=[8, 4])       # tests/test_gpu_vits_infer.py
VARIANTS = {"sdp": dict(n_speakers=0, gin_channels=0, use_sdp=True), "dp": dict(n_speakers=0, gin_channels=0, use_sdp=False)}
TEXT_LENS = [420, 301, 130]
LENGTH_SCALE, NOISE_SCALE, NOISE_SCALE_W = 1.0, 0.667, 0.8
LOGW_TOL = 5e-4                 # tests/test_gpu_vits_infer.py: "3 spline flows deep"
NEAR = math.exp(LOGW_TOL) - 1   # how far, relatively, a logw within LOGW_TOL can move exp(logw)


def _infer_weights(tag):
    with open(os.path.join(HERE, "golden", f"keys_vits_infer_{tag}.json")) as f:
        shapes = {k: tuple(s) for k, s in json.load(f)}
    return synth.synth_state_dict(shapes, 77, g_gain=0.5)


def _text_inputs():
    gen = torch.Generator().manual_seed(1)
    tokens = torch.randint(0, 40, (len(TEXT_LENS), max(TEXT_LENS)), generator=gen)
    noise_dp = torch.randn(len(TEXT_LENS), 2, max(TEXT_LENS), generator=gen)
    return tokens, torch.tensor(TEXT_LENS), noise_dp


@lru_cache(maxsize=None)
def _text_oracle(tag, dtype=F64):
    """text encoder + duration predictor of the oracle -> (enc_x, m, logs, x_mask, logw, w = exp(logw) * mask * length_scale)"""
    sd = {k: v.to(dtype) for k, v in _infer_weights(tag).items()}
    tokens, lens, noise_dp = _text_inputs()
    with torch.no_grad():
        x, m, logs, mask = vio.text_encoder(sd, "enc_p", tokens, lens, 32, 16, 2, 2, 3)
        if VARIANTS[tag]["use_sdp"]:
            logw = vio.stochastic_duration_predictor_reverse(sd, "dp", x, mask, noise_dp.to(dtype), NOISE_SCALE_W, 32, 3, 4)
        else:
            logw = vio.duration_predictor(sd, "dp", x, mask, 3)
    return x, m, logs, mask, logw, torch.exp(logw) * mask * LENGTH_SCALE


def _near_tokens(w):
    """tokens whose fp64 duration lies within a relative NEAR of an integer: the only ones whose ceil the logw bound lets differ"""
    r = torch.round(w)
    return (w - r).abs() <= NEAR * r.clamp_min(1)


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_long_text_inputs_meet_the_conditions(tag):
    """CPU: what the GPU comparison below presupposes holds in the oracle alone -- few tokens sit near an integer duration (at most
    2 % of the valid ones: a condition on the chosen seed, not a measurement), the oracle's own fp32 and fp64 runs agree on every
    duration, and the stochastic predictor's utterances cross one and two 1 024-frame row blocks."""
    _, _, _, mask, _, w = _text_oracle(tag)
    valid = mask.bool()
    assert int(_near_tokens(w)[valid].sum()) <= 0.02 * int(valid.sum())
    w32 = _text_oracle(tag, torch.float32)[5]
    assert torch.equal(torch.ceil(w32).double(), torch.ceil(w))
    frames = torch.ceil(w).sum(dim=(1, 2)).long().tolist()
    if tag == "sdp":
        assert frames == [2718, 1932, 1040]
    else:
        assert min(frames[:2]) > 1024


@gpu
@pytest.mark.parametrize("tag", list(VARIANTS))
def test_infer_long_text_stage_by_stage(tag, conv_precision):
    from amphion_amd.models.tts.vits.vits import SynthesizerTrn
    from amphion_amd.modules import hip_ops

    sd = _infer_weights(tag)
    net = SynthesizerTrn(40, 33, 8, **SMALL, **VARIANTS[tag])
    net.load_state_dict(sd)
    net = net.cuda().eval()
    tokens, lens, noise_dp = _text_inputs()
    B, Tx = tokens.shape
    rx, rm, rlogs, xmask, rlogw, rw = _text_oracle(tag)
    xv = xmask.bool()
    # 1. text encoder and duration predictor against fp64
    with torch.no_grad():
        h, m, logs, ld = net.enc_p(tokens.cuda(), lens)
        if VARIANTS[tag]["use_sdp"]:
            logw = net.dp(h, ld, g=None, reverse=True, noise_scale=NOISE_SCALE_W, noise=noise_dp.cuda())
        else:
            logw = net.dp(h, ld, g=None)
        w_ceil, cum, ylen = hip_ops.durations(logw, ld, LENGTH_SCALE)
    e = {k: (a.cpu().double() - b).abs().max().item() for k, a, b in (("enc_x", h, rx), ("m", m, rm), ("logs", logs, rlogs))}
    e["logw"] = ((logw.cpu().double() - rlogw) * xmask).abs().max().item()
    print(f"\n[vits long text] {tag} {conv_precision}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["enc_x"] <= 5e-5 and e["m"] <= 5e-5 and e["logs"] <= 5e-5 and e["logw"] <= LOGW_TOL
    for t in (h, m, logs):
        assert (t.cpu()[~xv.expand_as(t)] == 0).all()
    # 2. durations: exact, except that a token within NEAR of an integer may take either neighbour
    near = _near_tokens(rw)
    dur, want = w_ceil.cpu().double(), torch.ceil(rw)
    assert int(near[xv].sum()) <= 0.02 * int(xv.sum())
    assert torch.equal(dur[~near], want[~near])
    r = torch.round(rw)
    assert ((dur == r) | (dur == r + 1))[near].all()
    assert (dur[~xv] == 0).all()
    print(f"[vits long text] near tokens {int(near[xv].sum())} of {int(xv.sum())}, differing {int((dur != want).sum())}; "
          f"frames {ylen.tolist()}")
    assert torch.equal(cum.cpu().long(), torch.cumsum(dur[:, 0].long(), -1))
    assert torch.equal(ylen.cpu().long(), dur.sum(dim=(1, 2)).long().clamp_min(1))
    # 3. everything after the durations against the oracle's pieces fed the GPU's own w_ceil
    yl = ylen.cpu().long()
    ty = int(yl.max())
    noise_z = torch.randn(B, SMALL["inter_channels"], ty, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        o = net.infer(tokens.cuda(), lens, noise_scale=NOISE_SCALE, length_scale=LENGTH_SCALE, noise_scale_w=NOISE_SCALE_W,
                      noise_dp=noise_dp.cuda() if VARIANTS[tag]["use_sdp"] else None, noise_z=noise_z.cuda())
    ymask = _mask(yl, ty, F64)
    path = vio.generate_path(dur, xmask.unsqueeze(2) * ymask.unsqueeze(-1))
    assert torch.equal(o["attn"].cpu().double(), path)                                   # the very durations of step 2, bit for bit
    assert torch.equal(o["mask"].cpu().double(), ymask)
    sd64 = {k: v.double() for k, v in sd.items()}
    hp = dict(SMALL)
    with torch.no_grad():
        m_p = torch.matmul(path.squeeze(1), rm.transpose(1, 2)).transpose(1, 2)
        logs_p = torch.matmul(path.squeeze(1), rlogs.transpose(1, 2)).transpose(1, 2)
        z_p = m_p + noise_z.double() * torch.exp(logs_p) * NOISE_SCALE
        z = vo.coupling_block_forward(vio._sub(sd64, "flow."), "", z_p, ymask, reverse=True, channels=16, hidden=32, dtype=F64)
        y_hat = vo.hifigan_forward(vio._sub(sd64, "dec."), hp, z * ymask, dtype=F64)
    errs = {}
    for k, ref_t, tol in (("m_p", m_p, 5e-5), ("logs_p", logs_p, 5e-5), ("z_p", z_p, TOL), ("z", z, TOL)):
        assert o[k].shape == ref_t.shape, k
        errs[k] = ((o[k].cpu().double() - ref_t) * ymask).abs().max().item()
        assert errs[k] <= tol, (k, errs[k])
    hop = 8
    assert o["y_hat"].shape == y_hat.shape
    smask = _mask(yl * hop, ty * hop, F64)
    errs["y_hat"] = ((o["y_hat"].cpu().double() - y_hat) * smask).abs().max().item()
    print("[vits long text] " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["y_hat"] <= TOL
