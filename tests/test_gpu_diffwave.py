"""DiffWave on the MI355X (csrc/dw_layer_f16x3.hip, csrc/diffwave.hip) against the fp64 restatement of tests/diffwave_ref.py and the
golden outputs of the real reference classes, in both arithmetics (the `conv_precision` fixture).

Layer bound (derived, as tests/test_recipe_numerics.py does): a split-f16 product term is exact to 2^-22 of |w||v| and the fp32
accumulation adds a few 2^-24 of the partial sums, so a pre-activation is off by at most tol1 = 2e-6 * sum|w||v| + 3e-7 * |sum|.
|d sigmoid| <= 1/4, |d tanh| <= 1, both factors <= 1:  |d(sigmoid * tanh)| <= tol1_gate / 4 + tol1_filter, plus 5e-7 for the two fp32
library functions (<= 2 ulp of a value <= 1 each) and the product's rounding.  Through GEMM 2: sum|w2| * that + 2e-6 * sum|w2||z| + 3e-7 |r|.
The epilogue adds, divides and stores in fp32: 3 roundings of 2^-24 relative to the operands."""
import ctypes
import os
import subprocess
import sys
from math import sqrt

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diffwave_ref as D  # noqa: E402
from test_oracle_diffwave import sampler_case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def make_model(hp, sd):
    from amphion_amd.models.vocoders.diffusion.diffwave.diffwave import DiffWave

    m = DiffWave(D.make_cfg(**hp))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def op_layer(m, i, x, cond, dconst, skip_in):
    """amp_dw_layer on raw pointers: dconst [S, C] (S = 1: shared)"""
    from amphion_amd import _lib

    B, C, L = x.shape
    x_out, skip_out = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.lib().amp_dw_layer(m.handle(x.device), i, _p(x), _p(cond), _p(dconst), 0 if dconst.shape[0] == 1 else C, _p(skip_in),
                                       _p(x_out), _p(skip_out), B, L, _lib.current_stream_ptr(x.device)))
    return x_out, skip_out


def layer_bounds(sd64, i, d, x, dc, cond, skip_in):
    """fp64 outputs of one layer and the derived bound of each output element"""
    p = f"residual_layers.{i}."
    rec = {}
    x_out, skip = D.layer(sd64, i, d, x, dc, cond, rec)
    wd, wc, w2 = sd64[p + "dilated_conv.weight"].abs(), sd64[p + "conditioner_projection.weight"].abs(), sd64[p + "output_projection.weight"].abs()
    mag1 = F.conv1d(rec["y"].abs(), wd, padding=d, dilation=d) + F.conv1d(cond.abs(), wc) \
        + sd64[p + "dilated_conv.bias"].abs()[None, :, None] + sd64[p + "conditioner_projection.bias"].abs()[None, :, None]
    tol1 = 2e-6 * mag1 + 3e-7 * rec["a"].abs()
    tg, tf = torch.chunk(tol1, 2, dim=1)
    dz = tg / 4 + tf + 5e-7
    dr = F.conv1d(dz, w2) + 2e-6 * (F.conv1d(rec["z"].abs(), w2) + sd64[p + "output_projection.bias"].abs()[None, :, None]) + 3e-7 * rec["r"].abs()
    dres, dskip = torch.chunk(dr, 2, dim=1)
    res, sk = torch.chunk(rec["r"], 2, dim=1)
    tol_x = (dres + 1.2e-7 * (x.abs() + res.abs())) / sqrt(2.0) + 1.2e-7 * x_out.abs()
    tol_s = dskip + 1.2e-7 * sk.abs()
    if skip_in is not None:
        skip = skip + skip_in
        tol_s = tol_s + 1.2e-7 * (skip.abs() + skip_in.abs())
    return x_out, skip, tol_x, tol_s


def layer_inputs(C, n_mel, B, L, seed, per_item):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, L, generator=g).relu()
    cond = torch.randn(B, n_mel, L, generator=g)
    dc = 0.5 + torch.randn(B if per_item else 1, C, generator=g)      # a non-zero constant: wrong padding of y shows by O(1)
    skip_in = torch.randn(B, C, L, generator=g)
    return x, cond, dc, skip_in


def check_layer(m, sd64, i, d, x, cond, dc, skip_in):
    xo, so = op_layer(m, i, x.to(DEV), cond.to(DEV), dc.to(DEV), None if skip_in is None else skip_in.to(DEV))
    rx, rs, tx, ts = layer_bounds(sd64, i, d, x.double(), dc.double(), cond.double(), None if skip_in is None else skip_in.double())
    ex, es = (xo.cpu().double() - rx).abs(), (so.cpu().double() - rs).abs()
    print(f"layer d={d} L={x.shape[2]} B={x.shape[0]}: x_out err/tol max {float((ex / tx).max()):.3f}, skip {float((es / ts).max()):.3f}; "
          f"max err {float(ex.max()):.2e} {float(es.max()):.2e}")
    assert bool((ex <= tx).all()) and bool((es <= ts).all())
    # the zero-padding zone (columns within d of either end): the tap outside [0, L) contributes 0, not the diffusion constant
    L = x.shape[2]
    zone = torch.zeros(L, dtype=torch.bool)
    zone[: min(d, L)] = True
    zone[max(0, L - d):] = True
    assert bool((ex[:, :, zone] <= tx[:, :, zone]).all())


@pytest.fixture(scope="module")
def nets():
    out = {}
    for C, n_mel in ((64, 80), (64, 100), (32, 80), (128, 100)):
        hp = dict(C=C, N=10, cycle=10, n_mel=n_mel, u=(16, 16))
        out[(C, n_mel)] = (hp, D.synth_state_dict(C, 10, n_mel, (16, 16), 60 + C + n_mel))
    return out


@pytest.mark.parametrize("i", range(10))
def test_layer_every_dilation(conv_precision, nets, i):
    d = 1 << i
    hp, sd = nets[(64, 80)]
    m, sd64 = make_model(hp, sd), D.to_dtype(sd, torch.float64)
    from amphion_amd import _lib

    for L in sorted({1, max(1, d - 1), d, d + 1, 63, 64, 65, 8192}):
        x, cond, dc, skip_in = layer_inputs(64, 80, 3 if L <= 65 else 1, L, 100 * i + L % 97, per_item=L % 2 == 1)
        check_layer(m, sd64, i, d, x, cond, dc, skip_in if L % 3 else None)
    _lib.range_check(DEV)


@pytest.mark.parametrize("C,n_mel,B,L", [(64, 80, 3, 65536), (64, 100, 1, 8192), (32, 80, 3, 8192), (128, 100, 1, 8192), (32, 80, 1, 65), (128, 100, 3, 63)])
def test_layer_widths_mels_and_batches(conv_precision, nets, C, n_mel, B, L):
    hp, sd = nets[(C, n_mel)]
    m, sd64 = make_model(hp, sd), D.to_dtype(sd, torch.float64)
    for i in (0, 9) if L < 65536 else (9,):
        x, cond, dc, skip_in = layer_inputs(C, n_mel, B, L, C + L + i, per_item=True)
        check_layer(m, sd64, i, 1 << i, x, cond, dc, skip_in if i else None)


def _peak_rel(got, ref):
    return float((got.cpu().double() - ref).abs().max() / ref.abs().max())


def test_small_kernels(conv_precision, nets):
    from amphion_amd import _lib

    hp, sd = nets[(64, 100)]
    m, sd64 = make_model(hp, sd), D.to_dtype(sd, torch.float64)
    L_ = _lib.lib()
    st = _lib.current_stream_ptr(torch.device(DEV))
    mel = D.synth_mel(2, 100, 7, 3)
    assert _peak_rel(m.condition(mel.to(DEV)), D.upsample(sd64, hp["u"], mel.double())) <= 2e-6
    table = D.embedding_table(50)
    h = m.handle(torch.device(DEV))
    for steps in (torch.tensor([7]), torch.tensor([0, 49, 13]), torch.tensor([10.452]), torch.tensor([0.0, 48.5, 22.992])):
        ref = D.dconst_table(sd64, 10, D.embed(sd64, table, steps if steps.dtype == torch.int64 else steps.double()))
        out = torch.empty(ref.shape, dtype=torch.float32, device=DEV)
        _lib.check(L_.amp_dw_embed(h, _p(steps.float().to(DEV)), steps.numel(), _p(out), st))
        assert _peak_rel(out, ref) <= 2e-6
    g = torch.Generator().manual_seed(9)
    audio, skip = torch.randn(2, 1000, generator=g), 3 * torch.randn(2, 64, 1000, generator=g)
    x = torch.empty(2, 64, 1000, device=DEV)
    _lib.check(L_.amp_dw_input(h, _p(audio.to(DEV)), 2, 1000, _p(x), st))
    assert _peak_rel(x, F.relu(F.conv1d(audio.double().unsqueeze(1), sd64["input_projection.weight"], sd64["input_projection.bias"]))) <= 2e-6
    eps = torch.empty(2, 1000, device=DEV)
    _lib.check(L_.amp_dw_tail(h, _p(skip.to(DEV)), 2, 1000, _p(eps), st))
    assert _peak_rel(eps, D.tail(sd64, 10, skip.double()).squeeze(1)) <= 2e-6


def test_forward_matches_the_reference_class_golden(conv_precision):
    z = np.load(os.path.join(GOLDEN, "golden_diffwave.npz"))
    for tag, hp in (("small", D.SMALL), ("wide", D.WIDE)):
        sd = D.synth_state_dict(hp["C"], hp["N"], hp["n_mel"], hp["u"], int(z[f"{tag}_seed"]), out_gain=D.OUT_GAIN[tag])
        m = make_model(hp, sd)
        mel, audio = torch.from_numpy(z[f"{tag}_mel"]).to(DEV), torch.from_numpy(z[f"{tag}_audio"]).to(DEV)
        for key, step in (("y_int", torch.tensor([7], device=DEV)), ("y_flt", torch.tensor([10.452], device=DEV))):
            y = m(audio, step, mel)
            ref = torch.from_numpy(z[f"{tag}_{key}"])
            assert y.shape == ref.shape
            err = float((y.cpu() - ref).abs().max())
            print(f"golden {tag} {key}: {err:.2e}")
            assert err <= 1e-4
        y2 = m(audio, torch.tensor([7], device=DEV), mel)
        assert y2.data_ptr() != y.data_ptr()                     # a fresh output tensor per call


def test_forward_recipe_size_against_fp64(conv_precision):
    hp = D.RECIPE
    sd = D.synth_state_dict(hp["C"], hp["N"], hp["n_mel"], hp["u"], 53, out_gain=D.OUT_GAIN["recipe"])
    m = make_model(hp, sd)
    mel = D.synth_mel(2, 80, 32, 56)
    g = torch.Generator().manual_seed(57)
    audio = torch.randn(2, 8192, generator=g)
    table = D.embedding_table(50)
    step = torch.tensor([22.992, 3.0])
    ref = D.forward(D.to_dtype(sd, torch.float64), hp, table, audio, step.double(), mel=mel)
    t32 = D.forward(sd, hp, table, audio, step, mel=mel)
    y = m(audio.to(DEV), step.to(DEV), mel.to(DEV)).cpu()
    err, err32 = float((y.double() - ref).abs().max()), float((t32.double() - ref).abs().max())
    print(f"recipe forward vs fp64: ours {err:.2e}, torch fp32 {err32:.2e}, rms {float(ref.pow(2).mean().sqrt()):.3f}")
    assert err <= 1e-4
    # bitwise: repeatable; forward == condition + embed + input + per-layer op-level calls + tail chained by hand
    assert torch.equal(m(audio.to(DEV), step.to(DEV), mel.to(DEV)).cpu(), y)
    from amphion_amd import _lib

    L_ = _lib.lib()
    dev = torch.device(DEV)
    st = _lib.current_stream_ptr(dev)
    h = m.handle(dev)
    cond = m.condition(mel.to(DEV))
    dc = torch.empty(2, 30, 64, device=DEV)
    _lib.check(L_.amp_dw_embed(h, _p(step.to(DEV)), 2, _p(dc), st))
    x = torch.empty(2, 64, 8192, device=DEV)
    _lib.check(L_.amp_dw_input(h, _p(audio.to(DEV)), 2, 8192, _p(x), st))
    skip = None
    for i in range(30):
        xo, so = torch.empty_like(x), torch.empty_like(x)
        _lib.check(L_.amp_dw_layer(h, i, _p(x), _p(cond), _p(dc[:, i].contiguous()), 64, _p(skip), _p(xo), _p(so), 2, 8192, st))
        x, skip = xo, so
    eps = torch.empty(2, 8192, device=DEV)
    _lib.check(L_.amp_dw_tail(h, _p(skip), 2, 8192, _p(eps), st))
    assert torch.equal(eps.cpu(), y[:, 0])
    # a batch row does not depend on what it is batched with
    y0 = m(audio[:1].to(DEV), step[:1].to(DEV), mel[:1].to(DEV)).cpu()
    assert torch.equal(y0, y[:1])


@pytest.mark.parametrize("tag,kind,Fs", [("recipe", "fast", 32), ("small", "full", 24), ("wide", "fast", 1)])
def test_sampler_against_fp64(conv_precision, tag, kind, Fs):
    """bound: max(1e-4, 4 x the distance of the fp32 torch restatement from fp64 on the same case) -- 50 compositions of a network
    with a clamp cannot be derived; 4 is the factor DESIGN.md 3.0 shows between the reference's fp32 run and this library's
    arithmetics end to end, rounded up"""
    from amphion_amd.models.vocoders.diffusion.diffusion_vocoder_inference import vocoder_inference

    hp, cfg, sd, mel, noise = sampler_case(tag, kind, Fs)
    table = D.embedding_table(50)
    fast = kind == "fast"
    ref = D.sample(D.to_dtype(sd, torch.float64), hp, table, cfg, mel, noise, fast)
    d32 = float((D.sample(sd, hp, table, cfg, mel, noise, fast).double() - ref).abs().max())
    m = make_model(hp, sd)
    wav = vocoder_inference(m.cfg, m, mel, device=DEV, fast_inference=fast, noise=noise)
    assert wav.device.type == "cpu" and tuple(wav.shape) == tuple(ref.shape)
    err = float((wav.double() - ref).abs().max())
    print(f"sampler {tag} {kind}: ours {err:.3e}, torch fp32 {d32:.3e}, bound {max(1e-4, 4 * d32):.3e}")
    assert err <= max(1e-4, 4 * d32)
    # bitwise: two runs equal; a batch equals its items run alone with the same noise rows
    assert torch.equal(vocoder_inference(m.cfg, m, mel, device=DEV, fast_inference=fast, noise=noise), wav)
    if mel.shape[0] > 1:
        for b in range(mel.shape[0]):
            one = vocoder_inference(m.cfg, m, mel[b:b + 1], device=DEV, fast_inference=fast, noise=[n[b:b + 1] for n in noise])
            assert torch.equal(one, wav[b:b + 1])


def test_range_guard_and_fp32_repeat():
    from amphion_amd import _lib
    from amphion_amd.models.vocoders.diffusion.diffusion_vocoder_inference import vocoder_inference

    hp, cfg, sd, mel, noise = sampler_case("small", "fast", 24)
    big = [n.clone() for n in noise]
    big[0][0, 100] = 1e5
    _lib.set_precision("f16x3")
    m = make_model(hp, sd)
    with pytest.raises(_lib.AmpError) as e:
        m(big[0].to(DEV), torch.tensor([3], device=DEV), mel.to(DEV))
    assert e.value.status == _lib.AMP_ERR_RANGE
    wav = vocoder_inference(m.cfg, m, mel, device=DEV, fast_inference=True, noise=big)
    assert bool(torch.isfinite(wav).all())
    assert _lib.lib().amp_dw_precision(m.handle(torch.device(DEV))) == _lib.AMP_PRECISION_F16X3
    _lib.set_precision("f32")
    try:
        m32 = make_model(hp, sd)
        ref = vocoder_inference(m32.cfg, m32, mel, device=DEV, fast_inference=True, noise=big)
    finally:
        _lib.set_precision("f16x3")
    assert torch.equal(wav, ref)


_MANIFEST = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
import diffwave_ref as D
from amphion_amd import _lib
from amphion_amd.models.vocoders.diffusion.diffwave.diffwave import DiffWave
_lib.set_precision(sys.argv[2])
hp = D.SMALL
m = DiffWave(D.make_cfg(**hp))
m.load_state_dict(D.synth_state_dict(hp["C"], hp["N"], hp["n_mel"], hp["u"], 1))
m = m.to("cuda:0").eval()
y = m(torch.randn(2, 160, device="cuda:0"), torch.tensor([3], device="cuda:0"), torch.randn(2, 80, 10, device="cuda:0"))
torch.cuda.synchronize()
print("DONE")
'''


def test_launch_manifest(conv_precision, tmp_path):
    out = tmp_path / "manifest.tsv"
    env = dict(os.environ, AMP_LAUNCH_MANIFEST=str(out), PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _MANIFEST, os.path.join(ROOT, "tests"), conv_precision], env=env, capture_output=True, text=True, timeout=300)
    assert "DONE" in r.stdout, r.stdout + r.stderr
    lines = [ln.split("\t") for ln in out.read_text().splitlines()]
    name = "dw_layer_f16x3_kernel" if conv_precision == "f16x3" else "dw_layer_f32_kernel"
    layers = [ln for ln in lines if ln[0].startswith(name)]
    hp = D.SMALL
    assert len(layers) == hp["N"]
    C, n_mel = hp["C"], hp["n_mel"]
    flop = (2 * (3 * C + n_mel) * 2 * C + 2 * C * 2 * C) * 2 * 160
    assert all(abs(float(ln[2]) * 1e9 - flop) <= 1e-3 * flop for ln in layers)
    if conv_precision == "f32":
        assert not any("f16x3" in ln[0] for ln in lines)
    assert {ln[0].split("<")[0] for ln in lines} >= {"dw_upsample_kernel", "dw_embed_kernel", "dw_input_kernel", "dw_tail_kernel", name}


def test_refusals(conv_precision):
    from amphion_amd import _lib
    from amphion_amd.models.vocoders.diffusion.diffwave.diffwave import DiffWave

    hp = D.SMALL
    sd = D.synth_state_dict(hp["C"], hp["N"], hp["n_mel"], hp["u"], 1)
    m = make_model(hp, sd)
    mel, audio, step = torch.randn(1, 80, 10, device=DEV), torch.randn(1, 160, device=DEV), torch.tensor([3], device=DEV)
    with pytest.raises(RuntimeError):
        m(audio.cpu(), step, mel)
    with pytest.raises(RuntimeError):
        m(audio, step, mel.cpu())
    with pytest.raises(ValueError):
        m(audio, step, torch.randn(1, 100, 10, device=DEV))          # wrong n_mel
    with pytest.raises(ValueError):
        m(torch.randn(1, 161, device=DEV), step, mel)               # L != hop * F
    with pytest.raises(IndexError):
        m(audio, torch.tensor([50], device=DEV), mel)
    bad = DiffWave(D.make_cfg(**dict(hp, hop=256)))
    bad.load_state_dict(sd)
    with pytest.raises(ValueError):
        bad.to(DEV)(audio, step, mel)                               # hop_size != u0 * u1
    odd = DiffWave(D.make_cfg(**dict(hp, C=48)))
    with pytest.raises(_lib.AmpError):
        odd.to(DEV).handle(torch.device(DEV))                       # C % 32 != 0
    x = torch.zeros(1, 32, 160, device=DEV)
    with pytest.raises(_lib.AmpError):                              # x aliasing x_out
        _lib.check(_lib.lib().amp_dw_layer(m.handle(torch.device(DEV)), 0, _p(x), _p(torch.zeros(1, 80, 160, device=DEV)), _p(torch.zeros(32, device=DEV)), 0,
                                           None, _p(x), _p(torch.zeros_like(x)), 1, 160, None))
    _lib.range_check(DEV)
