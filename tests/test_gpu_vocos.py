"""Vocos on the MI355X (amphion_amd/models/codec/amphion_codec/vocos.py) against fp64, in both arithmetics.

- the pointwise GEMM (amp_pw_forward), each epilogue, at every layer shape of the three Vocos configurations and a ragged
  small one, against fp64 with the op-level bound 2e-6 * sum |w||x| (tests/test_recipe_numerics.py derives it);
- which kernel ran (the launch manifest, in a child process), and the f16x3 range flag;
- the fused depthwise k = 7 + LayerNorm, the polar ISTFT head (amp_istft_same_polar);
- the drop-in end to end against tests/vocos_ref.py and the golden outputs of the real reference class; determinism.
Reads no file of the reference.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vocos_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vocos.npz")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _L():
    from amphion_amd import _lib

    return _lib


PW_SHAPES = [(1024, 4096), (4096, 1024), (1024, 1922), (512, 4096), (4096, 512), (384, 1152), (1152, 384), (64, 97), (100, 97)]
PW_T = [1, 7, 255, 256, 1000]
PW_B = [1, 3, 16]


def _pw_case(cin, cout, B, T, epi, seed):
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(cin, cout)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(cout, cin, generator=g) / cin ** 0.5)
        lin.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    x = torch.randn(B, cin, T, generator=g).cuda()
    gamma = (torch.randn(cout, generator=g) * 0.05).cuda()
    res = torch.randn(B, cout, T, generator=g).cuda()
    return lin, x, gamma, res


@pytest.mark.parametrize("epi", [0, 1, 2], ids=["bias", "gelu", "scale_res"])
@pytest.mark.parametrize("cin,cout", PW_SHAPES, ids=[f"{a}x{b}" for a, b in PW_SHAPES])
def test_pointwise_gemm_against_fp64(conv_precision, cin, cout, epi):
    from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle, pw_forward

    _lib = _L()
    worst = 0.0
    for B in PW_B:
        for T in PW_T:
            lin, x, gamma, res = _pw_case(cin, cout, B, T, epi, seed=cin * 7 + cout + B * 131 + T)
            h = _PwHandle()
            y = torch.empty(B, cout, T, device="cuda")
            if epi == 2:
                y.copy_(res)                                  # in place: y aliases res
                pw_forward(h, lin, x, epi, y, gamma=gamma, res=y)
            else:
                pw_forward(h, lin, x, epi, y)
            torch.cuda.synchronize()
            _lib.range_check()
            w64 = lin.weight.detach().double().cuda()
            b64 = lin.bias.detach().double().cuda()
            x64 = x.double()
            lin64 = torch.einsum("oc,bct->bot", w64, x64) + b64[None, :, None]
            cond = torch.einsum("oc,bct->bot", w64.abs(), x64.abs())
            if epi == 0:
                ref, tol = lin64, 2e-6 * cond + 3e-7 * lin64.abs()
            elif epi == 1:
                ref = torch.nn.functional.gelu(lin64)
                tol = 1.2 * 2e-6 * cond + 3e-7 * lin64.abs() + 1e-30
            else:
                g64 = gamma.double()[None, :, None]
                ref = res.double() + g64 * lin64
                tol = g64.abs() * (2e-6 * cond + 3e-7 * lin64.abs()) + 2.5e-7 * ref.abs()
            err = (y.double() - ref).abs()
            ratio = (err / tol.clamp_min(1e-30)).max().item()
            worst = max(worst, ratio)
            assert torch.isfinite(y).all()
            assert ratio <= 1.0, (cin, cout, B, T, epi, ratio)
    print(f"pw {cin}->{cout} epi={epi} [{conv_precision}]: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("cin,cout,epi", [(1024, 4096, 1), (100, 300, 0), (1152, 384, 2)])
def test_pointwise_gemm_strided_input(conv_precision, cin, cout, epi):
    """x as a channel slice of a wider tensor: amp_pw_forward's x_batch_stride (the channels around the slice are huge: reading them
    would show)"""
    from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle, pw_forward

    _lib = _L()
    for B, T in ((1, 250), (3, 97), (16, 64)):
        lin, x, gamma, res = _pw_case(cin, cout, B, T, epi, seed=cin + cout + B + T)
        wide = torch.full((B, cin + 13, T), 3e3, device="cuda")
        wide[:, 5:5 + cin] = x
        xs = wide[:, 5:5 + cin]
        y = res.clone() if epi == 2 else torch.empty(B, cout, T, device="cuda")
        pw_forward(_PwHandle(), lin, xs, epi, y, gamma=gamma if epi == 2 else None, res=y if epi == 2 else None,
                   x_batch_stride=(cin + 13) * T)
        dense = res.clone() if epi == 2 else torch.empty(B, cout, T, device="cuda")
        pw_forward(_PwHandle(), lin, x, epi, dense, gamma=gamma if epi == 2 else None, res=dense if epi == 2 else None)
        torch.cuda.synchronize()
        _lib.range_check()
        assert torch.equal(y, dense), (cin, cout, epi, B, T)


_MANIFEST_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle, pw_forward
lin = torch.nn.Linear(1024, 4096)
x = torch.randn(16, 1024, 256).cuda()
y = torch.empty(16, 4096, 256, device="cuda")
pw_forward(_PwHandle(), lin, x, 1, y)
x1 = torch.randn(1, 1024, 250).cuda()
y1 = torch.empty(1, 4096, 250, device="cuda")
pw_forward(_PwHandle(), lin, x1, 0, y1)
torch.cuda.synchronize()
print("CHILD OK")
"""


def test_manifest_names_the_pointwise_kernel(conv_precision, tmp_path):
    man = tmp_path / "manifest.tsv"
    env = dict(os.environ, AMP_LAUNCH_MANIFEST=str(man), AMP_PRECISION=conv_precision)
    r = subprocess.run([sys.executable, "-c", _MANIFEST_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert "CHILD OK" in r.stdout, r.stdout + r.stderr
    lines = [ln.split("\t") for ln in man.read_text().splitlines() if ln.strip()]
    names = [ln[0] for ln in lines]
    if conv_precision == "f16x3":
        assert names == ["pw_f16x3_kernel<1, 2, 2>", "pw_f16x3_kernel<0, 1, 1>"], names
        gf = float(lines[0][2])
        assert abs(gf - 2 * 4096 * 1024 * 256 * 16 / 1e9) < 1e-3, lines[0]
        assert "pw 1024->4096" in lines[0][4]
    else:
        assert not any(n.startswith("pw_f16x3") for n in names), names
        assert any(n.startswith("conv_mfma_kernel<1,") for n in names), names
        assert "pw_epilogue_kernel<>" in names, names


def test_range_flag_trips_beyond_4094():
    from amphion_amd.models.codec.amphion_codec.vocos import Vocos, _PwHandle, pw_forward

    _lib = _L()
    lin = torch.nn.Linear(64, 97)
    x = torch.randn(2, 64, 40).cuda()
    y = torch.empty(2, 97, 40, device="cuda")
    _lib.set_precision("f16x3")
    pw_forward(_PwHandle(), lin, x, 0, y)
    _lib.range_check()                                     # in range: nothing reported
    x[1, 5, 17] = 5000.0
    pw_forward(_PwHandle(), lin, x, 0, y)
    with pytest.raises(_lib.AmpError) as e:
        _lib.range_check()
    assert e.value.status == _lib.AMP_ERR_RANGE
    _lib.range_check()                                     # the report cleared it
    # through the module: a feature spike that the embed conv carries past the range
    hp = V.small_hp()
    m = Vocos(**hp).cuda()
    m.load_state_dict(V.synth_vocos_state_dict(hp, 3))
    feats = V.synth_features(1, hp["input_channels"], 20, 4).cuda()
    m(feats)
    feats[0, :, 9] = 1e5
    with pytest.raises(_lib.AmpError) as e:
        m(feats)
    assert e.value.status == _lib.AMP_ERR_RANGE


@pytest.mark.parametrize("C", [384, 512, 1024])
def test_dwconv7_layer_norm_against_fp64(conv_precision, C):
    _lib = _L()
    g = torch.Generator().manual_seed(C)
    for B, T in ((1, 7), (3, 250)):
        x = torch.randn(B, C, T, generator=g).cuda()
        w = (torch.randn(C, 1, 7, generator=g) / 7 ** 0.5).cuda()
        b = (torch.randn(C, generator=g) * 0.1).cuda()
        lw = (1 + 0.1 * torch.randn(C, generator=g)).cuda()
        lb = (0.05 * torch.randn(C, generator=g)).cuda()
        y = torch.empty_like(x)
        _lib.check(_lib.lib().amp_dwconv_layer_norm_c(_p(x), _p(w), _p(b), 7, 1, _p(lw), _p(lb), None, B, C, T, 1e-6, 0, _p(y),
                                                      _lib.current_stream_ptr(x.device)))
        d = torch.nn.functional.conv1d(x.double(), w.double(), b.double(), padding=3, groups=C)
        ref = V._ln_c(d, lw.double(), lb.double())
        err = (y.double() - ref).abs().max().item()
        assert err < 2e-5, (C, B, T, err)


def _window_env(n_fft, hop, F):
    w = torch.hann_window(n_fft, dtype=torch.float64)
    e = torch.zeros((F - 1) * hop + n_fft, dtype=torch.float64)
    for f in range(F):
        e[f * hop: f * hop + n_fft] += w ** 2
    return w, e


@pytest.mark.parametrize("n_fft,hop", [(1920, 480), (800, 200), (256, 64)])
def test_istft_same_polar_against_fp64_and_split_path(conv_precision, n_fft, hop):
    _lib = _L()
    bins = n_fft // 2 + 1
    g = torch.Generator().manual_seed(n_fft)
    B, F = 2, 37
    # a wider slab than the head: exercises the batch stride
    slab = torch.randn(B, n_fft + 2 + 5, F, generator=g, dtype=torch.float64)
    slab[:, :bins] = slab[:, :bins] * 1.5 - 1.0
    slab[:, 3] = 6.0                                           # clipped: exp(6) > 100
    slab[0, 5, 3] = 200.0                                      # exp overflows to inf in fp32: clips to 100
    slab[:, bins:n_fft + 2] *= 35.0                            # |phase| up to ~100
    slab[1, bins + 2, :] = 100.0
    head32 = slab.float().cuda()
    w, env = _window_env(n_fft, hop, F)
    wdev, edev = w.float().cuda(), env.float().cuda()
    frames = torch.empty(B, F, n_fft, device="cuda")
    out = torch.empty(B, F * hop, device="cuda")
    d = _lib.amp_mel_desc(n_fft, n_fft, hop, 0, 1, 0.0, 0.0)
    _lib.check(_lib.lib().amp_istft_same_polar(ctypes.byref(d), _p(head32), (n_fft + 7) * F, B, F, 100.0, _p(wdev), _p(edev), _p(frames),
                                               _p(out), _lib.current_stream_ptr(head32.device)))
    torch.cuda.synchronize()
    h64 = head32.double().cpu()[:, : n_fft + 2]
    ref = V.istft_same(V.head_spec(h64, n_fft), n_fft, hop, w)
    err = (out.double().cpu() - ref).abs().max().item()
    peak = ref.abs().max().item()
    assert torch.isfinite(out).all()
    assert err <= 2e-6 * max(peak, 1.0) * 10, (err, peak)
    # the split path: exp / clip / cos / sin in torch (fp32 on the device), then amp_istft_same
    h = head32[:, : n_fft + 2]
    mag = torch.clip(torch.exp(h[:, :bins]), max=100.0)
    re = (mag * torch.cos(h[:, bins:])).contiguous()
    im = (mag * torch.sin(h[:, bins:])).contiguous()
    out2 = torch.empty_like(out)
    _lib.check(_lib.lib().amp_istft_same(ctypes.byref(d), _p(re), _p(im), B, F, _p(wdev), _p(edev), _p(frames), _p(out2),
                                         _lib.current_stream_ptr(re.device)))
    torch.cuda.synchronize()
    diff = (out - out2).abs().max().item()
    assert diff <= 1e-5 * max(peak, 1.0), (diff, peak)
    print(f"istft polar n_fft={n_fft}: max-abs vs fp64 {err:.2e}, vs split path {diff:.2e} (peak {peak:.2f})")


def _load(hp, sd):
    from amphion_amd.models.codec.amphion_codec.vocos import Vocos

    m = Vocos(**hp)
    m.load_state_dict(sd)
    return m.cuda().eval()


def test_golden_reference_outputs(conv_precision):
    z = np.load(GOLDEN)
    for tag in ("a", "b"):
        hp = V.small_hp(int(z[f"{tag}_n_fft"]), int(z[f"{tag}_hop"]))
        sd = V.synth_vocos_state_dict(hp, int(z[f"{tag}_seed"]))
        m = _load(hp, sd)
        x = torch.from_numpy(z[f"{tag}_x"]).cuda()
        with torch.no_grad():
            y = m(x).cpu()
        ref = torch.from_numpy(z[f"{tag}_y"])
        err = (y - ref).abs().max().item()
        print(f"golden {tag} (n_fft {hp['n_fft']}): max-abs {err:.2e}")
        assert y.shape == ref.shape and err <= 1e-4, err


SHAPES = {"recipe": V.recipe_hp, "maskgct": V.maskgct_decoder_hp, "default": V.class_default_hp}


@pytest.mark.parametrize("name", list(SHAPES))
def test_end_to_end_against_fp64(conv_precision, name):
    hp = SHAPES[name]()
    sd = V.synth_vocos_state_dict(hp, 11)
    m = _load(hp, sd)
    for B, F in ((1, 50), (2, 200)):
        x = V.synth_features(B, hp["input_channels"], F, seed=B * 100 + F)
        with torch.no_grad():
            y = m(x.cuda()).cpu().double()
        ref = V.vocos_forward(sd, hp, x)
        t32 = V.vocos_forward(sd, hp, x, dtype=torch.float32).double()
        err = (y - ref).abs().max().item()
        e32 = (t32 - ref).abs().max().item()
        print(f"vocos {name} B={B} F={F} [{conv_precision}]: max-abs {err:.2e} (torch fp32 {e32:.2e}), peak {ref.abs().max().item():.2f}")
        assert y.shape == ref.shape and err <= 1e-4, err


def test_forward_is_deterministic(conv_precision):
    hp = V.class_default_hp()
    m = _load(hp, V.synth_vocos_state_dict(hp, 5))
    x = V.synth_features(3, hp["input_channels"], 120, seed=9).cuda()
    with torch.no_grad():
        a = m(x)
        b = m(x)
    assert torch.equal(a, b)


def test_each_forward_returns_a_fresh_tensor(conv_precision):
    """a result stays what it was after a second forward of the same shape (the work buffers are reused, the output is not)"""
    hp = V.small_hp()
    m = _load(hp, V.synth_vocos_state_dict(hp, 6))
    x1 = V.synth_features(2, hp["input_channels"], 30, seed=1).cuda()
    x2 = V.synth_features(2, hp["input_channels"], 30, seed=2).cuda()
    with torch.no_grad():
        a = m(x1)
        a_copy = a.clone()
        b = m(x2)
    assert a.data_ptr() != b.data_ptr()
    assert torch.equal(a, a_copy)
    assert not torch.equal(a, b)


def test_mismatched_device_or_channels_raise_before_any_launch():
    """a module left on the CPU with a device input, and inputs with the wrong channel count, are refused by the Python layer"""
    from amphion_amd.models.codec.amphion_codec.vocos import ConvNeXtBlock, ISTFTHead, Vocos, VocosBackbone

    hp = V.small_hp()
    sd = V.synth_vocos_state_dict(hp, 7)
    cpu = Vocos(**hp)
    cpu.load_state_dict(sd)
    x = V.synth_features(1, hp["input_channels"], 16, seed=3).cuda()
    with pytest.raises(RuntimeError, match="is on cpu"):
        cpu(x)
    with pytest.raises(RuntimeError, match="is on cpu"):
        cpu.backbone(x)
    feat = torch.randn(1, hp["dim"], 16, device="cuda")
    with pytest.raises(RuntimeError, match="is on cpu"):
        cpu.backbone.convnext[0](feat)
    with pytest.raises(RuntimeError, match="is on cpu"):
        cpu.head(feat.transpose(1, 2))
    # the window alone left behind
    m = _load(hp, sd)
    m.head.istft.window = m.head.istft.window.cpu()
    with pytest.raises(RuntimeError, match="window"):
        m(x)
    m = _load(hp, sd)
    for bad in (x[:, :-1], torch.cat([x, x[:, :1]], 1)):
        with pytest.raises(ValueError, match="input channels"):
            m(bad)
        with pytest.raises(ValueError, match="input channels"):
            m.backbone(bad)
    with pytest.raises(ValueError, match="input channels"):
        m.backbone.convnext[0](feat[:, :-3])
    with pytest.raises(ValueError, match="input channels"):
        m.head(feat[:, :-3].transpose(1, 2))
    assert isinstance(m.backbone, VocosBackbone) and isinstance(m.head, ISTFTHead) and isinstance(m.backbone.convnext[0], ConvNeXtBlock)
    torch.cuda.synchronize()
