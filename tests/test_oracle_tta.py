"""AudioLDM text-to-audio without a GPU: the restatement (tests/tta_ref.py) against goldens written from the REAL classes of the reference
(tests/golden/make_golden_tta.py), the state_dict keys of the drop-in modules, what they refuse, and the C ABI's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import tta_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "golden_tta.npz")


@pytest.fixture(scope="module")
def G():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}


def _keys(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def _models():
    from amphion_amd.models.tta.autoencoder import AutoencoderKL
    from amphion_amd.models.tta.ldm import AudioLDM

    return AudioLDM(R.Cfg(R.small_hp())), AutoencoderKL(R.Cfg(R.small_vae_hp()))


def _check(name, got32, got64, gold):
    """the fp32 restatement is the golden up to the fp32-vs-fp64 distance it measures itself (4 x, scaled by max(1, |ref|max))"""
    e32 = float((got32.double() - got64).abs().max())
    eg = float((gold.double() - got64).abs().max())
    bound = 4.0 * max(e32, 1e-7) * max(1.0, float(got64.abs().max()))
    print(f"{name}: golden-fp64 {eg:.3e} fp32-fp64 {e32:.3e} bound {bound:.3e} |ref|max {float(got64.abs().max()):.3f}")
    assert gold.shape == got64.shape and eg <= bound and float(got64.abs().max()) > 1e-2


def test_keys_are_the_reference_s():
    unet, vae = _models()
    assert list(unet.state_dict().keys()) == _keys("keys_tta.json") and len(_keys("keys_tta.json")) == 626
    assert list(vae.state_dict().keys()) == _keys("keys_autoencoderkl.json") and len(_keys("keys_autoencoderkl.json")) == 272


def test_restatement_reproduces_the_unet_goldens(G):
    unet, _ = _models()
    hp = R.small_hp()
    sd = R.synth_state_dict({k: v.shape for k, v in unet.state_dict().items()}, int(G["seed"]))
    sd64 = R.cast(sd, torch.float64)
    for n in "ab":
        x, t, ctx = G[f"unet_{n}_x"], G[f"unet_{n}_t"], G[f"unet_{n}_ctx"]
        _check(f"unet {n}", R.unet_forward(sd, hp, x, t, ctx), R.unet_forward(sd64, hp, x.double(), t, ctx.double()), G[f"unet_{n}_y"])
    steps, gd = int(G["steps"]), float(G["guidance"])
    for n in "ab":
        lat, ctx = G[f"unet_{n}_lat"], G[f"unet_{n}_ctx"]
        _check(f"loop {n}", R.generate_latents_ref(sd, hp, ctx, steps, gd, lat), R.generate_latents_ref(sd64, hp, ctx.double(), steps, gd, lat.double()),
               G[f"unet_{n}_lat_out"])


def test_restatement_reproduces_the_decoder_goldens(G):
    _, vae = _models()
    hp = R.small_vae_hp()
    sd = R.synth_state_dict({k: v.shape for k, v in vae.state_dict().items()}, int(G["vae_seed"]))
    sd64 = R.cast(sd, torch.float64)
    for n in "abc":
        z = G[f"vae_{n}_z"]
        _check(f"decode {n}", R.decode_ref(sd, hp, z), R.decode_ref(sd64, hp, z.double()), G[f"vae_{n}_mel"])


def test_zero_modules_are_zero_after_init_and_state_dict_round_trips():
    unet, vae = _models()
    sd0 = unet.state_dict()
    for k in ("unet.out.2.weight", "unet.input_blocks.1.0.out_layers.3.weight", "unet.input_blocks.1.1.proj_out.weight", "unet.middle_block.1.proj_out.bias"):
        assert float(sd0[k].abs().max()) == 0.0, k
    for m, seed in ((unet, 5), (vae, 6)):
        sd = R.synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed)
        assert not m.load_state_dict(sd).missing_keys
        back = m.state_dict()
        assert all(torch.equal(back[k], sd[k]) for k in sd)
    # the encoder's parameters are held, never run
    assert "encoder.down.0.downsample.conv.weight" in vae.state_dict() and "quant_conv.weight" in vae.state_dict()
    with pytest.raises(NotImplementedError):
        vae.encode(torch.zeros(1, 1, 16, 16))
    with pytest.raises(NotImplementedError):
        vae(torch.zeros(1, 1, 16, 16))


@pytest.mark.parametrize("arg,value", [("use_spatial_transformer", False), ("legacy", True), ("num_head_channels", 32), ("use_scale_shift_norm", True),
                                       ("resblock_updown", True), ("dims", 1), ("num_classes", 10), ("conv_resample", False), ("use_fp16", True),
                                       ("n_embed", 8)])
def test_unsupported_constructor_arguments_are_refused_by_name(arg, value):
    from amphion_amd.models.tta.ldm import UNetModel

    hp = dict(R.small_hp())
    hp.update({arg: value})
    with pytest.raises(NotImplementedError, match=arg):
        UNetModel(**hp)


def test_modules_refuse_what_is_not_built():
    from amphion_amd.models.tta.ldm import ResBlock, timestep_embedding
    from amphion_amd.models.tta.ldm.attention import CrossAttention, FeedForward

    for kw in (dict(use_conv=True), dict(use_scale_shift_norm=True), dict(up=True), dict(down=True), dict(dims=3)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            ResBlock(64, 256, 0.0, out_channels=128, **kw)
    with pytest.raises(NotImplementedError):
        CrossAttention(96, heads=2, dim_head=48)
    with pytest.raises(NotImplementedError):
        FeedForward(64, glu=False)
    t = torch.tensor([0, 500])
    e = timestep_embedding(t, 64)
    assert tuple(e.shape) == (2, 64) and torch.equal(e[0], torch.cat([torch.ones(32), torch.zeros(32)]))      # cos | sin
    assert torch.equal(e, R.timestep_embedding(t, 64, torch.float32))
    with pytest.raises(RuntimeError):                              # no CPU fallback
        ResBlock(64, 256, 0.0).eval()(torch.zeros(1, 64, 2, 2), torch.zeros(1, 256))


def test_scheduler_and_loop_are_duck_typed():
    """``generate_latents`` is the reference's loop: with a model that returns a known function the update is the scheduler's, step by step"""
    from amphion_amd.models.tta.ldm import generate_latents

    class Toy(torch.nn.Module):
        def forward(self, x, t, c):
            assert x.shape[0] == 2 and t.shape == (2,) and int(t[0]) == int(t[1])
            return torch.cat([0.1 * x[:1], 0.3 * x[1:]])

    lat = torch.randn(1, 4, 2, 3, generator=torch.Generator().manual_seed(1))
    got = generate_latents(Toy(), torch.zeros(2, 1, 4), R.TestScheduler(), 3, 3.0, lat)
    sch = R.TestScheduler()
    sch.set_timesteps(3)
    want = lat
    for t in sch.timesteps:
        want = sch.step(0.1 * want + 3.0 * (0.3 * want - 0.1 * want), t, want).prev_sample
    assert torch.equal(got, want)


def test_abi_version_symbols_and_argument_checks():
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 159
    names = ("amp_conv2d_create", "amp_conv2d_precision", "amp_conv2d_workspace_bytes", "amp_conv2d_plan", "amp_conv2d_forward", "amp_conv2d_destroy", "amp_group_norm_stats",
             "amp_group_norm", "amp_geglu", "amp_cross_attention_hd")
    with open(os.path.join(HERE, "..", "include", "amphion_hip.h")) as f:
        header = f.read()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and f" {n}(" in header and hasattr(L, n), n
    INV, UNS = _lib.AMP_ERR_INVALID, _lib.AMP_ERR_UNSUPPORTED
    buf, other = (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)()
    msg = lambda: L.amp_last_error().decode()
    h = ctypes.c_void_p()
    for cin, cout in ((3, 64), (48, 64), (2080, 64), (64, 2), (64, 48), (64, 1056)):
        assert L.amp_conv2d_create(cin, cout, buf, None, ctypes.byref(h)) == UNS and "not covered" in msg() and not h.value
    assert L.amp_conv2d_create(64, 64, None, None, ctypes.byref(h)) == INV
    assert L.amp_conv2d_forward(None, buf, 1, 2, 2, 1, 0, None, None, None, None, 0, None, other, None, 0, None) == INV
    assert L.amp_conv2d_plan(None, 2, 2, 1, 0, None, None, None) == INV
    assert L.amp_conv2d_workspace_bytes(None, 1, 2, 2, 1, 0) == 0 and L.amp_conv2d_precision(None) == -1
    assert L.amp_group_norm_stats(buf, 1, 48, 4, 1e-5, other, None) == UNS and "32" in msg()
    assert L.amp_group_norm_stats(buf, 1, 32, 0, 1e-5, other, None) == INV
    assert L.amp_group_norm_stats(buf, 1, 32, 4, -1.0, other, None) == INV
    assert L.amp_group_norm_stats(None, 1, 32, 4, 1e-5, other, None) == INV
    assert L.amp_group_norm_stats(buf, 1, 32, 4, 1e-5, buf, None) == INV and "overlap" in msg()
    assert L.amp_group_norm(buf, other, other, other, 1, 48, 4, 0, other, None) == UNS
    assert L.amp_group_norm(buf, None, other, other, 1, 32, 4, 0, other, None) == INV
    assert L.amp_geglu(buf, 1, 0, 4, other, None) == INV
    assert L.amp_geglu(buf, 1, 8, 4, buf, None) == INV and "overlap" in msg()
    assert L.amp_geglu(None, 1, 8, 4, other, None) == INV
    for dk in (16, 48, 96, 256):
        assert L.amp_cross_attention_hd(buf, 0, buf, buf, 0, None, 1, 2, dk, 4, 4, 0.1, other, None) == INV and "32, 64 or 128" in msg()
    assert L.amp_cross_attention_hd(buf, 0, buf, buf, 0, None, 1, 2, 32, 0, 4, 0.1, other, None) == INV
    assert L.amp_cross_attention_hd(buf, 0, buf, buf, 0, None, 1, 2, 128, 4, 4, 0.1, buf, None) == INV and "overlap" in msg()
    for dk in (32, 128):                                           # the NaturalSpeech2 entry keeps its one head dimension
        assert L.amp_cross_attention(buf, 0, buf, buf, 0, None, 1, 2, dk, 4, 4, 0.1, other, None) == INV and "64" in msg()
