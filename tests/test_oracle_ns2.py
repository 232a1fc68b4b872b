"""NaturalSpeech2 on the CPU: the restatement (tests/ns2_ref.py) against the runs stored from the real reference class
(tests/golden/make_golden_ns2.py), the two traps of the reference that the goldens must tell apart, the host fold of out_proj into FiLM, the
package's classes against the real ``state_dict``, and the new entry points' surface with their host-side refusals."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ns2_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNS = {"euler": (dict(), 4), "midpoint": (dict(solver="midpoint"), 3), "flow": (dict(diffusion_type="flow"), 4)}
CONT = ("x0", "prior_out", "dur_pred_log", "dur_pred", "pitch_pred_log")
DISCRETE = ("dur_pred_round", "mel_len", "pitch_token")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_ns2.npz"))


def run_inputs(gold, name):
    over, n_steps = RUNS[name]
    hp = R.small_hp(**over)
    sd = R.synth_state_dict(hp, int(gold["seed"]))
    t = lambda k: torch.from_numpy(gold[f"{name}/{k}"])
    return hp, sd, t("ref_code").transpose(0, 1), t("phone_id"), t("ref_mask"), t("z"), n_steps


@pytest.fixture(scope="module")
def evaluations(gold):
    """every stored run in fp64 and in fp32, once"""
    out = {}
    for name in RUNS:
        hp, sd, codes, phone, mask, z, n = run_inputs(gold, name)
        x64, p64 = R.inference(R.cast(sd, torch.float64), hp, codes, phone, mask, z.double(), n)
        x32, p32 = R.inference(sd, hp, codes, phone, mask, z, n)
        p64["x0"], p32["x0"] = x64, x32
        out[name] = (p64, p32)
    return out


@pytest.mark.parametrize("name", list(RUNS))
def test_restatement_is_the_reference(name, gold, evaluations):
    """The real class and the fp32 restatement are two fp32 evaluations of the fp64 restatement.  With e_g the golden's own distance from
    fp64: the fp32 restatement is within 4 e_g max(1, |golden|max) of the golden (the project's rule with the golden's error as the scale), the
    golden itself is within the same multiple of the fp32 restatement's distance from fp64 (so e_g IS rounding, not a different formula), and
    every discrete output is equal.  Every decision is at least 4 tau from its boundary."""
    p64, p32 = evaluations[name]
    hp, sd, codes, phone, mask, z, n = run_inputs(gold, name)
    ok, tau, d_gap, p_gap, _, _ = R.decided(sd, hp, codes, phone, mask, None, 0)
    print(f"{name}: tau {tau[0]:.2e} / {tau[1]:.2e}, smallest gaps {d_gap:.1f} (durations) / {p_gap:.1f} (pitch bins) tau")
    assert ok and d_gap >= 4 and p_gap >= 4
    for k in DISCRETE:
        assert torch.equal(p32[k], torch.from_numpy(gold[f"{name}/{k}"])), k
    for k in CONT:
        g = torch.from_numpy(gold[f"{name}/{k}"])
        assert p32[k].shape == g.shape
        scale = max(1.0, float(g.abs().max()))
        e_g = float((g.double() - p64[k]).abs().max())
        e_32 = float((p32[k].double() - p64[k]).abs().max())
        d = float((p32[k] - g).abs().max())
        print(f"{name} {k}: golden vs fp64 {e_g:.2e}, fp32 restatement vs fp64 {e_32:.2e}, fp32 restatement vs golden {d:.2e}")
        assert d <= 4 * e_g * scale, (k, d, e_g)
        assert e_g <= 4 * e_32 * scale, (k, e_g, e_32)
    if name == "euler":                                   # ragged frame counts, durations with zeros and a spread
        d = p32["dur_pred_round"]
        assert len(set(p32["mel_len"].tolist())) == 2 and int((d == 0).sum()) > 0 and int(d.max()) >= 5


@pytest.mark.parametrize("fix", ["fix_pe", "fix_style"])
def test_the_goldens_catch_a_repaired_trap(fix, gold, evaluations):
    """PositionalEncoding adds row b of its table to every frame of item b, and StyleAdaptiveLayerNorm averages the prompt over its padded
    length: a restatement with either one "repaired" misses the ragged-prompt golden by far more than the bound"""
    p64, p32 = evaluations["euler"]
    hp, sd, codes, phone, mask, z, n = run_inputs(gold, "euler")
    _, pf = R.inference(sd, hp, codes, phone, mask, None, 0, **{fix: True})
    g = torch.from_numpy(gold["euler/dur_pred_log"])
    e_g = float((g.double() - p64["dur_pred_log"]).abs().max())
    bound = 4 * e_g * max(1.0, float(g.abs().max()))
    miss = float((pf["dur_pred_log"] - g).abs().max())
    print(f"{fix}: dur_pred_log misses the golden by {miss:.3e}, bound {bound:.3e}")
    assert miss > 1000 * bound


def test_film_fold_against_the_unfolded_product():
    """(Wg Wo) a + (Wg bo + bg) against film(out_proj(a)) in fp64: the fold is an fp32 rounding of the exact map"""
    from amphion_amd.models.tts.naturalspeech2.wavenet import fold_film

    g = torch.Generator().manual_seed(5)
    H, T = 128, 33
    gw, bw, ow = (torch.randn(s, generator=g) / H ** 0.5 for s in ((2 * H, H), (2 * H, H), (H, H)))
    gb, bb, ob = 1.0 + 0.1 * torch.randn(2 * H, generator=g), 0.1 * torch.randn(2 * H, generator=g), 0.1 * torch.randn(H, generator=g)
    a = torch.randn(H, T, generator=g).double()
    y = ow.double() @ a + ob.double()[:, None]
    ref = torch.cat((gw.double() @ y + gb.double()[:, None], bw.double() @ y + bb.double()[:, None]), 0)
    W, b = fold_film(gw, gb, bw, bb, ow, ob)
    assert W.dtype == torch.float32 and tuple(W.shape) == (4 * H, H) and tuple(b.shape) == (4 * H,)
    got = W.double() @ a + b.double()[:, None]
    # one fp32 rounding of each folded weight: at most 2^-24 relative per term of a sum of H + 1 terms
    bound = 2.0 ** -24 * (W.double().abs() @ a.abs() + b.double().abs()[:, None]).max()
    assert float((got - ref).abs().max()) <= float(bound)


def test_state_dict_keys_and_refusals():
    from amphion_amd.models.tts.naturalspeech2 import NaturalSpeech2

    with open(os.path.join(GOLDEN, "keys_ns2.json")) as f:
        keys = json.load(f)
    hp = R.small_hp()
    assert {k: list(v) for k, v in R.param_shapes(hp).items()} == keys
    m = NaturalSpeech2(R.make_cfg(hp))
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == keys
    sd = R.synth_state_dict(hp, 0)
    m.load_state_dict(sd, strict=True)
    assert m.prior_encoder.enc_emb_tokens is m.prior_encoder.encoder.enc_emb_tokens            # one embedding under two keys
    assert torch.equal(m.prompt_encoder.position_emb.pe, R.pe_table(hp["hidden"])) and tuple(m.prompt_encoder.position_emb.pe.shape) == (5000, 1, hp["hidden"])
    assert torch.equal(m.prior_encoder.pitch_bins, R.pitch_bins(hp))
    saved = m.state_dict()
    assert all(torch.equal(saved[k], sd[k]) for k in sd if "quantizer" in k)
    for flow in (False, True):
        assert type(NaturalSpeech2(R.make_cfg(R.small_hp(diffusion_type="flow" if flow else "diffusion"))).diffusion).__name__ == ("DiffusionFlow" if flow else "Diffusion")
    with pytest.raises(NotImplementedError, match="prompt_lin"):
        NaturalSpeech2(R.make_cfg(R.small_hp(latent=hp["hidden"])))
    with pytest.raises(NotImplementedError):
        m()
    with pytest.raises(NotImplementedError):
        m.latent_to_code(torch.zeros(1, hp["latent"], 4))
    with pytest.raises(NotImplementedError):
        m.reverse_diffusion_from_t()
    with pytest.raises(NotImplementedError, match="eval"):
        m.inference(ref_latent=torch.zeros(1, hp["latent"], 4), phone_id=torch.ones(1, 3, dtype=torch.long), ref_mask=torch.ones(1, 4))
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.inference(ref_latent=torch.zeros(1, hp["latent"], 4), phone_id=torch.ones(1, 3, dtype=torch.long), ref_mask=torch.ones(1, 4))


def test_abi_surface_and_host_refusals():
    """the symbols are exported, bound and declared, the version says so, and every refusal is made on the host before anything is launched:
    the pointers below are host buffers that are never read"""
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 157
    names = ("amp_cross_attention", "amp_ns2_layer_create", "amp_ns2_layer_precision", "amp_ns2_layer_workspace_bytes", "amp_ns2_layer_forward",
             "amp_ns2_layer_destroy", "amp_ns2_ode_step")
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "amphion_hip.h")) as f:
        header = f.read()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and f" {n}(" in header, n
    INV, UNS = _lib.AMP_ERR_INVALID, _lib.AMP_ERR_UNSUPPORTED
    buf, other = (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)()
    msg = lambda: L.amp_last_error().decode()
    # amp_cross_attention: dk, sizes, strides, scale, overlap, NULL
    for dk in (32, 96, 128):
        assert L.amp_cross_attention(buf, 0, buf, buf, 0, None, 1, 2, dk, 4, 4, 0.1, other, None) == INV and "64" in msg()
    assert L.amp_cross_attention(buf, 0, buf, buf, 0, None, 1, 2, 64, 0, 4, 0.1, other, None) == INV
    assert L.amp_cross_attention(buf, 0, buf, buf, 0, None, 1, 2, 64, 4, 0, 0.1, other, None) == INV
    assert L.amp_cross_attention(buf, 0, buf, buf, 0, None, 1, 2, 64, 40000, 4, 0.1, other, None) == INV
    assert L.amp_cross_attention(buf, 100, buf, buf, 0, None, 2, 2, 64, 4, 4, 0.1, other, None) == INV and "q batch stride" in msg()
    assert L.amp_cross_attention(buf, 0, buf, buf, 100, None, 2, 2, 64, 4, 4, 0.1, other, None) == INV
    assert L.amp_cross_attention(buf, 0, buf, buf, 0, None, 1, 2, 64, 4, 4, 0.0, other, None) == INV
    assert L.amp_cross_attention(buf, 0, buf, buf, 0, None, 1, 2, 64, 4, 4, 0.1, buf, None) == INV and "overlap" in msg()
    assert L.amp_cross_attention(None, 0, buf, buf, 0, None, 1, 2, 64, 4, 4, 0.1, other, None) == INV
    # amp_ns2_layer_create: the geometry is judged before a device is asked for
    h = ctypes.c_void_p()
    for hidden, dil in ((96, 1), (64, 1), (576, 1), (160, 1), (128, 0), (128, 9)):
        assert L.amp_ns2_layer_create(hidden, dil, buf, buf, buf, buf, ctypes.byref(h)) == UNS, (hidden, dil)
        assert h.value is None
    assert L.amp_ns2_layer_create(128, 1, None, buf, buf, buf, ctypes.byref(h)) == INV
    assert L.amp_ns2_layer_forward(None, buf, buf, 0, buf, 0, None, None, 1, 4, other, other, other, 0, None) == INV
    assert L.amp_ns2_layer_workspace_bytes(None, 1, 4) == 0 and L.amp_ns2_layer_precision(None) == -1
    # amp_ns2_ode_step
    assert L.amp_ns2_ode_step(buf, buf, buf, 0, 1.0, 1.0, 1.0, 1.0, 0, other, None) == INV
    assert L.amp_ns2_ode_step(None, buf, buf, 4, 1.0, 1.0, 1.0, 1.0, 0, other, None) == INV
    assert L.amp_ns2_ode_step(buf, buf, buf, 4, float("nan"), 1.0, 1.0, 1.0, 0, other, None) == INV and "NaN" in msg()
    shifted = ctypes.cast(ctypes.addressof(buf) + 8, ctypes.POINTER(ctypes.c_float))
    assert L.amp_ns2_ode_step(buf, buf, buf, 16, 1.0, 1.0, 1.0, 1.0, 0, shifted, None) == INV and "overlap" in msg()
