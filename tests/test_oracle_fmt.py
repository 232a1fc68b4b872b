"""CPU checks of Vevo's flow-matching transformer: the fp32 restatement of tests/fmt_ref.py against the golden outputs of the real reference
classes (tests/golden/make_golden_fmt.py), the state_dict key lists, that the goldens can tell the likely mistakes apart, and the new ABI.

Bound of the restatement against the golden: two fp32 evaluations of one formula in different operation orders (HF's attention, fused
Linears), 2e-5 relative to max(1, |golden|max) as in tests/test_oracle_facodec_vc.py; measured here: 0 in fp32 (the same torch operations in the same order), 1.2e-6 in fp64."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fmt_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
REL = 2e-5


def dist(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_fmt.npz"))


@pytest.fixture(scope="module")
def sd(gold):
    return R.synth_state_dict(R.small_hp(), int(gold["seed"]))


def _forward(gold, sd, T, dtype=torch.float32, **kw):
    x, t, codes = (torch.from_numpy(gold[f"fwd_{k}_{T}"]) for k in ("x", "t", "codes"))
    mask = torch.ones(2, T)
    mask[1, int(gold["valid"]):] = 0
    hid = []
    y = R.diffllama_forward(R.cast(sd, dtype), R.small_hp(), x.to(dtype), t.to(dtype), sd["cond_emb.weight"][codes].to(dtype), mask.to(dtype),
                            hidden=hid, **kw)
    return y, hid


def _reverse(gold, sd, cfg, dtype=torch.float32, **kw):
    prompt, codes, noise = (torch.from_numpy(gold[k]) for k in ("rd_prompt", "rd_codes", "rd_noise"))
    cond = sd["cond_emb.weight"][codes]
    return R.reverse_diffusion(R.cast(sd, dtype), R.small_hp(), cond.to(dtype), prompt.to(dtype), noise.to(dtype), n_timesteps=4, cfg=cfg, **kw)


@pytest.mark.parametrize("T", [37, 150])
def test_forward_restatement_reproduces_the_golden(gold, sd, T):
    for dtype in (torch.float32, torch.float64):
        y, hid = _forward(gold, sd, T, dtype)
        assert dist(y, gold[f"fwd_y_{T}"]) <= REL and dist(hid[0], gold[f"fwd_h0_{T}"]) <= REL


@pytest.mark.parametrize("cfg", [0.0, 2.0])
def test_reverse_diffusion_restatement_reproduces_the_golden(gold, sd, cfg):
    for dtype in (torch.float32, torch.float64):
        assert dist(_reverse(gold, sd, cfg, dtype), gold[f"rd_y_{cfg}"]) <= REL


def test_golden_noise_is_the_seeded_draw(gold):
    torch.manual_seed(int(gold["rd_seed"]))
    assert torch.equal(torch.randn(2, 26, 20), torch.from_numpy(gold["rd_noise"]))


def test_sensitivity_of_the_goldens(gold, sd):
    """Each likely mistake misses the goldens by a large multiple of the bound: interleaved-pair RoPE instead of rotate-half, the mask applied to
    queries instead of keys, and the classifier-free std taken per item instead of over the whole tensor.

    A BIASED std over the whole tensor is not among them, and cannot be: the std enters reverse_diffusion only as the ratio
    ``flow_pred.std() / flow_pred_cfg.std()`` of two tensors of one size n, and the factor sqrt((n - 1) / n) cancels.  The biased variant
    reproduces the golden to rounding, which is asserted here so that nobody takes the cancellation for coverage."""
    for kw in (dict(rope="interleaved"), dict(mask_on="queries")):
        for T in (37, 150):
            assert dist(_forward(gold, sd, T, **kw)[0], gold[f"fwd_y_{T}"]) > 100 * REL, kw
    assert dist(_reverse(gold, sd, 2.0, rope="interleaved"), gold["rd_y_2.0"]) > 100 * REL        # (the sampler's goldens carry no mask)
    assert dist(_reverse(gold, sd, 2.0, unbiased=False), gold["rd_y_2.0"]) <= REL
    per_item = _reverse(gold, sd, 2.0, std=lambda v: v.std(dim=(1, 2), keepdim=True))
    assert dist(per_item, gold["rd_y_2.0"]) > 100 * REL


def test_rope_is_hf_rotate_half():
    """against the expression of modeling_llama.py (rotate_half / apply_rotary_pos_emb) written out, and unlike the interleaved form"""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 2, 5, 64, generator=g, dtype=torch.float64)
    cos, sin = R.rope_cos_sin(5, 64, dtype=torch.float64)
    got = R.apply_rope(x, cos, sin)
    for i in range(32):
        assert torch.allclose(got[..., i], x[..., i] * cos[:, i] - x[..., i + 32] * sin[:, i], rtol=0, atol=1e-15)
        assert torch.allclose(got[..., i + 32], x[..., i + 32] * cos[:, i] + x[..., i] * sin[:, i], rtol=0, atol=1e-15)
    assert float((R.apply_rope(x, cos, sin, "interleaved") - got).abs().max()) > 0.1
    assert torch.equal(got[:, :, 0], x[:, :, 0])          # position 0 is not rotated


def test_state_dict_keys_and_loading():
    from amphion_amd.models.vc.flow_matching_transformer import DiffLlama, FlowMatchingTransformer, LlamaAdaptiveRMSNorm, SinusoidalPosEmb  # noqa: F401

    hp = R.small_hp()
    with open(os.path.join(GOLDEN, "keys_fmt.json")) as f:
        keys = json.load(f)
    m = FlowMatchingTransformer(**hp)
    assert list(m.state_dict()) == keys == R.state_dict_keys(hp)
    assert list(DiffLlama(mel_dim=20, hidden_size=128, num_heads=2, num_layers=2).state_dict()) == [k.split(".", 1)[1] for k in keys[1:]]
    sd = R.synth_state_dict(hp, 3)
    old = dict(sd)                      # a checkpoint saved under an older transformers carries the rotary buffers
    old["diff_estimator.layers.0.self_attn.rotary_emb.inv_freq"] = torch.zeros(32)
    old["diff_estimator.layers.1.self_attn.rotary_emb.inv_freq"] = torch.zeros(32)
    m.load_state_dict(old)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    with pytest.raises(RuntimeError):
        m.load_state_dict({**sd, "diff_estimator.layers.0.bogus": torch.zeros(1)})


def test_package_does_not_import_transformers():
    import subprocess

    code = "import sys; import amphion_amd.models.vc.flow_matching_transformer; sys.exit(1 if 'transformers' in sys.modules else 0)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


def test_cfg_overrides_and_eval_only_scope():
    from types import SimpleNamespace

    from amphion_amd.models.vc.flow_matching_transformer import DiffLlama, FlowMatchingTransformer

    m = FlowMatchingTransformer(cfg=SimpleNamespace(mel_dim=24, hidden_size=128, num_layers=1, num_heads=2, use_cond_code=False, cond_dim=48))
    assert (m.mel_dim, m.hidden_size, m.num_layers, m.num_heads) == (24, 128, 1, 2)
    assert isinstance(m.cond_emb, torch.nn.Linear) and m.cond_emb.in_features == 48
    assert m.diff_estimator.mel_mlp[0].in_features == 24 and len(m.diff_estimator.layers) == 1
    x = torch.zeros(1, 4, 24)
    for f in (lambda: m(x, None), lambda: m.compute_loss(x, None), lambda: m.loss_t(x, None, None), lambda: m.forward_diffusion(x, None)):
        with pytest.raises(NotImplementedError, match="eval-only"):
            f()
    with pytest.raises(NotImplementedError, match="64"):
        DiffLlama(hidden_size=1024, num_heads=8)
    n = m.diff_estimator.norm                 # the reference's initialisation: the adaptive norms start as plain RMS norms
    assert float(n.to_weight.weight.detach().abs().max()) == 0.0 and bool((n.to_weight.bias == 1).all())


def test_abi():
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 153
    for name in ("amp_rope_attention", "amp_rms_norm_c_adaptive", "amp_silu", "amp_swiglu"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(L, name) is not None
    # judged on the host, before a device is asked for
    assert L.amp_rope_attention(None, None, None, 0, None, None, None, 1, 1, 64, 1, 0.125, None, None) == _lib.AMP_ERR_INVALID
    assert L.amp_silu(None, 0, None, None) == _lib.AMP_ERR_INVALID
