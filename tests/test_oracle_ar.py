"""Vevo's autoregressive transformer without a device: the restatement (tests/ar_ref.py) against the golden outputs of the real
``AutoregressiveTransformer`` (tests/golden/make_golden_ar.py), the ``state_dict`` keys, the C ABI surface with every host-side refusal of the
new entries, and the model's ``NotImplementedError`` cases."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ar_ref as A
from ar_ref import FWD_SEED, GEN_SEED, MAX_LENGTH, MIN_NEW, RUNS, SD_SEED

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_ar.npz"))


@pytest.mark.parametrize("dk", [96, 64])
def test_restatement_forward_is_the_reference(dk, gold):
    """the golden is an fp32 evaluation of the function the restatement states: its distance from the fp64 restatement is within 4 x the
    fp32 restatement's own (another order of the same sums), and so is the loss"""
    hp = A.small_hp(dk)
    sd = A.synth_state_dict(hp, SD_SEED)
    inputs = A.synth_forward_inputs(hp, FWD_SEED)
    l32, loss32 = A.forward(sd, hp, *inputs)
    l64, loss64 = A.forward(A.cast(sd, torch.float64), hp, *inputs)
    g = torch.from_numpy(gold[f"fwd_logits_{dk}"]).double()
    e32, eg = float((l32.double() - l64).abs().max()), float((g - l64).abs().max())
    scale = max(1.0, float(l64.abs().max()))
    print(f"forward dk={dk}: restatement fp32 {e32:.3e}, golden {eg:.3e} from fp64 (|logit| max {scale:.2f})")
    assert g.shape == l64.shape and e32 > 0
    assert eg <= 4 * e32 * scale
    el32, elg = abs(float(loss32) - float(loss64)), abs(float(gold[f"fwd_loss_{dk}"]) - float(loss64))
    print(f"loss {float(loss64):.5f}: restatement fp32 {el32:.3e}, golden {elg:.3e}")
    assert elg <= 4 * max(el32, float(np.spacing(np.float32(loss64)))) * max(1.0, abs(float(loss64)))


@pytest.mark.parametrize("name", sorted(RUNS))
def test_restatement_generate_is_the_reference(name, gold):
    """every stored run: decided (each discrete decision at least 4 tau from its boundary) and reproduced token for token"""
    dk, kw, end = RUNS[name]
    hp = A.small_hp(dk)
    sd = A.synth_state_dict(hp, SD_SEED)
    ii, po = A.synth_generate_inputs(hp, GEN_SEED)
    q = gold[f"gen_{name}_q"]
    raw, tau, gap = A.decidedness(sd, A.cast(sd, torch.float64), hp, ii, po, A.Replay(q), max_length=MAX_LENGTH, min_new_tokens=MIN_NEW, **kw)
    print(f"{name}: {len(raw)} tokens, tau {tau:.3e}, smallest gap {gap:.3e} = {gap / tau:.1f} tau")
    assert raw.tolist() == gold[f"gen_{name}_raw"].tolist()
    assert gap >= 4 * tau
    gen, _ = A.generate(sd, hp, ii, po, A.Replay(q), max_length=MAX_LENGTH, min_new_tokens=MIN_NEW, **kw)
    assert gen.tolist() == gold[f"gen_{name}_tokens"].tolist()
    n0 = ii.shape[1] + 2 + po.shape[1] + 1
    eos = A.special(hp)["output_eos"]
    if end == "eos":
        assert int(raw[-1]) == eos and MIN_NEW < len(raw) and n0 + len(raw) < MAX_LENGTH and gen.shape[1] == len(raw) - 1
    if end == "max":
        assert int(raw[-1]) != eos and n0 + len(raw) == MAX_LENGTH and gen.shape[1] == len(raw)


def test_state_dict_keys():
    from amphion_amd.models.vc.autoregressive_transformer import AutoregressiveTransformer

    with open(os.path.join(GOLDEN, "keys_ar.json")) as f:
        keys = json.load(f)
    hp = A.small_hp(96)
    model = AutoregressiveTransformer(**hp)
    assert list(model.state_dict().keys()) == keys == A.state_dict_keys(hp)
    sd = A.synth_state_dict(hp, SD_SEED)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    sp = A.special(hp)
    assert (model.pad_token_id, model.input_bos_token_id, model.input_eos_token_id, model.output_bos_token_id, model.output_eos_token_id) == \
        (sp["pad"], sp["input_bos"], sp["input_eos"], sp["output_bos"], sp["output_eos"])
    assert model.config.vocab_size == sp["vocab"]
    # a checkpoint saved under an older transformers carries the rotary buffers
    old = dict(sd)
    for i in range(hp["num_hidden_layers"]):
        old[f"model.model.layers.{i}.self_attn.rotary_emb.inv_freq"] = torch.zeros(48)
    model.load_state_dict(old)
    assert all(torch.equal(model.state_dict()[k], sd[k]) for k in keys)
    # the padding helpers are the reference's
    ii, im, oi, om = A.synth_forward_inputs(hp, FWD_SEED)
    for mine, ref in zip(model.padding_for_input(ii, im, sp["input_eos"], sp["input_bos"], sp["pad"]), A.padding_for_input(hp, ii, im)):
        assert torch.equal(mine, ref)
    for mine, ref in zip(model.padding_for_output(oi, om, sp["output_eos"], sp["output_bos"], sp["pad"]), A.padding_for_output(hp, oi, om)):
        assert torch.equal(mine, ref)


def test_not_implemented_cases():
    from types import SimpleNamespace

    from amphion_amd.models.vc.autoregressive_transformer import AutoregressiveTransformer

    hp = A.small_hp(64)
    with pytest.raises(NotImplementedError, match="use_global_style_encoder"):
        AutoregressiveTransformer(**hp, use_global_style_encoder=True)
    with pytest.raises(NotImplementedError, match="use_global_style_encoder"):
        AutoregressiveTransformer(cfg=SimpleNamespace(**hp, use_global_style_encoder=True))
    with pytest.raises(NotImplementedError, match="head dimension"):
        AutoregressiveTransformer(hidden_size=2048, num_attention_heads=16, num_hidden_layers=1, intermediate_size=64)
    model = AutoregressiveTransformer(cfg=SimpleNamespace(**hp, use_global_style_encoder=False))
    ii, im, oi, om = A.synth_forward_inputs(hp, FWD_SEED)
    model.train()
    with pytest.raises(NotImplementedError, match="training"):
        model(ii, im, oi, om)
    with pytest.raises(NotImplementedError, match="training"):
        model.generate(ii[:1], prompt_output_ids=oi[:1])
    model.eval()
    with pytest.raises(NotImplementedError, match="one sample"):
        model.generate(ii, prompt_output_ids=oi)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(ii, im, oi, om)


def test_abi_surface_and_host_refusals():
    """the symbols are exported, bound and declared, the version says so, and every refusal is made on the host before anything is launched:
    the pointers below are host buffers that are never read"""
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 155
    names = ("amp_rope_attention_causal", "amp_kv_append", "amp_attention_decode", "amp_attention_decode_workspace_bytes",
             "amp_attention_decode_split", "amp_pw_forward_vec", "amp_pw_forward_vec_workspace_bytes", "amp_ar_sample")
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "amphion_hip.h")) as f:
        header = f.read()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and f" {n}(" in header, n
    INV = _lib.AMP_ERR_INVALID
    buf = (ctypes.c_float * 4096)()
    other = (ctypes.c_float * 4096)()
    third = (ctypes.c_float * 4096)()
    ids = (ctypes.c_longlong * 64)()
    p = lambda a, off=0: ctypes.c_void_p(ctypes.addressof(a) + 4 * off)

    # amp_rope_attention_causal: amp_rope_attention's refusals, in its own name
    def causal(**kw):
        a = dict(q=p(buf), k=p(buf, 256), v=p(buf, 512), bs=0, cos=p(other), sin=p(other, 64), B=1, H=1, dk=64, T=2, scale=0.125, out=p(third))
        a.update(kw)
        return L.amp_rope_attention_causal(a["q"], a["k"], a["v"], a["bs"], a["cos"], a["sin"], None, a["B"], a["H"], a["dk"], a["T"], a["scale"],
                                           a["out"], None)
    for kw in (dict(q=None), dict(out=None), dict(dk=128), dict(T=0), dict(B=0), dict(T=40000), dict(scale=0.0), dict(bs=100), dict(cos=p(other, 1)),
               dict(out=p(buf, 64))):
        assert causal(**kw) == INV, kw
        assert b"amp_rope_attention_causal" in L.amp_last_error(), kw

    def append(**kw):
        a = dict(k=p(buf), v=p(buf, 512), bs=0, cos=p(other), sin=p(other, 64), B=1, H=1, dk=64, T=2, pos0=0, Lmax=8, kc=p(third), vc=p(third, 1024))
        a.update(kw)
        return L.amp_kv_append(a["k"], a["v"], a["bs"], a["cos"], a["sin"], a["B"], a["H"], a["dk"], a["T"], a["pos0"], a["Lmax"], a["kc"], a["vc"], None)
    for kw in (dict(k=None), dict(vc=None), dict(cos=None), dict(dk=32), dict(dk=128), dict(B=0), dict(H=0), dict(T=0), dict(pos0=-1), dict(pos0=7),
               dict(T=9), dict(Lmax=0), dict(bs=64), dict(vc=p(third, 256)), dict(kc=p(buf, 64))):
        assert append(**kw) == INV, kw
        assert b"amp_kv_append" in L.amp_last_error(), kw

    def decode(**kw):
        a = dict(q=p(buf), qbs=0, cos=p(other), sin=p(other, 2048), kc=p(third), vc=p(third, 2048), B=1, H=1, dk=64, L=4, Lmax=8, scale=0.125,
                 out=p(buf, 1024), ws=p(buf, 2048), wsb=4096)
        a.update(kw)
        return L.amp_attention_decode(a["q"], a["qbs"], a["cos"], a["sin"], a["kc"], a["vc"], a["B"], a["H"], a["dk"], a["L"], a["Lmax"], a["scale"],
                                      a["out"], a["ws"], a["wsb"], None)
    S = L.amp_attention_decode_split()
    assert S >= 64 and L.amp_attention_decode_workspace_bytes(1, 16, 96, 2048) == 16 * ((2048 + S - 1) // S) * 98 * 4
    assert L.amp_attention_decode_workspace_bytes(0, 16, 96, 2048) == 0
    for kw in (dict(q=None), dict(out=None), dict(kc=None), dict(sin=None), dict(dk=32), dict(dk=128), dict(B=0), dict(H=0), dict(L=0), dict(L=9),
               dict(Lmax=0), dict(scale=-1.0), dict(scale=float("nan")), dict(qbs=32), dict(out=p(buf, 32)), dict(out=p(third, 8)),
               dict(L=S + 1, Lmax=S + 1, ws=None), dict(L=S + 1, Lmax=S + 1, wsb=8), dict(L=S + 1, Lmax=S + 1, kc=None)):
        assert decode(**kw) == INV, kw
        assert b"amp_attention_decode" in L.amp_last_error(), kw

    # amp_pw_forward_vec: a handle needs a device (amp_pw_create uploads the weights); without one the NULL refusals (the others are
    # exercised on the device, tests/test_gpu_ar.py)
    assert L.amp_pw_forward_vec(None, p(buf), 0, 1, 0, None, None, p(other), p(third), 4096, None) == INV
    assert b"amp_pw_forward_vec" in L.amp_last_error()
    assert L.amp_pw_forward_vec_workspace_bytes(None, 1) == 0

    def sample(**kw):
        a = dict(lg=p(buf), bs=0, B=1, V=150, q=p(other), ids=ctypes.cast(ids, ctypes.c_void_p), cap=64, n=3, eos=5, sup=1, temp=0.8, k=50,
                 top_p=0.9, pen=1.1)
        a.update(kw)
        return L.amp_ar_sample(a["lg"], a["bs"], a["B"], a["V"], a["q"], a["ids"], a["cap"], a["n"], a["eos"], a["sup"], a["temp"], a["k"], a["top_p"],
                               a["pen"], None)
    for kw in (dict(lg=None), dict(q=None), dict(ids=None), dict(V=1), dict(V=16385), dict(B=0), dict(k=0), dict(top_p=0.0), dict(top_p=float("nan")),
               dict(temp=0.0), dict(temp=float("inf")), dict(pen=0.0), dict(pen=float("nan")), dict(n=-1), dict(n=64), dict(cap=0), dict(eos=150),
               dict(eos=-1), dict(bs=100), dict(ids=p(buf, 8))):
        assert sample(**kw) == INV, kw
        assert b"amp_ar_sample" in L.amp_last_error(), kw
