"""VALL-E without a device: the restatement (tests/valle_ref.py), both of its AR paths, against the golden outputs of the real ``VALLE``
(tests/golden/make_golden_valle.py), the cached path against the recomputing one, the host fold of the adaptive norms against the unfolded
form, the ``state_dict`` keys, the C ABI surface with the host-side refusals of the new entries, and the model's ``NotImplementedError``
cases."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import valle_ref as V
from valle_ref import CONTINUAL_FRAMES, CONTINUAL_HP, CONTINUAL_TEXT, IN_SEED, RUNS, SD_SEED

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_valle.npz"))


def _run(name):
    over, text_len, kw, end = RUNS[name]
    hp = V.make_hp(**over)
    sd = V.synth_state_dict(hp, SD_SEED)
    return hp, sd, V.synth_inputs(hp, IN_SEED, text_len), kw, end


@pytest.mark.parametrize("name", sorted(RUNS))
def test_restatement_inference_is_the_reference(name, gold):
    """every stored run: decided (each discrete decision at least 4 tau from its boundary), reproduced token for token by the cached and by
    the recomputing path in fp32, and ended as the real class ended it"""
    hp, sd, (x, x_lens, y, enroll), kw, end = _run(name)
    q, want = gold[f"inf_{name}_q"], gold[f"inf_{name}_codes"]
    codes, ended, tau, gap = V.decidedness(sd, V.cast(sd, torch.float64), hp, x, x_lens, y, enroll, V.Replay(q), path="cache", **kw)
    print(f"{name}: {codes.shape[1]} tokens, ends on {ended}, tau {tau:.3e}, smallest gap {gap:.3e} = {gap / tau:.1f} tau")
    assert codes.tolist() == want.tolist()
    assert gap >= 4 * tau
    again, ended2 = V.inference(sd, hp, x, x_lens, y, enroll, V.Replay(q), path="recompute", **kw)
    assert again.tolist() == want.tolist() and ended2 == ended == end == str(gold[f"inf_{name}_end"])
    n, bos = want.shape[1], int(hp["prepend_bos"])
    assert want.shape == (1, n, hp["num_quantizers"]) and q.shape == (n + 1, hp["audio_token_num"] + 1)
    if end == "cap":
        assert n + bos == 16 * x.shape[1] + 1
    else:
        assert 10 <= n <= 40 and n + bos <= 16 * x.shape[1]


def test_restatement_continual_is_the_reference(gold):
    hp = V.make_hp(**CONTINUAL_HP)
    sd = V.synth_state_dict(hp, int(gold["continual_sd_seed"]))
    x, x_lens, y, _ = V.synth_inputs(hp, IN_SEED, CONTINUAL_TEXT, CONTINUAL_FRAMES)
    codes, tau, gap = V.continual_decidedness(sd, V.cast(sd, torch.float64), hp, x, x_lens, y)
    print(f"continual: tau {tau:.3e}, smallest gap {gap:.3e} = {gap / tau:.1f} tau")
    assert codes.tolist() == gold["continual_codes"].tolist() and gap >= 4 * tau
    assert codes.shape == (1, CONTINUAL_FRAMES - CONTINUAL_FRAMES // 2, 8) and torch.equal(codes[..., 0], y[:, CONTINUAL_FRAMES // 2:, 0])


@pytest.mark.parametrize("name", ["eos", "bos"])
def test_cached_decoding_is_the_recomputation(name, gold):
    """the step logits of the cached path equal the recomputing path's within the fp32-vs-fp64 bound: with e32 the distance of the fp32
    recomputation from the fp64 one (teacher-forced on the stored tokens), the cached fp32 logits are within 4 e32 max(1, |l64|max) of fp64,
    and the two fp64 paths agree to fp64 rounding"""
    hp, sd, (x, x_lens, y, enroll), kw, _ = _run(name)
    q, teacher = gold[f"inf_{name}_q"], torch.from_numpy(gold[f"inf_{name}_codes"])
    sd64 = V.cast(sd, torch.float64)
    rec = {}
    for tag, w, path in (("r32", sd, "recompute"), ("c32", sd, "cache"), ("r64", sd64, "recompute"), ("c64", sd64, "cache")):
        r = []
        V.inference(w, hp, x, x_lens, y, enroll, V.Replay(q), path=path, teacher=teacher, record=r, **kw)
        rec[tag] = torch.stack([e["logits"].double() for e in r if "logits" in e])
    assert rec["r64"].shape == (teacher.shape[1] + 1, hp["audio_token_num"] + 1)
    scale = max(1.0, float(rec["r64"].abs().max()))
    e32 = float((rec["r32"] - rec["r64"]).abs().max())
    ec = float((rec["c32"] - rec["r64"]).abs().max())
    e64 = float((rec["c64"] - rec["r64"]).abs().max())
    print(f"{name}: recompute fp32 {e32:.3e}, cached fp32 {ec:.3e}, cached fp64 {e64:.3e} from the fp64 recomputation (|logit| max {scale:.2f})")
    assert e32 > 0 and ec <= 4 * e32 * scale
    assert e64 <= 1e-9 * scale


def test_host_fold_of_the_adaptive_norms(gold):
    """one gamma | beta pair per stage and norm, folded in fp64 (amphion_amd/modules/norms/norm.py and valle_ref.fold_affine state the same
    fold), against ``weight * LN(x) + bias``: the NAR logits of every level are within the fp32-vs-fp64 bound of the unfolded fp64 form, and
    the codes are the golden's"""
    from amphion_amd.modules.norms.norm import fold_adaptive

    hp = V.make_hp(**CONTINUAL_HP)
    sd = V.synth_state_dict(hp, int(gold["continual_sd_seed"]))
    x, x_lens, y, _ = V.synth_inputs(hp, IN_SEED, CONTINUAL_TEXT, CONTINUAL_FRAMES)
    teacher = torch.from_numpy(gold["continual_codes"])
    r32, rf, r64 = [], [], []
    V.continual(sd, hp, x, x_lens, y, teacher=teacher, record=r32)
    codes = V.continual(sd, hp, x, x_lens, y, teacher=teacher, record=rf, folded=True)
    V.continual(V.cast(sd, torch.float64), hp, x, x_lens, y, teacher=teacher, record=r64)
    assert codes.tolist() == teacher.tolist()
    for a, f, b in zip(r32, rf, r64):
        scale = max(1.0, float(b["nar_logits"].abs().max()))
        e32 = float((a["nar_logits"].double() - b["nar_logits"]).abs().max())
        ef = float((f["nar_logits"].double() - b["nar_logits"]).abs().max())
        assert e32 > 0 and ef <= 4 * e32 * scale, (e32, ef)
    # the port's fold is the restatement's, bit for bit
    p = "nar_decoder.layers.1.norm2"
    stage = sd["nar_stage_embeddings.3.word_embeddings.weight"]
    g, b = fold_adaptive(sd[p + ".project_layer.weight"], sd[p + ".project_layer.bias"], sd[p + ".norm.weight"], sd[p + ".norm.bias"], stage)
    g2, b2 = V.fold_affine(sd, p, stage)
    assert torch.equal(g, g2) and torch.equal(b, b2)


def test_state_dict_keys():
    from amphion_amd.models.tts.valle import VALLE

    with open(os.path.join(GOLDEN, "keys_valle.json")) as f:
        keys = json.load(f)
    hp = V.make_hp()
    model = VALLE(SimpleNamespace(**hp))
    assert not model.training
    assert len(keys) == 80 and list(model.state_dict().keys()) == keys == V.state_dict_keys(hp)
    sd = V.synth_state_dict(hp, SD_SEED)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    model.load_state_dict(sd)
    assert all(torch.equal(model.state_dict()[k], sd[k]) for k in keys)
    for j in range(hp["num_quantizers"] - 2):                       # the tied pairs stay tied
        assert model.nar_predict_layers[j].weight is model.nar_audio_embeddings[j + 2].weight
    for over in (dict(prepend_bos=True), dict(prefix_mode=1), CONTINUAL_HP, dict(num_quantizers=1), dict(share_embedding=False)):
        hp = V.make_hp(**over)
        assert list(VALLE(SimpleNamespace(**hp)).state_dict().keys()) == V.state_dict_keys(hp)
    # the position table is the reference's formula
    from amphion_amd.modules.transformer.position_embedding import sine_table
    assert torch.equal(sine_table(50, 128), V.sine_pe(50, 128, torch.float32, "cpu"))


def test_not_implemented_cases():
    from amphion_amd.models.tts.valle import VALLE

    for over, match in ((dict(add_prenet=True), "add_prenet"), (dict(norm_first=False), "norm_first"), (dict(decoder_dim=96), "head dimension"),
                        (dict(nhead=4), "head dimension"), (dict(nar_scale_factor=0.75), "head dimension")):
        with pytest.raises(NotImplementedError, match=match):
            VALLE(SimpleNamespace(**V.make_hp(**over)))
    hp = V.make_hp()
    model = VALLE(SimpleNamespace(**hp))
    x, x_lens, y, enroll = V.synth_inputs(hp, IN_SEED, 6)
    with pytest.raises(NotImplementedError, match="training"):
        model(x, x_lens, y, x_lens)
    model.train()
    with pytest.raises(NotImplementedError, match="training"):
        model.inference(x, x_lens, y, enroll)
    model.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.inference(x, x_lens, y, enroll)
    with pytest.raises(AssertionError):
        model.inference(x, x_lens, y.repeat(2, 1, 1), enroll)
    with pytest.raises(AssertionError):                              # the reference's num_quantizers == 8
        model.continual(x, x_lens, y)


def test_abi_surface_and_host_refusals():
    """the symbols are exported, bound and declared, the version says so, and every refusal is made on the host before anything is launched:
    the pointers below are host buffers that are never read"""
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 158
    names = ("amp_prefix_attention", "amp_pw_forward_vec_ln", "amp_pw_forward_vec_ln_workspace_bytes", "amp_embed_pos")
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "amphion_hip.h")) as f:
        header = f.read()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and f" {n}(" in header and hasattr(L, n), n
    INV = _lib.AMP_ERR_INVALID
    buf = (ctypes.c_float * 4096)()
    other = (ctypes.c_float * 4096)()
    third = (ctypes.c_float * 4096)()
    ids = (ctypes.c_longlong * 64)()
    flag = (ctypes.c_uint * 1)()
    p = lambda a, off=0: ctypes.c_void_p(ctypes.addressof(a) + 4 * off)

    # amp_prefix_attention: amp_rope_attention_causal's refusals minus the tables, and the prefix's range
    def prefix(**kw):
        a = dict(q=p(buf), k=p(buf, 256), v=p(buf, 512), bs=0, B=1, H=1, dk=64, T=2, prefix=1, scale=0.125, out=p(third))
        a.update(kw)
        return L.amp_prefix_attention(a["q"], a["k"], a["v"], a["bs"], None, a["B"], a["H"], a["dk"], a["T"], a["prefix"], a["scale"], a["out"], None)
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(dk=128), dict(dk=96), dict(T=0), dict(B=0), dict(H=0), dict(T=40000),
               dict(scale=0.0), dict(scale=float("nan")), dict(bs=100), dict(out=p(buf, 64)), dict(prefix=-1), dict(prefix=3), dict(B=70000)):
        assert prefix(**kw) == INV, kw
        assert b"amp_prefix_attention" in L.amp_last_error(), kw

    # amp_pw_forward_vec_ln: a handle needs a device (amp_pw_create uploads the weights); without one the NULL refusals (the others are
    # exercised on the device, tests/test_gpu_valle.py)
    assert L.amp_pw_forward_vec_ln(None, p(buf), 0, 1, None, None, 1e-5, 0, None, None, p(other), p(third), 4096, None) == INV
    assert b"amp_pw_forward_vec_ln" in L.amp_last_error()
    assert L.amp_pw_forward_vec_ln_workspace_bytes(None, 1) == 0

    def embed(**kw):
        a = dict(tok=ctypes.cast(ids, ctypes.c_void_p), w=p(buf), rows=8, D=16, pe=p(other), pe_rows=10, pos0=2, xs=1.0, alpha=p(third), B=1, T=8,
                 y=p(third, 64), flag=ctypes.cast(flag, ctypes.c_void_p))
        a.update(kw)
        return L.amp_embed_pos(a["tok"], a["w"], a["rows"], a["D"], a["pe"], a["pe_rows"], a["pos0"], a["xs"], a["alpha"], a["B"], a["T"], a["y"],
                               a["flag"], None)
    for kw in (dict(tok=None), dict(w=None), dict(pe=None), dict(alpha=None), dict(y=None), dict(flag=None), dict(rows=0), dict(D=0), dict(B=0),
               dict(T=0), dict(pe_rows=0), dict(pos0=-1), dict(pos0=3), dict(T=9)):
        assert embed(**kw) == INV, kw
        assert b"amp_embed_pos" in L.amp_last_error(), kw
    assert embed(B=70000) == _lib.AMP_ERR_UNSUPPORTED
