"""MaskGCT on the CPU: the fp32 restatement (tests/maskgct_ref.py) against the golden outputs of the REAL reference classes
(tests/golden/make_golden_maskgct.py), the decidedness of every golden run, the state_dict keys, the constructor rules, the eval-only refusals
and the ABI surface.  No GPU.

The restatement performs the reference's torch operations in the reference's order.  On the machine that wrote the goldens it reproduces every
one of them BIT FOR BIT in fp32 -- the generator asserts ``torch.equal`` on every stored step's embeds and on the tokens before it stores them,
and this test measured 0 on the forwards there.  Another CPU's BLAS rounds a Linear differently (seen on another host: the forwards were not
bit-equal), so here the continuous outputs are held to the bound of tests/test_oracle_fmt.py, 2e-5 relative to max(1, |golden|max), with the
measured distance printed; the TOKENS are compared exactly everywhere, which the decidedness of every run is there to allow."""
import ctypes
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import maskgct_ref as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 2e-5


def dist(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
HPS = {"s2a": M.small_hp_s2a(), "t2s": M.small_hp_t2s()}


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "golden_maskgct.npz")))
    g.update(np.load(os.path.join(GOLDEN, "golden_maskgct_embeds.npz")))
    return g


@pytest.fixture(scope="module")
def sds(gold):
    return {k: M.synth_state_dict(k, HPS[k], int(gold["seed"])) for k in HPS}


def _draws(gold, name):
    return [torch.from_numpy(gold[f"{name}_u{i}"]) for i in range(int(gold[f"{name}_ndraws"]))]


def test_estimator_forwards_reproduce_the_golden(gold, sds):
    valid = int(gold["valid"])
    cast = lambda sd, dt: {k: v.to(dt) for k, v in sd.items()}
    for dtype in (torch.float32, torch.float64):
        ds = []
        for T in (37, 150):
            x, t, cond, mask = (v.to(dtype) for v in M.diffllama_inputs(HPS["s2a"], T, valid))
            ds.append(dist(M.diffllama_forward(cast(sds["s2a"], dtype), HPS["s2a"], x, t, cond, mask), gold[f"dl_y_{T}"]))
        x, t, ph, mask, pmask = (v.to(dtype) for v in M.prefix_inputs(HPS["t2s"], valid))
        ds.append(dist(M.prefix_forward(cast(sds["t2s"], dtype), HPS["t2s"], x, t, mask, ph, pmask), gold["px_y_phones"]))
        ds.append(dist(M.prefix_forward(cast(sds["t2s"], dtype), HPS["t2s"], x, t, mask), gold["px_y_plain"]))
        print(f"{dtype}: relative distance from the goldens {ds}")
        assert max(ds) <= REL


@pytest.mark.parametrize("name", list(M.RUNS))
def test_reverse_diffusion_reproduces_the_golden_and_is_decided(gold, sds, name):
    """the tokens exactly, every stored step's embeds within the bound, the number and shapes of the draws; and the run is decided: zero
    undecided comparisons"""
    kind, cfg, gt = M.RUNS[name]
    hp, sd = HPS[kind], sds[kind]
    inp = M.sampler_inputs(kind, hp, int(gold[f"{name}_seed"]))
    draws, rec = _draws(gold, name), []
    replay = M.Replay(draws)
    y = M.golden_run(kind, sd, hp, inp, cfg, gt, replay, record=rec)
    assert replay.i == len(draws)
    assert torch.equal(y, torch.from_numpy(gold[f"{name}_y"]))
    if f"{name}_embeds" in gold:
        d_emb = dist(torch.stack(rec), gold[f"{name}_embeds"])
        print(f"{name}: every step's embeds, relative distance from the golden {d_emb:.3e}")
        assert d_emb <= REL
    d = M.decidedness(lambda dtype, trace, teacher: M.golden_run(kind, sd, hp, inp, cfg, gt, M.Replay(draws), dtype, trace=trace, teacher=teacher))
    print(f"{name}: tau (logit, noisy, score) {d['tau']}, smallest gap / tau {d['worst']}, undecided {d['undecided']}")
    assert d["undecided"] == 0
    assert torch.equal(d["out"], y)                    # the fp64 trajectory gives the golden's tokens


def test_goldens_tell_wrong_variants_apart(gold, sds):
    """k by ``floor`` (6 of 64 instead of 7; 12 of 128 instead of 13) and the confidence taken at the sampling temperature instead of 1 both
    miss the golden tokens of at least one run (the 13th of 128 logits seldom wins: the T2S run alone tells ``floor`` apart by one token or none)"""
    floor_k = lambda V, thres: math.floor((1 - thres) * V)
    assert floor_k(64, 0.9) == 6 and M.top_k_count(64, 0.9) == 7
    for kw in (dict(k_of=floor_k), dict(score_temperature=0.3)):
        differ = {}
        for name in ("s2a_cfg25", "t2s_cfg25"):
            kind, cfg, gt = M.RUNS[name]
            inp = M.sampler_inputs(kind, HPS[kind], int(gold[f"{name}_seed"]))
            got = M.golden_run(kind, sds[kind], HPS[kind], inp, cfg, gt, M.Replay(_draws(gold, name)), **kw)
            differ[name] = int((got != torch.from_numpy(gold[f"{name}_y"])).sum())
        print(f"{list(kw)}: tokens that differ from the golden {differ}")
        assert max(differ.values()) > 0, kw


def test_state_dict_keys_match_the_reference():
    """the real classes' keys, minus the ones that carry nothing of the computation, are this package's; a reference checkpoint loads strictly"""
    from amphion_amd.models.tts.maskgct import MaskGCT_S2A, MaskGCT_T2S

    with open(os.path.join(GOLDEN, "keys_maskgct.json")) as f:
        ref = json.load(f)
    for kind, cls in (("s2a", MaskGCT_S2A), ("t2s", MaskGCT_T2S)):
        m = cls(**HPS[kind])
        ours = m.state_dict()
        kept = [k for k in ref[kind] if not k.endswith(M.DROPPED)]
        assert sorted(ours) == sorted(kept) and sorted(ours) == sorted(M.state_dict_shapes(kind, HPS[kind]))
        assert {k: tuple(v.shape) for k, v in ours.items()} == M.state_dict_shapes(kind, HPS[kind])
        ckpt = dict(M.synth_state_dict(kind, HPS[kind], 3))
        for k in ref[kind]:                             # a checkpoint of the real class: every key it has, the dropped ones included
            if k not in ckpt:
                ckpt[k] = torch.zeros(0, 256) if k.endswith("embed_tokens.weight") else torch.zeros(32)
        ckpt["diff_estimator.layers.0.self_attn.rotary_emb.inv_freq"] = torch.zeros(32)
        m.load_state_dict(ckpt, strict=True)
        assert torch.equal(m.state_dict()["mask_emb.weight"], ckpt["mask_emb.weight"])
    assert "diff_estimator.embed_tokens.weight" in ref["s2a"] and "diff_estimator.embed_tokens.weight" not in ref["t2s"]


def test_cfg_overrides_and_refusals():
    from amphion_amd.models.tts.maskgct import DiffLlama, DiffLlamaPrefix, MaskGCT_S2A, MaskGCT_T2S

    cfg = types.SimpleNamespace(hidden_size=128, num_heads=2, num_layers=1, codebook_size=16, num_quantizer=2)
    m = MaskGCT_S2A(hidden_size=1024, num_layers=16, cond_codebook_size=33, cfg=cfg)          # an attribute of cfg overrides the argument
    assert (m.hidden_size, m.num_layers, m.num_heads, m.codebook_size, m.num_quantizer, m.cond_codebook_size) == (128, 1, 2, 16, 2, 33)
    assert m.token_emb[1].weight.shape == (16, 128) and len(m.to_logits) == 2 and m.cond_emb.weight.shape == (33, 128)
    cfg = types.SimpleNamespace(hidden_size=192, num_heads=2, num_layers=1, use_phone_cond=False)
    t = MaskGCT_T2S(cond_codebook_size=40, cfg=cfg)
    assert t.hidden_size == 192 and not hasattr(t, "phone_emb") and not hasattr(t.diff_estimator, "cond_mlp") and t.to_logit.out_features == 40
    assert bool((MaskGCT_T2S(hidden_size=128, num_heads=2, num_layers=1).phone_emb.weight[1023] == 0).all())    # padding_idx
    for name, args in (("forward", (None, None)), ("compute_loss", (None, None)), ("loss_t", (None, None, None)), ("forward_diffusion", (None, None)),
                       ("mask_layer", (None,))):
        with pytest.raises(NotImplementedError, match="eval-only"):
            getattr(m, name)(*args)
        if name != "mask_layer":
            with pytest.raises(NotImplementedError, match="eval-only"):
                getattr(t, name)(*args)
    DiffLlama(hidden_size=192, num_heads=2, num_layers=1)                                      # dk = 96
    for cls in (DiffLlama, DiffLlamaPrefix):
        with pytest.raises(NotImplementedError):
            cls(hidden_size=256, num_heads=2, num_layers=1)                                    # dk = 128
        with pytest.raises(NotImplementedError):
            cls(hidden_size=96, num_heads=2, num_layers=1)                                     # dk = 48


def test_next_mask_count_is_the_reference_expression():
    """the host-side schedule: fp32 on the CPU, the product formed as the reference forms it"""
    from amphion_amd.models.tts.maskgct._sampler import next_mask_count, top_k_count

    for steps in (1, 2, 4, 5, 25, 40, 50):
        for T in (1, 26, 500, 1333):
            for i in range(steps + 1):
                t = 1.0 - i / steps if i < steps else 0.0
                t = [1.0 - j * (1.0 / steps) for j in range(steps)][i] if i < steps else 0.0
                want = (torch.sin((t * torch.ones(2)) * np.pi / 2) * T).long()[0].item()
                assert next_mask_count(t, T) == want == M.next_mask_count(t, T)
    assert top_k_count(8192, 0.98) == 164 and top_k_count(1024, 0.98) == 21 and top_k_count(64, 0.9) == 7


def test_abi_surface():
    """the symbol is exported and bound, the version says so, and the host-side refusals need no device"""
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 154
    assert "amp_mask_sample" in _lib.EXPORTED_SYMBOLS
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "amphion_hip.h")) as f:
        assert "int amp_mask_sample(" in f.read()
    buf = (ctypes.c_float * 64)()
    ids = (ctypes.c_longlong * 8)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    one = ctypes.c_float(1.0)
    assert L.amp_mask_sample(None, 0, 1, 8, 4, 2, None, one, None, None, None) == _lib.AMP_ERR_INVALID
    for V, k in ((1, 1), (8193, 2), (8, 0), (8, 9)):       # refused on the host before anything is launched: the pointers are never read
        assert L.amp_mask_sample(p(buf), 0, 1, V, 4, k, None, one, p(ids), p(buf), None) == _lib.AMP_ERR_INVALID, (V, k)
        assert L.amp_last_error()
