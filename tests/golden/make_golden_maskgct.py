"""Writes tests/golden/golden_maskgct.npz and keys_maskgct.json from the REAL reference classes (models/tts/maskgct/{maskgct_t2s,maskgct_s2a,
llama_nar}.py) on the CPU:

    python tests/golden/make_golden_maskgct.py /path/to/Amphion

The reference is imported the way make_golden_fmt.py does it: ``transformers.LlamaConfig`` takes the five positional arguments of
``LlamaConfig(0, 256, 1024, 1, 1)`` while the module is imported, and the estimators' forwards are composed from the real instances' own
submodules (cond_mlp, diff_step_embedding, diff_step_mlp, every layer's norms / self_attn / mlp, norm), their own
``_prepare_decoder_attention_mask`` and HF's LlamaRotaryEmbedding in ``forward``'s order (llama_nar.py:295-424, 522-659), bound as the
instances' ``diff_estimator.forward``; the REAL ``reverse_diffusion`` loops run on top under a torch seed.  The uniform draws of a run are
recovered by running the restatement (tests/maskgct_ref.py) under the same seed with a recording noise function: same shapes in the same order.

Every stored run is DECIDED (maskgct_ref.decidedness) with every gap at 4 tau or more: seeds are searched from the first candidate up until that
holds, and recorded.
The npz holds outputs, seeds and the drawn noise only: the weights and the inputs regenerate from their seeds (maskgct_ref.synth_state_dict,
diffllama_inputs, prefix_inputs, sampler_inputs); every step's guided embeds of one S2A and one T2S run go to golden_maskgct_embeds.npz.

Seen while writing this (the T2S classifier-free quirk, maskgct_t2s.py:301-308): with 9 phones <= prompt 11 the unconditional branch runs (the
slice ``phone_mask[:, prompt_len:]`` is empty); with 12 phones > prompt 11 the real class fails with "RuntimeError: The size of tensor a (26) must
match the size of tensor b (27) at non-singleton dimension 3" where the attention adds its mask (the mask is one key longer than the sequence)
-- printed below when this script runs."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import maskgct_ref as M  # noqa: E402

SEED = M.GOLDEN_SEED
FWD_T = (37, 150)
VALID = 29               # item 1 of the forwards is masked beyond this frame
TP, TT, NPH = M.TP, M.TT, M.NPH
S2A_STEPS, S2A_THRES, S2A_TEMP = M.S2A_STEPS, M.S2A_THRES, M.S2A_TEMP
T2S_STEPS, T2S_THRES, T2S_TEMP = M.T2S_STEPS, M.T2S_THRES, M.T2S_TEMP
RESCALE = M.RESCALE
RUNS = [("s2a_cfg0", "s2a", 0.0, False), ("s2a_cfg25", "s2a", 2.5, False), ("s2a_gt", "s2a", 2.5, True),
        ("t2s_cfg0", "t2s", 0.0, False), ("t2s_cfg25", "t2s", 2.5, False)]
MARGIN = 4.0             # a stored run's smallest gap is 4 tau or more: the GPU tests allow the kernels 4 x the fp32 restatement's distance from fp64
RECORDED = ("s2a_cfg25", "t2s_cfg25")      # every step's guided embeds are stored for these


def import_reference(amphion_root):
    import transformers

    real = transformers.LlamaConfig

    class PositionalLlamaConfig(real):
        def __init__(self, *args, **kw):
            names = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads")
            kw.update(dict(zip(names, args)))
            super().__init__(**kw)

    sys.path.insert(0, amphion_root)
    transformers.LlamaConfig = PositionalLlamaConfig
    try:
        from models.tts.maskgct.maskgct_s2a import MaskGCT_S2A
        from models.tts.maskgct.maskgct_t2s import MaskGCT_T2S
    finally:
        transformers.LlamaConfig = real
    return MaskGCT_S2A, MaskGCT_T2S


def _walk(est, h, step, x_mask):
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding

    B, T, _ = h.shape
    if x_mask is None:
        x_mask = torch.ones((B, T), dtype=torch.bool)
    mask = est._prepare_decoder_attention_mask(x_mask, (B, T), h, 0)
    rotary = LlamaRotaryEmbedding(config=est.layers[0].self_attn.config)
    cos, sin = rotary(h, torch.arange(T, dtype=torch.long)[None])
    for layer in est.layers:
        res = h
        y = layer.input_layernorm(h, cond_embedding=step)
        y = layer.self_attn(hidden_states=y, position_embeddings=(cos, sin), attention_mask=mask)[0]
        h = res + y
        res = h
        h = res + layer.mlp(layer.post_attention_layernorm(h, cond_embedding=step))
    return est.norm(h, cond_embedding=step)


def composed_diffllama(est, x, diffusion_step, cond, x_mask):
    """llama_nar.py:295-424"""
    cond_embedding = est.cond_mlp(cond)
    step = est.diff_step_mlp(est.diff_step_embedding(diffusion_step).to(x.device))
    return _walk(est, x + cond_embedding, step, x_mask)


def composed_prefix(est, x, diffusion_step, x_mask, phone_embedding=None, phone_mask=None):
    """llama_nar.py:522-659"""
    if est.use_phone_cond and phone_embedding is not None:
        phone_embedding = est.cond_mlp(phone_embedding)
        phone_length = phone_embedding.shape[1]
        inputs_embeds = torch.cat([phone_embedding, x], dim=1)
        attention_mask = torch.cat([phone_mask, x_mask], dim=1)
    else:
        inputs_embeds, attention_mask, phone_length = x, x_mask, 0
    step = est.diff_step_mlp(est.diff_step_embedding(diffusion_step).to(x.device))
    return _walk(est, inputs_embeds, step, attention_mask)[:, phone_length:]


def load(model, kind, hp, keys_out):
    keys_out[kind] = list(model.state_dict())
    sd = M.synth_state_dict(kind, hp, SEED)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(M.DROPPED) for k in missing), (missing, unexpected)
    return sd


inputs = M.sampler_inputs


restated = M.golden_run


def main(amphion_root):
    S2A, T2S = import_reference(amphion_root)
    hps = {"s2a": M.small_hp_s2a(), "t2s": M.small_hp_t2s()}
    models = {"s2a": S2A(**hps["s2a"]).eval(), "t2s": T2S(**hps["t2s"]).eval()}
    keys, sds = {}, {}
    for kind in ("s2a", "t2s"):
        sds[kind] = load(models[kind], kind, hps[kind], keys)
    with open(os.path.join(HERE, "keys_maskgct.json"), "w") as f:
        json.dump(keys, f, indent=0)
    es, et = models["s2a"].diff_estimator, models["t2s"].diff_estimator
    es.forward = lambda x, t, cond, x_mask: composed_diffllama(es, x, t, cond, x_mask)
    et.forward = lambda x, t, x_mask, phone_embedding=None, phone_mask=None: composed_prefix(et, x, t, x_mask, phone_embedding, phone_mask)
    out, embeds = {"seed": np.int64(SEED), "valid": np.int64(VALID)}, {}
    with torch.no_grad():
        # ---- estimator forwards
        for T in FWD_T:
            x, t, cond, mask = M.diffllama_inputs(hps["s2a"], T, VALID)
            y = es(x, t, cond, mask)
            out[f"dl_y_{T}"] = y.numpy()
            print(f"DiffLlama.forward T={T}: max |y| {float(y.abs().max()):.3f}")
        x, t, ph, mask, pmask = M.prefix_inputs(hps["t2s"], VALID)
        out["px_y_phones"] = et(x, t, mask, phone_embedding=ph, phone_mask=pmask).numpy()
        out["px_y_plain"] = et(x, t, mask).numpy()
        # ---- the samplers: search each run's seed until the run is decided
        for name, kind, cfg, gt in RUNS:
            hp, sd, model = hps[kind], sds[kind], models[kind]
            for seed in range(1000, 1400):
                inp = inputs(kind, hp, seed)
                torch.manual_seed(seed)
                draws = []

                def recording(shape):
                    draws.append(torch.zeros(shape).uniform_(0, 1))
                    return draws[-1]

                rec32 = []
                y32 = restated(kind, sd, hp, inp, cfg, gt, recording, record=rec32)
                d = M.decidedness(lambda dtype, trace, teacher: restated(kind, sd, hp, inp, cfg, gt, M.Replay(draws), dtype, trace=trace, teacher=teacher))
                if d["undecided"] == 0 and min(d["worst"]) >= MARGIN and torch.equal(d["out"], y32):
                    break
                print(f"{name}: seed {seed} has {d['undecided']} undecided comparisons, smallest gap / tau {min(d['worst']):.2f}, next")
            else:
                raise SystemExit(f"{name}: no decided seed")
            torch.manual_seed(seed)
            rec = []                                   # the guided embeds of every step: what the real class hands to to_logit(s)
            heads = list(model.to_logits) if kind == "s2a" else [model.to_logit]
            hooks = [m.register_forward_pre_hook(lambda mod, args: rec.append(args[0].clone())) for m in heads]
            if kind == "s2a":
                y = model.reverse_diffusion(model.cond_emb(inp["codes"]), inp["prompt"], temp=S2A_TEMP, filter_thres=S2A_THRES,
                                            gt_code=inp["gt"] if gt else None, n_timesteps=S2A_STEPS, cfg=cfg, rescale_cfg=RESCALE)
            else:
                y = model.reverse_diffusion(inp["prompt"], TT, inp["phones"], temp=T2S_TEMP, filter_thres=T2S_THRES, n_timesteps=T2S_STEPS, cfg=cfg,
                                            rescale_cfg=RESCALE)
            for hk in hooks:
                hk.remove()
            assert len(rec) == len(rec32) and all(torch.equal(a, b) for a, b in zip(rec, rec32)), "embeds differ"
            print(f"{name}: seed {seed}, taus {d['tau']}, smallest gap / tau {d['worst']}, restatement equal: {torch.equal(y, y32)}")
            assert torch.equal(y, y32), "the fp32 restatement does not reproduce the reference"
            out[f"{name}_seed"], out[f"{name}_y"] = np.int64(seed), y.numpy()
            out[f"{name}_ndraws"] = np.int64(len(draws))
            for i, u in enumerate(draws):
                out[f"{name}_u{i}"] = u.numpy()
            if name in RECORDED:
                embeds[f"{name}_embeds"] = torch.stack(rec).numpy()
        # ---- the T2S classifier-free quirk
        inp = inputs("t2s", hps["t2s"], 1)
        torch.manual_seed(1)
        try:
            models["t2s"].reverse_diffusion(inp["prompt"], TT, torch.randint(0, 1023, (2, TP + 1)), n_timesteps=2, cfg=2.5)
            print("P = 12 > prompt_len = 11 with cfg > 0: the reference ran")
        except Exception as e:  # noqa: BLE001
            print(f"P = 12 > prompt_len = 11 with cfg > 0: the reference raises {type(e).__name__}: {e}")
    for fn, d in (("golden_maskgct.npz", out), ("golden_maskgct_embeds.npz", embeds)):      # two files: each within the size limit of a committed file
        np.savez_compressed(os.path.join(HERE, fn), **d)
        print("wrote", fn, os.path.getsize(os.path.join(HERE, fn)), "bytes;", len(d), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
