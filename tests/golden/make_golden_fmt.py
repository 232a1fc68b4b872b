"""Writes tests/golden/golden_fmt.npz and keys_fmt.json from the REAL reference classes (models/vc/flow_matching_transformer/fmt_model.py:
FlowMatchingTransformer around llama_nar.py: DiffLlama) on the CPU:

    python tests/golden/make_golden_fmt.py /path/to/Amphion

The reference was written against transformers 4.3x and does not run as it stands under transformers 5:

  * ``DiffLlama.__init__`` has the default ``config=LlamaConfig(0, 256, 1024, 1, 1)`` (llama_nar.py:137), evaluated at import; LlamaConfig no
    longer takes positional arguments.  While the reference module is imported, ``transformers.LlamaConfig`` is a subclass that maps those five
    positions to their keywords (vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads).
  * ``LlamaNARDecoderLayer.forward`` calls ``self.self_attn(..., position_ids=...)`` (llama_nar.py:98-105); LlamaAttention now takes the rotary
    tables as ``position_embeddings`` and returns two values.  ``composed_forward`` below runs the real instance's own submodules (cond_mlp,
    mel_mlp, diff_step_embedding, diff_step_mlp, every layer's input_layernorm / self_attn / post_attention_layernorm / mlp, norm, mel_out_mlp),
    its own ``_prepare_decoder_attention_mask`` and HF's own LlamaRotaryEmbedding in ``forward``'s order (llama_nar.py:236-397).

For ``reverse_diffusion`` that composition is bound as the instance's ``diff_estimator.forward`` and the REAL loop (fmt_model.py:228-283) runs
under a torch seed; the noise it drew is recovered by drawing again under the same seed and stored.

The npz holds inputs, outputs and the seed only: the weights regenerate from the seed (tests/fmt_ref.py: synth_state_dict)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import fmt_ref as R  # noqa: E402

SEED = 53
FWD_T = (37, 150)
VALID = 29               # item 1 of the forwards is masked beyond this frame
TP, TT, STEPS = 11, 26, 4
CFGS = (0.0, 2.0)
RD_SEED = 1234


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
        from models.vc.flow_matching_transformer.fmt_model import FlowMatchingTransformer
    finally:
        transformers.LlamaConfig = real
    return FlowMatchingTransformer


def composed_forward(est, x, diffusion_step, cond, x_mask, hidden=None):
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding

    B, T, _ = x.shape
    cond_embedding = est.cond_mlp(cond)
    x = est.mel_mlp(x)
    step = est.diff_step_mlp(est.diff_step_embedding(diffusion_step).to(x.dtype))
    h = x + cond_embedding
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
        if hidden is not None:
            hidden.append(h.clone())
    return est.mel_out_mlp(est.norm(h, cond_embedding=step))


def main(amphion_root):
    FMT = import_reference(amphion_root)
    hp = R.small_hp()
    model = FMT(**hp).eval()
    with open(os.path.join(HERE, "keys_fmt.json"), "w") as f:
        json.dump(list(model.state_dict()), f, indent=0)
    missing, unexpected = model.load_state_dict(R.synth_state_dict(hp, SEED), strict=False)
    assert not unexpected and all(k.endswith("rotary_emb.inv_freq") for k in missing), (missing, unexpected)
    est = model.diff_estimator
    est.forward = lambda x, t, cond, x_mask: composed_forward(est, x, t, cond, x_mask)
    out = {"seed": np.int64(SEED), "valid": np.int64(VALID), "rd_seed": np.int64(RD_SEED)}
    with torch.no_grad():
        for T in FWD_T:
            x, t, codes = R.synth_inputs(hp, 2, T, 100 + T)
            mask = torch.ones(2, T)
            mask[1, VALID:] = 0
            hidden = []
            y = composed_forward(est, x, t, model.cond_emb(codes), mask, hidden)
            out[f"fwd_x_{T}"], out[f"fwd_t_{T}"], out[f"fwd_codes_{T}"] = x.numpy(), t.numpy(), codes.numpy()
            out[f"fwd_y_{T}"], out[f"fwd_h0_{T}"] = y.numpy(), hidden[0].numpy()
            print(f"forward T={T}: max |y| {float(y.abs().max()):.3f}, max |h0| {float(hidden[0].abs().max()):.3f}")
        prompt, _, codes = R.synth_inputs(hp, 2, TP + TT, 300)
        prompt = prompt[:, :TP]
        out["rd_prompt"], out["rd_codes"] = prompt.numpy(), codes.numpy()
        torch.manual_seed(RD_SEED)
        out["rd_noise"] = torch.randn((2, TT, hp["mel_dim"]), dtype=torch.float32).numpy()
        for cfg in CFGS:
            torch.manual_seed(RD_SEED)
            y = model.reverse_diffusion(model.cond_emb(codes), prompt, n_timesteps=STEPS, cfg=cfg)
            out[f"rd_y_{cfg}"] = y.numpy()
            print(f"reverse_diffusion cfg={cfg}: max |y| {float(y.abs().max()):.3f}")
    np.savez_compressed(os.path.join(HERE, "golden_fmt.npz"), **out)
    print("wrote", {k: getattr(v, "shape", ()) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
