"""Writes golden_ar.npz and keys_ar.json from the REAL ``AutoregressiveTransformer`` of an Amphion checkout, on the CPU:

    python tests/golden/make_golden_ar.py /path/to/Amphion

The reference constructs its own ``LlamaConfig`` with keywords, so the class runs under transformers 5 as it stands; only the IMPORT of its
sibling global_encoder.py needs help (a positional ``LlamaConfig(0, 256, 1024, 1, 1)`` default, make_golden_fmt.py's problem): see
``import_reference``.

``forward``: logits and loss at B = 2 with ragged masks, item 1 shorter on both sides.

``generate``: the real method, with HF's own processors, warpers, cache and stopping.  One substitution for its duration: ``torch.multinomial``
is the exponential race ``argmax(p / q)`` with q = ``torch.empty(V).exponential_()`` drawn under the run's seed and STORED -- the race is what
multinomial runs inside, but it does not consume the generator the way ``exponential_`` does, so the draw has to be an input for anybody to
replay the run.  The runs are searched over seeds until each is DECIDED (ar_ref.decidedness: every discrete decision at least 4 tau from
its boundary) and the fp32 restatement reproduces the reference token for token; among them one that ends on EOS after ``min_new_tokens``
and before ``max_length``, one stopped by ``max_length``, one with ``repeat_penalty`` 1.1, one with ``top_p`` 1.0, one per head dimension.

The npz holds outputs, seeds and the q draws; weights and inputs regenerate from the seeds (ar_ref.synth_*)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ar_ref as A  # noqa: E402

SD_SEED, FWD_SEED, GEN_SEED, MAX_LENGTH, MIN_NEW, RUNS = A.SD_SEED, A.FWD_SEED, A.GEN_SEED, A.MAX_LENGTH, A.MIN_NEW, A.RUNS


def import_reference(amphion_root):
    import transformers

    # global_encoder.py (imported by ar_model.py) has the default ``config=LlamaConfig(0, 256, 1024, 1, 1)``, evaluated at import, and is
    # reached AFTER ar_model.py's own ``from transformers import LlamaForCausalLM`` has loaded the Llama modules: from then on
    # ``from transformers import LlamaConfig`` no longer returns an attribute set on the package, so the five positions are mapped to their
    # keywords in the class's own __init__ while the reference is imported
    real = transformers.LlamaConfig
    init = real.__init__

    def positional(self, *args, **kw):
        names = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads")
        kw.update(dict(zip(names, args)))
        init(self, **kw)

    sys.path.insert(0, amphion_root)
    real.__init__ = positional
    try:
        from models.vc.autoregressive_transformer.ar_model import AutoregressiveTransformer
    finally:
        real.__init__ = init
    return AutoregressiveTransformer


def real_generate(model, ii, po, seed, kw):
    """the real generate with torch.multinomial replaced by the stored race -> (raw new tokens incl. a closing EOS, stripped tokens, q)"""
    g = torch.Generator().manual_seed(seed)
    qs, raw = [], []
    real = torch.multinomial

    def raced(probs, num_samples, *a, **k):
        q = torch.empty(probs.shape[-1]).exponential_(generator=g)
        qs.append(q)
        tok = torch.argmax(probs / q, dim=-1, keepdim=True)
        raw.append(int(tok))
        return tok

    torch.multinomial = raced
    try:
        gen = model.generate(ii, prompt_output_ids=po, max_length=MAX_LENGTH, min_new_tokens=MIN_NEW, **kw)
    finally:
        torch.multinomial = real
    return torch.tensor(raw), gen, torch.stack(qs)


def main(amphion_root):
    torch.manual_seed(0)
    Cls = import_reference(amphion_root)
    out, keys = {}, None
    models = {}
    for dk in (96, 64):
        hp = A.small_hp(dk)
        model = Cls(**hp).eval()
        if keys is None:
            keys = list(model.state_dict().keys())
        else:
            assert keys == list(model.state_dict().keys())
        sd = A.synth_state_dict(hp, SD_SEED)
        model.load_state_dict(sd)
        models[dk] = (hp, model, sd, A.cast(sd, torch.float64))
        with torch.no_grad():
            o = model(*A.synth_forward_inputs(hp, FWD_SEED))
        out[f"fwd_logits_{dk}"], out[f"fwd_loss_{dk}"] = o.logits.numpy(), o.loss.numpy()
        print(f"forward dk={dk}: logits {tuple(o.logits.shape)} max |l| {float(o.logits.abs().max()):.3f} loss {float(o.loss):.4f}")
    assert keys == A.state_dict_keys(A.small_hp(96)), "ar_ref.state_dict_keys is not the real class's order"
    for name, (dk, kw, end) in RUNS.items():
        hp, model, sd, sd64 = models[dk]
        ii, po = A.synth_generate_inputs(hp, GEN_SEED)
        n0 = ii.shape[1] + 2 + po.shape[1] + 1
        for seed in range(1, 200):
            raw, gen, q = real_generate(model, ii, po, seed, kw)
            ended = "eos" if int(raw[-1]) == A.special(hp)["output_eos"] and n0 + len(raw) < MAX_LENGTH else "max"
            if end is not None and ended != end:
                continue
            mine, tau, gap = A.decidedness(sd, sd64, hp, ii, po, A.Replay(q), max_length=MAX_LENGTH, min_new_tokens=MIN_NEW, **kw)
            same = mine.tolist() == raw.tolist()
            print(f"{name} seed {seed}: {len(raw)} tokens, ends on {ended}, tau {tau:.3e}, gap {gap:.3e} = {gap / tau:.1f} tau, restatement "
                  f"{'equal' if same else 'DIFFERENT'}")
            if same and gap >= 4 * tau:
                break
        else:
            raise SystemExit(f"{name}: no decided run in 200 seeds")
        out[f"gen_{name}_seed"], out[f"gen_{name}_raw"], out[f"gen_{name}_tokens"] = np.int64(seed), raw.numpy(), gen.numpy()
        out[f"gen_{name}_q"] = q.numpy()
    np.savez_compressed(os.path.join(HERE, "golden_ar.npz"), **out)
    with open(os.path.join(HERE, "keys_ar.json"), "w") as f:
        json.dump(keys, f, indent=0)
    print("wrote", {k: getattr(v, "shape", ()) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
