"""Writes golden_valle.npz and keys_valle.json from the REAL ``VALLE`` of an Amphion checkout, on the CPU:

    python tests/golden/make_golden_valle.py /path/to/Amphion

The class imports ``torchmetrics`` (its training metrics) and, through ``utils.util``, ``json5``, ``ruamel_yaml`` and ``lhotse``; none is needed
to run ``inference`` / ``continual``, so absent ones are stubbed for the import (``import_reference``).

``inference``: the real method.  One substitution for its duration: ``torch.multinomial`` is the exponential race ``argmax(p / q)`` with q =
``torch.empty(V).exponential_()`` drawn under the run's seed and STORED (make_golden_ar.py has the reasons).  The runs (valle_ref.RUNS: one that
ends on EOS with ``top_k = -100``, one that ends on the length cap with a text of 2 tokens, one with ``temperature`` 0.7 / ``top_k`` 10, one
with ``prefix_mode`` 1, one with ``prepend_bos``) are searched over seeds until each is DECIDED (valle_ref.decidedness: every discrete decision
-- top-k membership, the race's winner, the stop test's arg-max, every NAR arg-max of every level and frame -- at least 4 tau from its
boundary), lasts 10 - 40 new tokens, and the fp32 restatement reproduces the reference token for token on both of its paths.
``continual``: one more small model with 8 quantizers, under the same rule.

The npz holds outputs, seeds and the q draws; weights and inputs regenerate from the seeds (valle_ref.synth_*)."""
import importlib
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import valle_ref as V  # noqa: E402


class _Anything:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return self


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """every module under the absent packages imports as an empty package whose attributes are all ``_Anything``"""

    def __init__(self, roots):
        self.roots = tuple(roots)

    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in self.roots:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = types.ModuleType(spec.name)
        m.__path__ = []
        m.__getattr__ = lambda attr: _Anything
        return m

    def exec_module(self, module):
        pass


def import_reference(amphion_root):
    absent = []
    for name in ("torchmetrics", "lhotse", "json5", "ruamel_yaml"):
        try:
            importlib.import_module(name)
        except ImportError:
            absent.append(name)
    sys.meta_path.append(_StubFinder(absent))
    sys.path.insert(0, amphion_root)
    from models.tts.valle.valle import VALLE
    return VALLE


def real_inference(model, x, x_lens, y, enroll, seed, kw):
    """the real inference with torch.multinomial replaced by the stored race -> (codes [1, n, nq], q [steps, V])"""
    g = torch.Generator().manual_seed(seed)
    qs = []
    real = torch.multinomial

    def raced(probs, num_samples, *a, **k):
        q = torch.empty(probs.shape[-1]).exponential_(generator=g)
        qs.append(q)
        return torch.argmax(probs / q, dim=-1, keepdim=True)

    torch.multinomial = raced
    try:
        with torch.no_grad():
            codes = model.inference(x, x_lens, y, enroll, **kw)
    finally:
        torch.multinomial = real
    return codes, torch.stack(qs)


def main(amphion_root):
    torch.manual_seed(0)
    Cls = import_reference(amphion_root)
    ns = lambda hp: types.SimpleNamespace(**hp)
    out = {}
    keys = list(Cls(ns(V.make_hp())).state_dict().keys())
    assert keys == V.state_dict_keys(V.make_hp()), "valle_ref.state_dict_keys is not the real class's order"
    for name, (over, text_len, kw, end) in V.RUNS.items():
        hp = V.make_hp(**over)
        model = Cls(ns(hp)).eval()
        assert list(model.state_dict().keys()) == V.state_dict_keys(hp)
        sd = V.synth_state_dict(hp, V.SD_SEED)
        model.load_state_dict(sd)
        sd64 = V.cast(sd, torch.float64)
        x, x_lens, y, enroll = V.synth_inputs(hp, V.IN_SEED, text_len)
        for seed in range(1, 1000):
            try:
                codes, q = real_inference(model, x, x_lens, y, enroll, seed, kw)
            except SyntaxError:
                continue
            n = codes.shape[1]
            ended = "cap" if n + int(hp["prepend_bos"]) > 16 * text_len else "eos"
            if ended != end or (ended == "eos" and not 10 <= n <= 40):
                continue
            mine, mine_end, tau, gap = V.decidedness(sd, sd64, hp, x, x_lens, y, enroll, V.Replay(q), path="cache", **kw)
            again, _ = V.inference(sd, hp, x, x_lens, y, enroll, V.Replay(q), path="recompute", **kw)
            same = mine.tolist() == codes.tolist() and again.tolist() == codes.tolist() and mine_end == ended
            print(f"{name} seed {seed}: {n} tokens, ends on {ended}, tau {tau:.3e}, gap {gap:.3e} = {gap / tau:.1f} tau, restatement "
                  f"{'equal' if same else 'DIFFERENT'}")
            if same and gap >= 4 * tau:
                break
        else:
            raise SystemExit(f"{name}: no decided run in 1000 seeds")
        out[f"inf_{name}_seed"], out[f"inf_{name}_codes"], out[f"inf_{name}_q"] = np.int64(seed), codes.numpy(), q.numpy()
        out[f"inf_{name}_end"] = np.array(ended)
    hp = V.make_hp(**V.CONTINUAL_HP)
    model = Cls(ns(hp)).eval()
    for sd_seed in range(V.SD_SEED, V.SD_SEED + 50):
        sd = V.synth_state_dict(hp, sd_seed)
        model.load_state_dict(sd)
        x, x_lens, y, _ = V.synth_inputs(hp, V.IN_SEED, V.CONTINUAL_TEXT, V.CONTINUAL_FRAMES)
        with torch.no_grad():
            codes = model.continual(x, x_lens, y)
        mine, tau, gap = V.continual_decidedness(sd, V.cast(sd, torch.float64), hp, x, x_lens, y)
        same = mine.tolist() == codes.tolist()
        print(f"continual weights {sd_seed}: tau {tau:.3e}, gap {gap:.3e} = {gap / tau:.1f} tau, restatement {'equal' if same else 'DIFFERENT'}")
        if same and gap >= 4 * tau:
            break
    else:
        raise SystemExit("continual: no decided run in 50 weight seeds")
    out["continual_sd_seed"], out["continual_codes"] = np.int64(sd_seed), codes.numpy()
    np.savez_compressed(os.path.join(HERE, "golden_valle.npz"), **out)
    with open(os.path.join(HERE, "keys_valle.json"), "w") as f:
        json.dump(keys, f, indent=0)
    print("wrote", {k: getattr(v, "shape", ()) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
