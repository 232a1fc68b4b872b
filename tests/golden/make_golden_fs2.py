"""Writes tests/golden/golden_fs2.npz, keys_fs2.json and keys_jets.json from the REAL reference classes (models/tts/fastspeech2/fs2.py:
FastSpeech2 and models/tts/jets/jets.py: Jets, around modules/transformer/{Models,Layers,SubLayers,Modules}.py) on the CPU:

    python tests/golden/make_golden_fs2.py /path/to/Amphion

What makes the class import and construct outside its recipe: MagicMock modules for the text front end's third-party packages (``text`` is
imported for ``len(symbols)`` only), a config object that answers both ``cfg.a.b`` and ``cfg["a"]`` (tests/fs2_ref.py: Cfg), and two temporary
``statistics.json`` files (plus ``spk2id.json`` for the multi-speaker run) under a temporary ``processed_dir``; for ``Jets`` also the stubs of
make_golden.install_stubs() and ``load_config`` replaced in ``models.tts.jets.jets`` while the constructor runs (it loads the HiFi-GAN recipe
from a path relative to the reference's root).  ``Jets.inference`` runs on the ragged batch; its wave is the largest stored item.

The npz holds inputs, outputs and the seed only: the weights regenerate from the seed (tests/fs2_ref.py: synth_state_dict).  Durations and
bins are discrete decisions, so the script keeps the first seed under which EVERY stored run is decided: each rounded duration and each bin
index of the fp64 restatement at least 4 tau from its boundary (tau: the fp32 restatement's distance from fp64 on the quantity the decision
reads) and the fp32 restatement reproducing the real class's d_rounded, mel_lens and bin indices exactly.  tau and the smallest gaps are
printed and stored per run."""
import json
import os
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import fs2_ref as R  # noqa: E402

RUNS = {
    "ragged": (dict(), [13, 9], (1.0, 1.0, 1.0)),
    "controls": (dict(), [13, 9], (1.2, 0.8, 1.25)),
    "long": (dict(max_seq_len=40), [45, 30], (1.0, 1.0, 1.0)),
    "frame_level": (dict(pitch_level="frame_level", energy_level="frame_level"), [13, 9], (1.0, 1.0, 1.0)),
    "multi_speaker": (dict(n_speaker=4), [13, 9], (1.0, 1.0, 1.0)),
}
STORED = ("output", "postnet_output", "p_predictions", "e_predictions", "log_d_predictions", "d_rounded", "mel_lens", "src_masks", "mel_masks")


def import_reference(amphion_root):
    for name in ("json5", "unidecode", "ruamel", "ruamel.yaml", "inflect", "g2p_en", "pypinyin", "phonemizer", "jieba", "cn2an", "eng_to_ipa",
                 "numba"):
        sys.modules.setdefault(name, MagicMock())
    sys.path.insert(0, amphion_root)
    import make_golden as mg

    mg.install_stubs()
    from models.tts.fastspeech2.fs2 import FastSpeech2
    from text.symbols import symbols
    import models.tts.jets.jets as jets_module

    return FastSpeech2, jets_module, len(symbols) + 1


def real_jets(jets_module, hp, sd, texts, lens, spk):
    real_load = jets_module.load_config
    jets_module.load_config = lambda path: R.Cfg(model=R.Cfg(hifigan=R.Cfg(**R.JETS_HIFIGAN)), preprocess=R.Cfg())
    try:
        with tempfile.TemporaryDirectory() as tmp:
            write_stats(tmp, hp)
            model = jets_module.Jets(R.make_cfg(hp, processed_dir=tmp))
    finally:
        jets_module.load_config = real_load
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    model.eval()
    with torch.no_grad():
        wav, d = model.inference({"texts": texts, "text_len": lens, "spk_id": spk})
    return wav, d, keys


def write_stats(root, hp, dataset="ds"):
    """statistics.json files whose normalised extremes are hp['stats'] (mean 0, std 1)"""
    s = hp["stats"]
    for sub, which in (("pitches", "pitch"), ("phone_pitches", "pitch"), ("energys", "energy"), ("phone_energys", "energy")):
        d = os.path.join(root, dataset, sub)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "statistics.json"), "w") as f:
            json.dump({dataset + "_" + dataset: {"voiced_positions": {"mean": 0.0, "std": 1.0},
                                                 "total_positions": {"min": s[which + "_min"], "max": s[which + "_max"]}}}, f)
    with open(os.path.join(root, dataset, "spk2id.json"), "w") as f:
        json.dump({f"spk{i}": i for i in range(max(1, hp["n_speaker"]))}, f)


def real_run(FastSpeech2, hp, sd, texts, lens, spk, controls):
    with tempfile.TemporaryDirectory() as tmp:
        write_stats(tmp, hp)
        model = FastSpeech2(R.make_cfg(hp, processed_dir=tmp))
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    model.eval()
    with torch.no_grad():
        out = model({"texts": texts, "text_len": lens, "spk_id": spk}, *controls)
    return out, keys


def main(amphion_root):
    FastSpeech2, jets_module, n_vocab = import_reference(amphion_root)
    assert n_vocab == R.small_hp()["n_vocab"], n_vocab
    for seed in range(48):
        store, keys, report = {"seed": np.int64(seed)}, {}, {}
        for name, (over, text_len, controls) in RUNS.items():
            hp = R.small_hp(**over)
            sd = R.synth_state_dict(hp, seed)
            texts, lens, spk = R.make_inputs(text_len, hp["n_vocab"], seed, hp["n_speaker"])
            ok, tau, d_gap, b_gap, o64, o32 = R.decided(hp, sd, texts, lens, spk, controls)
            if not ok:
                print(f"seed {seed}: run {name} is not decided (gaps {d_gap:.1f} / {b_gap:.1f} tau)")
                break
            out, k = real_run(FastSpeech2, hp, sd, texts, lens, spk, controls)
            if not (torch.equal(out["d_rounded"], o32["d_rounded"]) and torch.equal(out["mel_lens"], o32["mel_lens"])
                    and torch.equal(torch.bucketize(out["p_predictions"], sd["variance_adaptor.pitch_bins"]), o32["p_index"])
                    and torch.equal(torch.bucketize(out["e_predictions"], sd["variance_adaptor.energy_bins"]), o32["e_index"])):
                print(f"seed {seed}: run {name}: the fp32 restatement does not reproduce the real class's decisions")
                break
            keys[name if name == "multi_speaker" else "base"] = k
            store[name + "/texts"], store[name + "/text_len"], store[name + "/spk_id"] = texts.numpy(), lens.numpy(), spk.numpy()
            store[name + "/controls"] = np.asarray(controls, dtype=np.float64)
            for key in STORED:
                v = out[key].numpy()
                store[f"{name}/{key}"] = v.astype(np.float32) if v.dtype == np.float64 else v
            report[name] = dict(tau=tau, duration_gap_tau=d_gap, bin_gap_tau=b_gap, mel_lens=out["mel_lens"].tolist(),
                                d_max=float(out["d_rounded"].max()))
            store[name + "/tau_gaps"] = np.asarray([tau, d_gap, b_gap])
            err = max(float((out[k2].double() - o64[k2]).abs().max()) for k2 in ("output", "postnet_output"))
            print(f"seed {seed} {name}: tau {tau:.2e}, gaps {d_gap:.1f} / {b_gap:.1f} tau, mel_lens {out['mel_lens'].tolist()}, "
                  f"d_rounded max {float(out['d_rounded'].max())}, real class vs fp64 restatement {err:.2e}")
        else:
            hp = R.small_hp()
            sd = R.jets_state_dict(hp, seed)
            texts, lens, spk = R.make_inputs(RUNS["ragged"][1], hp["n_vocab"], seed)
            ok, tau, gap, o64, o32 = R.jets_decided(hp, sd, texts, lens)
            wav, d, jets_keys = real_jets(jets_module, hp, sd, texts, lens, spk)
            if not ok or not torch.equal(d, o32["d_predictions"]):
                print(f"seed {seed}: the JETS run is not decided or not reproduced (gap {gap:.1f} tau)")
                continue
            print(f"seed {seed} jets: tau {tau:.2e}, gap {gap:.1f} tau, d {d.tolist()}, wav {tuple(wav.shape)}, real class vs fp64 restatement "
                  f"{float((wav.double() - o64['wav']).abs().max()):.2e}")
            store["jets/texts"], store["jets/text_len"], store["jets/spk_id"] = texts.numpy(), lens.numpy(), spk.numpy()
            store["jets/wav"], store["jets/d_predictions"], store["jets/tau_gap"] = wav.numpy(), d.numpy(), np.asarray([tau, gap])
            with open(os.path.join(HERE, "keys_jets.json"), "w") as f:
                json.dump(jets_keys, f, indent=0, sort_keys=True)
            np.savez_compressed(os.path.join(HERE, "golden_fs2.npz"), **store)
            with open(os.path.join(HERE, "keys_fs2.json"), "w") as f:
                json.dump(keys, f, indent=0, sort_keys=True)
            print(json.dumps(report, indent=1))
            return
    raise SystemExit("no seed among the first 48 decides every run: widen the duration head's spread (fs2_ref.synth_state_dict)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AMPHION_ROOT", ""))
