"""Writes tests/golden/golden_ns2.npz and keys_ns2.json from the REAL NaturalSpeech2 of an Amphion checkout, on the CPU:

    python tests/golden/make_golden_ns2.py <amphion root>

The ``encodec`` package is replaced by a stand-in written here: ``EncodecModel.encodec_model_24khz()`` returns an object with
``set_target_bandwidth``, ``requires_grad_`` and a ``.quantizer`` module whose buffers carry the package's names
(``vq.layers.{i}._codebook.{inited,cluster_size,embed,embed_avg}``) and whose ``decode(codes [n_q, B, T])`` is the sum of the look-ups,
transposed to [B, D, T].  Small model: tests/ns2_ref.py ``small_hp``.  Runs: ``euler`` 4 steps with B = 2, equal phone counts (11) and ragged
prompts (37 and 23 frames); ``midpoint`` 3 steps, B = 1; ``flow`` 4 steps, B = 1.

The npz holds inputs, the drawn noise, outputs and the seed only: the weights regenerate from the seed (ns2_ref.synth_state_dict).  The noise
is what the class draws: eval mode draws nothing but ``torch.randn(B, latent, T)``, so re-seeding and drawing the same shape repeats it.
Durations and pitch tokens are discrete decisions, so the script keeps the first seed under which EVERY run is decided: each rounded duration
and each pitch bin of the fp64 restatement at least 4 tau from its boundary (tau: the fp32 restatement's distance from fp64 on the quantity
the decision reads) and the fp32 restatement reproducing the real class's dur_pred_round, mel_len and pitch_token exactly.  tau and the
smallest gaps are printed and stored per run."""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ns2_ref as R  # noqa: E402

RUNS = {
    "euler": (dict(), 11, [37, 23], 4),
    "midpoint": (dict(solver="midpoint"), 11, [29], 3),
    "flow": (dict(diffusion_type="flow"), 11, [29], 4),
}
STORED = ("dur_pred_round", "dur_pred_log", "dur_pred", "pitch_pred_log", "pitch_token", "mel_len", "prior_out")
_SIZE = {}


class _Codebook(nn.Module):
    def __init__(self, K, D):
        super().__init__()
        self.register_buffer("inited", torch.zeros(1))
        self.register_buffer("cluster_size", torch.zeros(K))
        self.register_buffer("embed", torch.zeros(K, D))
        self.register_buffer("embed_avg", torch.zeros(K, D))


class _Layer(nn.Module):
    def __init__(self, K, D):
        super().__init__()
        self._codebook = _Codebook(K, D)


class _Rvq(nn.Module):
    def __init__(self, n_q, K, D):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(K, D) for _ in range(n_q)])


class _Quantizer(nn.Module):
    def __init__(self, n_q, K, D):
        super().__init__()
        self.vq = _Rvq(n_q, K, D)

    def decode(self, codes):
        out = 0.0
        for i in range(codes.shape[0]):
            out = out + nn.functional.embedding(codes[i], self.vq.layers[i]._codebook.embed)
        return out.transpose(1, 2)


class _Codec(nn.Module):
    def __init__(self):
        super().__init__()
        self.quantizer = _Quantizer(_SIZE["n_q"], _SIZE["codebook_size"], _SIZE["latent"])

    def set_target_bandwidth(self, bw):
        pass


class EncodecModel:
    @staticmethod
    def encodec_model_24khz():
        return _Codec()


def import_reference(amphion_root):
    stand_in = types.ModuleType("encodec")
    stand_in.EncodecModel = EncodecModel
    sys.modules["encodec"] = stand_in
    sys.path.insert(0, amphion_root)
    from models.tts.naturalspeech2.ns2 import NaturalSpeech2

    return NaturalSpeech2


def real_run(NaturalSpeech2, hp, sd, codes, phone, mask, n_steps, draw_seed):
    _SIZE.update(n_q=hp["n_q"], codebook_size=hp["codebook_size"], latent=hp["latent"])
    model = NaturalSpeech2(R.make_cfg(hp))
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(sd, strict=True)
    model.eval()
    torch.manual_seed(draw_seed)
    with torch.no_grad():
        x0, po = model.inference(ref_code=codes.transpose(0, 1), phone_id=phone, ref_mask=mask, inference_steps=n_steps)
    torch.manual_seed(draw_seed)
    z = torch.randn(x0.shape[0], hp["latent"], x0.shape[2])
    return x0, po, z, keys


def main():
    NaturalSpeech2 = import_reference(sys.argv[1])
    for seed in range(64):
        store, report, keys = {"seed": np.int64(seed)}, {}, None
        for ri, (name, (over, n_phones, ref_lens, n_steps)) in enumerate(RUNS.items()):
            hp = R.small_hp(**over)
            sd = R.synth_state_dict(hp, seed)
            phone, codes, mask = R.make_inputs(hp, seed + ri, n_phones, ref_lens)
            ok, tau, d_gap, p_gap, p64, p32 = R.decided(sd, hp, codes, phone, mask, None, 0)
            if not ok or int(p64["mel_len"].min()) < 1:
                print(f"seed {seed}: run {name} is not decided (gaps {d_gap:.1f} / {p_gap:.1f} tau, mel_len {p64['mel_len'].tolist()})")
                break
            x0, po, z, k = real_run(NaturalSpeech2, hp, sd, codes, phone, mask, n_steps, 7000 + seed + ri)
            if name == "euler":
                keys = k
            if not all(torch.equal(po[q].cpu(), p32[q]) for q in ("dur_pred_round", "mel_len", "pitch_token")):
                print(f"seed {seed}: the fp32 restatement does not reproduce the real class's decisions in run {name}")
                break
            x64, _ = R.inference(R.cast(sd, torch.float64), hp, codes, phone, mask, z.double(), n_steps)
            x32, _ = R.inference(sd, hp, codes, phone, mask, z, n_steps)
            store[f"{name}/phone_id"], store[f"{name}/ref_code"], store[f"{name}/ref_mask"] = phone.numpy(), codes.transpose(0, 1).numpy(), mask.numpy()
            store[f"{name}/z"], store[f"{name}/x0"] = z.numpy(), x0.numpy()
            for q in STORED:
                store[f"{name}/{q}"] = po[q].numpy()
            store[f"{name}/tau_gaps"] = np.asarray([tau[0], tau[1], d_gap, p_gap])
            report[name] = dict(tau=tau, duration_gap_tau=d_gap, pitch_gap_tau=p_gap, mel_len=po["mel_len"].tolist(), d_max=int(po["dur_pred_round"].max()))
            print(f"seed {seed} {name}: tau {tau[0]:.2e} / {tau[1]:.2e}, gaps {d_gap:.1f} / {p_gap:.1f} tau, mel_len {po['mel_len'].tolist()}, durations up to "
                  f"{int(po['dur_pred_round'].max())}, x0 |max| {float(x0.abs().max()):.3f}; real class vs fp64 restatement {float((x0.double() - x64).abs().max()):.2e}, "
                  f"fp32 restatement vs fp64 {float((x32.double() - x64).abs().max()):.2e}")
        else:
            np.savez_compressed(os.path.join(HERE, "golden_ns2.npz"), **store)
            with open(os.path.join(HERE, "keys_ns2.json"), "w") as f:
                json.dump(keys, f, indent=0, sort_keys=True)
            print(json.dumps(report, indent=1))
            print("kept seed", seed, "->", os.path.getsize(os.path.join(HERE, "golden_ns2.npz")), "bytes")
            return
    raise SystemExit("no seed decides every run")


if __name__ == "__main__":
    main()
