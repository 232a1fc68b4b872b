"""Times FastSpeech2 text -> mel on one GPU at the recipe sizes (config/fs2.json: hidden 256 in 2 heads of 128, 4 + 6 layers, filter 1024,
k = (9, 1), predictors 256 x k 3, 256 bins, 80 mel bands) with synthetic weights at 1 / sqrt(fan_in), against torch fp32 ops on the same GPU
(DESIGN.md §23):

    python tools/bench_fs2.py [--rounds 3] [--phones 100] [--frames-per-phone 8]

  attention      amp_mh_attention at T in {100, 800}, B in {1, 16} against fp32 scaled_dot_product_attention on the same strided q | k | v
  fft block      one FFT block at the same shapes against the restatement of tests/fs2_ref.py on the device
  text -> mel    the whole model for 100 phones of 8 frames each (durations handed to both sides, so both expand to the same 800 frames) at
                 B = 1 and B = 16 against the restatement on the device
  text -> wave   Jets.inference for the same 100 phones (the duration head set to predict 8 frames everywhere: weight 0, bias log 9) against
                 the restatement with torch's HiFi-GAN ops on the device

Each figure is the median over ``rounds`` of (device events around ``iters`` back-to-back calls) / iters, the two sides alternating round by
round after a warm-up of both -- tools/bench_ar.py's method.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fs2_ref as R  # noqa: E402
from amphion_amd.models.tts.fastspeech2 import FastSpeech2  # noqa: E402
from amphion_amd.models.tts.jets import Jets  # noqa: E402
from amphion_amd.modules import hip_ops  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters                  # ms per call


def compare(fns, iters, rounds, warm=2):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, iters))
    out = {k: round(statistics.median(v), 5) for k, v in t.items()}
    out["spread"] = {k: round(max(v) - min(v), 5) for k, v in t.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--phones", type=int, default=100)
    ap.add_argument("--frames-per-phone", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hp = R.small_hp(enc_layers=4, dec_layers=6, d_inner=1024, n_mel=80, max_seq_len=1000)
    sd = R.synth_state_dict(hp, 0)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    model = FastSpeech2(R.make_cfg(hp), stats=R.stats_of(hp), n_src_vocab=hp["n_vocab"])
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    H, C = hp["heads"], hp["hidden"]
    jsd = R.jets_state_dict(hp, 0)
    jsd["variance_adaptor.duration_predictor.linear_layer.weight"].zero_()
    jsd["variance_adaptor.duration_predictor.linear_layer.bias"].fill_(float(torch.log(torch.tensor(1.0 + args.frames_per_phone))))
    jsd_dev = {k: v.to(dev) for k, v in jsd.items()}
    jets = Jets(R.make_cfg(hp), stats=R.stats_of(hp), n_src_vocab=hp["n_vocab"])
    jets.load_state_dict(jsd)
    jets = jets.to(dev).eval()
    res = {"attention_ms": {}, "fft_block_ms": {}, "text_to_mel_ms": {}, "text_to_wave_ms": {}}
    with torch.no_grad():
        for Bn in (1, 16):
            for T in (args.phones, args.phones * args.frames_per_phone):
                qkv = torch.randn(Bn, 3 * C, T, device=dev)
                q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
                sdpa = lambda: F.scaled_dot_product_attention(*(t.reshape(Bn, H, C // H, T).transpose(2, 3) for t in (q, k, v)))
                res["attention_ms"][f"B{Bn}_T{T}"] = compare({"hip": lambda: hip_ops.mh_attention(q, k, v, H), "torch_sdpa": sdpa}, 50, args.rounds)
                x = torch.randn(Bn, T, C, device=dev)
                pad = torch.zeros(Bn, T, dtype=torch.bool, device=dev)
                block = model.decoder.layer_stack[0]
                res["fft_block_ms"][f"B{Bn}_T{T}"] = compare({
                    "hip": lambda: block(x, mask=pad, slf_attn_mask=None),
                    "torch": lambda: R.fft_block(sd_dev, "decoder.layer_stack.0", x, pad, H)}, 20, args.rounds)
            texts = torch.randint(1, hp["n_vocab"], (Bn, args.phones), device=dev)
            lens = torch.full((Bn,), args.phones, dtype=torch.long, device=dev)
            dur = torch.full((Bn, args.phones), float(args.frames_per_phone), device=dev)
            data = {"texts": texts, "text_len": lens, "spk_id": torch.zeros(Bn, dtype=torch.long, device=dev)}
            res["text_to_mel_ms"][f"B{Bn}"] = compare({
                "hip": lambda: model(data, durations=dur),
                "torch": lambda: R.fs2_forward(sd_dev, hp, texts, lens, None, durations=dur)}, 3, args.rounds, warm=1)
            res["text_to_wave_ms"][f"B{Bn}"] = compare({
                "hip": lambda: jets.inference(data),
                "torch": lambda: R.jets_inference(jsd_dev, hp, texts, lens)}, 2, args.rounds, warm=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
