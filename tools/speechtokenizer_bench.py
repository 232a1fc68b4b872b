#!/usr/bin/env python
"""Times SpeechTokenizer's drop-ins (amphion_amd/models/codec/speechtokenizer) and their two new hot paths on one GPU, in one process,
alternating with what each is compared against.

    python tools/speechtokenizer_bench.py [--rounds 10] [--iters 10] [--json out.json] [--skip-recipe]

(a) The LSTM stack of the public recipe, H = 1024, T = 500 (10 s at 50 frames / s), 2 layers bidirectional (the encoder's) and 2 layers
    unidirectional (the decoder's), B = 1 and 16: SLSTM of this package (amp_lstm_forward: one GEMM per layer + one launch per time step) against
    the reference's SLSTM.forward on torch.nn.LSTM (MIOpen through PyTorch-ROCm, permutes and skip included), same weights.  The two routes run
    in alternation for --rounds rounds; medians with [min, max].  The recurrence alone (amp_lstm_recur on a prepared Gx) gives us per step.
(b) amp_evq_encode at D = 1024, K = 1024, 8 levels, T = 500 against the reference's own torch ops on the GPU (speechtokenizer_ref.rvq_encode_plain:
    per level the distance, max(-1).indices, the embedding and the subtraction, fp32 -- what ResidualVectorQuantization.encode runs, nothing more).
(c) encode and decode of the recipe for 10 s at 16 kHz, B = 1 and 16, against the fp32 torch restatement of tests/speechtokenizer_ref.py on the
    same GPU with its LSTMs on torch.nn.LSTM; launches counted from the launch manifest of a child process (--manifest-pass; the manifest is
    off while timing) and the LSTMs' share of the time.  Synthetic weights."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import speechtokenizer_ref as R  # noqa: E402
from amphion_amd import _lib  # noqa: E402
from amphion_amd.models.codec.speechtokenizer import SpeechTokenizer  # noqa: E402
from amphion_amd.models.codec.speechtokenizer.modules import SLSTM  # noqa: E402
from amphion_amd.models.codec.speechtokenizer.modules.quantization import ResidualVectorQuantizer  # noqa: E402

SR, SECONDS, FRAMES, HID = 16000, 10, 500, 1024


def _once(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def _alternate(routes, rounds, warmup=2):
    """routes: {name: fn}; every round runs each route once, in turn -> {name: (median, min, max)} in ms"""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            ts[k].append(_once(fn))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def _put(row, name, t):
    row[name + "_ms"] = round(t[0], 3)
    row[name + "_min_max_ms"] = [round(t[1], 3), round(t[2], 3)]


def torch_slstm(lstm, x, bidir):
    """SLSTM.forward of the reference (modules/lstm.py:38-46)"""
    x = x.permute(2, 0, 1)
    y, _ = lstm(x)
    if bidir:
        x = x.repeat(1, 1, 2)
    return (y + x).permute(1, 2, 0)


def bench_lstm(rounds, res):
    dev = torch.device("cuda", torch.cuda.current_device())
    for bidir in (True, False):
        torch.manual_seed(3)
        m = SLSTM(HID, num_layers=2, bidirectional=bidir).cuda().eval()
        h = m._handle(dev)
        ndir = 2 if bidir else 1
        for B in (1, 16):
            x = torch.randn(B, HID, FRAMES, device="cuda")
            y, yt = m.run(x), torch_slstm(m.lstm, x, bidir)
            err = float((y - yt).abs().max())
            gx = torch.randn(B, ndir * 4 * HID, FRAMES, device="cuda")
            out = torch.empty(B, ndir * HID, FRAMES, device="cuda")
            ws = torch.empty(_lib.lib().amp_lstm_workspace_bytes(h, B, FRAMES) // 4, device="cuda")

            def recur():
                _lib.check(_lib.lib().amp_lstm_recur(h, 0, _lib.ptr(gx), B, FRAMES, None, _lib.ptr(out), _lib.ptr(ws), _lib.current_stream_ptr(dev)))

            t = _alternate({"hip": lambda: m.run(x), "torch": lambda: torch_slstm(m.lstm, x, bidir), "recur": recur}, rounds)
            row = dict(H=HID, layers=2, bidirectional=bidir, B=B, T=FRAMES, rounds=rounds, launches=2 * (1 + FRAMES), max_abs_diff_vs_torch=err)
            _put(row, "hip", t["hip"])
            _put(row, "torch_nn_lstm", t["torch"])
            _put(row, "recur_one_layer", t["recur"])
            row["us_per_step"] = round(t["recur"][0] / FRAMES * 1e3, 2)
            row["weight_mb_per_step"] = round(ndir * 4 * HID * HID * 4 / 1e6, 1)
            row["tb_per_s_weights"] = round(ndir * 4 * HID * HID * 4 / 1e12 / (t["recur"][0] / FRAMES / 1e3), 2)
            row["hip_over_torch"] = round(t["hip"][0] / t["torch"][0], 2)
            res["lstm"].append(row)
            print(json.dumps(row), flush=True)


def bench_evq(rounds, res):
    D, K, N = 1024, 1024, 8
    cbs = R.synth_codebooks(D, K, N, 11)
    q = ResidualVectorQuantizer(dimension=D, n_q=N, bins=K)
    for i, c in enumerate(cbs):
        q.vq.layers[i]._codebook.embed.copy_(c)
        q.vq.layers[i]._codebook.inited.fill_(1.0)
    q = q.cuda().eval()
    cb_d = [c.cuda() for c in cbs]

    def ref(z):
        return R.rvq_encode_plain(cb_d, z)

    for B in (1, 16):
        z = torch.randn(B, D, FRAMES, device="cuda")
        same = float((q.encode(z) == ref(z)).double().mean())
        t = _alternate({"hip": lambda: q.encode(z), "torch": lambda: ref(z)}, rounds)
        row = dict(D=D, K=K, N=N, B=B, T=FRAMES, rounds=rounds, launches=1, codes_equal_torch_fp32=round(same, 5))
        _put(row, "hip", t["hip"])
        _put(row, "torch_ops", t["torch"])
        row["hip_over_torch"] = round(t["hip"][0] / t["torch"][0], 2)
        row["tflops_fp32"] = round(2.0 * B * FRAMES * K * D * N / 1e12 / (t["hip"][0] / 1e3), 2)
        res["evq"].append(row)
        print(json.dumps(row), flush=True)


def _recipe():
    hp = R.recipe_hp()
    sd = R.synth_state_dict(hp, 5)
    m = SpeechTokenizer(hp)
    m.load_state_dict(sd)
    return hp, sd, m.cuda().eval()


def _manifest():
    d = tempfile.mkdtemp(prefix="speechtokenizer_bench_")
    counts = {}
    for stage in ("encode", "decode"):
        man = os.path.join(d, stage + ".tsv")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--manifest-pass", stage], env=dict(os.environ, AMP_LAUNCH_MANIFEST=man), check=True,
                       timeout=900)
        with open(man) as f:
            rows = [ln.split("\t")[0] for ln in f if ln.strip()]
        counts[stage] = dict(launches=len(rows), lstm_steps=sum(r.startswith("lstm_step_kernel") for r in rows))
    return counts


def _manifest_stage(stage):
    _, _, m = _recipe()
    with torch.no_grad():
        if stage == "encode":
            m.encode(R.synth_wave(1, SR * SECONDS, 5).cuda())
        else:
            m.decode(torch.zeros(8, 1, FRAMES, dtype=torch.int64, device="cuda"))
        torch.cuda.synchronize()


def bench_recipe(iters, res):
    counts = _manifest()
    hp, sd, m = _recipe()
    sd_d = {k: v.cuda() for k, v in sd.items()}
    # the restatement's LSTMs on torch.nn.LSTM (MIOpen): the torch-ROCm route a user of the reference runs
    lstms = {}
    for kind, p, g in R.encoder_layout(hp) + R.decoder_layout(hp):
        if kind == "lstm":
            mod = torch.nn.LSTM(g["H"], g["H"], g["layers"], bidirectional=g["bidir"])
            mod.load_state_dict({k[len(p) + 5:]: v for k, v in sd.items() if k.startswith(p + "lstm.")})
            lstms[p + "lstm."] = mod.cuda().eval()
    R.slstm = lambda P, p, x, layers, bidir, skip=True: torch_slstm(lstms[p], x, bidir)
    enc_lstm, dec_lstm = m.encoder.model[13], m.decoder.model[1]
    cbs_d = R.codebooks_of(sd_d, hp)
    for B in (1, 16):
        x = R.synth_wave(B, SR * SECONDS, 5).cuda()
        codes = m.encode(x)
        t = _alternate({"hip": lambda: m.encode(x), "torch": lambda: R.rvq_encode_plain(cbs_d, R.encoder_forward(sd_d, hp, x, torch.float32))}, iters, 2)
        xl = torch.randn(B, HID, FRAMES, device="cuda")
        tl = _alternate({"lstm": lambda: enc_lstm.run(xl)}, iters, 2)["lstm"]
        row = dict(stage="encode", B=B, samples=SR * SECONDS, frames=int(codes.shape[2]), rounds=iters, **counts["encode"])
        _put(row, "hip", t["hip"])
        _put(row, "torch_fp32", t["torch"])
        row.update(lstm_ms=round(tl[0], 3), lstm_share=round(tl[0] / t["hip"][0], 3), x_realtime=round(B * SECONDS / t["hip"][0] * 1e3, 1),
                   hip_over_torch=round(t["hip"][0] / t["torch"][0], 2))
        res["recipe"].append(row)
        print(json.dumps(row), flush=True)
        t = _alternate({"hip": lambda: m.decode(codes), "torch": lambda: R.model_decode(sd_d, hp, codes, torch.float32)}, iters, 2)
        tl = _alternate({"lstm": lambda: dec_lstm.run(xl)}, iters, 2)["lstm"]
        row = dict(stage="decode", B=B, frames=int(codes.shape[2]), samples=int(codes.shape[2]) * R.hop(hp), rounds=iters, **counts["decode"])
        _put(row, "hip", t["hip"])
        _put(row, "torch_fp32", t["torch"])
        row.update(lstm_ms=round(tl[0], 3), lstm_share=round(tl[0] / t["hip"][0], 3), x_realtime=round(B * SECONDS / t["hip"][0] * 1e3, 1),
                   hip_over_torch=round(t["hip"][0] / t["torch"][0], 2))
        res["recipe"].append(row)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10, help="rounds of the recipe tables")
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-recipe", action="store_true")
    ap.add_argument("--manifest-pass", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.manifest_pass:
        return _manifest_stage(a.manifest_pass)
    assert not os.environ.get("AMP_LAUNCH_MANIFEST"), "time with the launch manifest off"
    res = {"lstm": [], "evq": [], "recipe": []}
    with torch.no_grad():
        bench_lstm(a.rounds, res)
        bench_evq(a.rounds, res)
        if not a.skip_recipe:
            bench_recipe(a.iters, res)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
