"""FastSpeech2 on the CPU: the restatement (tests/fs2_ref.py) against the runs stored from the real reference class
(tests/golden/make_golden_fs2.py), the package's classes against the real ``state_dict``, the new entry points' surface and their host-side
refusals."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import fs2_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNS = {
    "ragged": dict(),
    "controls": dict(),
    "long": dict(max_seq_len=40),
    "frame_level": dict(pitch_level="frame_level", energy_level="frame_level"),
    "multi_speaker": dict(n_speaker=4),
}
CONT = ("output", "postnet_output", "p_predictions", "e_predictions", "log_d_predictions")
CPU_BOUND = 2e-5


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_fs2.npz"))


def run_inputs(gold, name):
    hp = R.small_hp(**RUNS[name])
    sd = R.synth_state_dict(hp, int(gold["seed"]))
    t = lambda k: torch.from_numpy(gold[f"{name}/{k}"])
    return hp, sd, t("texts"), t("text_len"), t("spk_id"), tuple(float(c) for c in gold[name + "/controls"])


@pytest.mark.parametrize("name", list(RUNS))
def test_restatement_is_the_reference(name, gold):
    """every stored run: decided (each duration and bin decision at least 4 tau from its boundary), the discrete outputs reproduced exactly
    and the continuous ones within the CPU bound"""
    hp, sd, texts, lens, spk, controls = run_inputs(gold, name)
    ok, tau, d_gap, b_gap, o64, o32 = R.decided(hp, sd, texts, lens, spk, controls)
    print(f"{name}: tau {tau:.2e}, smallest gaps {d_gap:.1f} (durations) / {b_gap:.1f} (bins) tau")
    assert ok and d_gap >= 4 and b_gap >= 4
    assert torch.equal(o32["d_rounded"], torch.from_numpy(gold[name + "/d_rounded"]))
    assert torch.equal(o32["mel_lens"], torch.from_numpy(gold[name + "/mel_lens"]))
    assert torch.equal(o32["mel_masks"], torch.from_numpy(gold[name + "/mel_masks"]))
    assert torch.equal(o32["src_masks"], torch.from_numpy(gold[name + "/src_masks"]))
    va = "variance_adaptor."
    for which, key, idx in (("pitch", "p_predictions", "p_index"), ("energy", "e_predictions", "e_index")):
        assert torch.equal(torch.bucketize(torch.from_numpy(gold[f"{name}/{key}"]), sd[va + which + "_bins"]), o32[idx])
    for k in CONT:
        g = torch.from_numpy(gold[f"{name}/{k}"])
        assert o32[k].shape == g.shape
        e = float((o32[k] - g).abs().max())
        assert e <= CPU_BOUND * max(1.0, float(g.abs().max())), (k, e)
    if name == "long":                                    # both on-the-fly position tables ran
        assert texts.shape[1] > hp["max_seq_len"] and int(o32["mel_lens"].max()) > hp["max_seq_len"]
    if name == "ragged":                                  # durations include zeros and a spread of values
        d = o32["d_rounded"][~o32["src_masks"]]
        assert int((d == 0).sum()) > 0 and float(d.max()) >= 3


@pytest.mark.parametrize("which", ["base", "multi_speaker"])
def test_state_dict_keys(which):
    from amphion_amd.models.tts.fastspeech2 import FastSpeech2

    with open(os.path.join(GOLDEN, "keys_fs2.json")) as f:
        keys = json.load(f)[which]
    hp = R.small_hp(**RUNS["multi_speaker" if which == "multi_speaker" else "ragged"])
    m = FastSpeech2(R.make_cfg(hp), stats=R.stats_of(hp), n_speaker=hp["n_speaker"] or None)
    mine = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert mine == keys
    assert list(mine) == list(R.param_shapes(hp)) or set(mine) == set(R.param_shapes(hp))
    m.load_state_dict(R.synth_state_dict(hp, 0))          # strict
    assert torch.equal(m.variance_adaptor.pitch_bins, R.bins_of(hp, "pitch")) and torch.equal(m.encoder.position_enc[0], R.sinusoid_table(hp["max_seq_len"] + 1, hp["hidden"]))


def test_constructor_reads_statistics_files(tmp_path):
    """without ``stats=`` the two statistics.json files are read as the reference reads them"""
    from amphion_amd.models.tts.fastspeech2 import FastSpeech2

    hp = R.small_hp(pitch_quant="log", stats=dict(pitch_min=0.1, pitch_max=6.0, energy_min=-1.5, energy_max=5.0))
    for sub, which in (("phone_pitches", "pitch"), ("phone_energys", "energy")):
        d = tmp_path / "ds" / sub
        d.mkdir(parents=True)
        s = hp["stats"]
        (d / "statistics.json").write_text(json.dumps({"ds_ds": {"voiced_positions": {"mean": 1.0, "std": 2.0}, "total_positions": {
            "min": 1.0 + 2.0 * s[which + "_min"], "max": 1.0 + 2.0 * s[which + "_max"]}}}))
    m = FastSpeech2(R.make_cfg(hp, processed_dir=str(tmp_path)))
    assert torch.allclose(m.variance_adaptor.pitch_bins, R.bins_of(hp, "pitch"), rtol=1e-6, atol=0)
    assert torch.allclose(m.variance_adaptor.energy_bins, R.bins_of(hp, "energy"), rtol=1e-6, atol=1e-7)


def test_not_implemented_cases():
    from amphion_amd.models.tts.fastspeech2 import FastSpeech2

    hp = R.small_hp()
    m = FastSpeech2(R.make_cfg(hp), stats=R.stats_of(hp))
    data = {"texts": torch.ones(1, 4, dtype=torch.long), "text_len": torch.tensor([4]), "spk_id": torch.zeros(1, dtype=torch.long)}
    with pytest.raises(NotImplementedError, match="training"):
        m(data)
    m.eval()
    for k in ("durations", "pitch", "energy", "target_len"):
        with pytest.raises(NotImplementedError, match=k):
            m(dict(data, **{k: torch.zeros(1, 4)}))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(data)


def test_abi_surface_and_host_refusals():
    """the symbols are exported, bound and declared, the version says so, and every refusal is made on the host before anything is launched:
    the pointers below are host buffers that are never read"""
    from amphion_amd import _lib

    L = _lib.lib()
    assert L.amp_version() >= 156
    names = ("amp_mh_attention", "amp_fs2_durations", "amp_bucketize_embed_add", "amp_layer_norm_c_head")
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "amphion_hip.h")) as f:
        header = f.read()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and f" {n}(" in header, n
    INV, UNS = _lib.AMP_ERR_INVALID, _lib.AMP_ERR_UNSUPPORTED
    buf, other = (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)()
    ints = (ctypes.c_int * 64)()
    msg = lambda: L.amp_last_error().decode()
    # amp_mh_attention: dk, sizes, stride, scale, overlap, NULL
    assert L.amp_mh_attention(buf, buf, buf, 0, None, 1, 2, 64, 4, 0.1, other, None) == INV and "128" in msg()
    assert L.amp_mh_attention(buf, buf, buf, 0, None, 1, 2, 96, 4, 0.1, other, None) == INV
    assert L.amp_mh_attention(None, buf, buf, 0, None, 1, 2, 128, 4, 0.1, other, None) == INV
    assert L.amp_mh_attention(buf, buf, buf, 0, None, 0, 2, 128, 4, 0.1, other, None) == INV
    assert L.amp_mh_attention(buf, buf, buf, 0, None, 1, 2, 128, 40000, 0.1, other, None) == INV
    assert L.amp_mh_attention(buf, buf, buf, 0, None, 40000, 2, 128, 4, 0.1, other, None) == INV
    assert L.amp_mh_attention(buf, buf, buf, 100, None, 1, 2, 128, 4, 0.1, other, None) == INV and "stride" in msg()
    assert L.amp_mh_attention(buf, buf, buf, 0, None, 1, 2, 128, 4, 0.0, other, None) == INV
    assert L.amp_mh_attention(buf, buf, buf, 0, None, 1, 2, 128, 4, 0.1, buf, None) == INV and "overlap" in msg()
    assert L.amp_rope_attention(buf, buf, buf, 0, buf, buf, None, 1, 2, 128, 4, 0.1, other, None) == INV      # dk 128 stays refused there
    # amp_fs2_durations
    assert L.amp_fs2_durations(None, 1, 4, 1.0, other, ints, ints, None) == INV
    assert L.amp_fs2_durations(buf, 0, 4, 1.0, other, ints, ints, None) == INV
    assert L.amp_fs2_durations(buf, 1, 4, 0.0, other, ints, ints, None) == INV and "d_control" in msg()
    assert L.amp_fs2_durations(buf, 1, 4, float("nan"), other, ints, ints, None) == INV
    assert L.amp_fs2_durations(buf, 1, 4, 1.0, buf, ints, ints, None) == INV
    # amp_bucketize_embed_add
    assert L.amp_bucketize_embed_add(buf, 1.0, buf, 3, buf, 3, buf, 1, 4, 4, other, other, None) == INV and "rows" in msg()
    assert L.amp_bucketize_embed_add(buf, 1.0, buf, 0, buf, 3, buf, 1, 4, 4, other, other, None) == INV
    assert L.amp_bucketize_embed_add(buf, float("nan"), buf, 3, buf, 4, buf, 1, 4, 4, other, other, None) == INV
    assert L.amp_bucketize_embed_add(buf, 1.0, buf, 3, buf, 4, buf, 1, 4, 4, other, buf, None) == INV
    assert L.amp_bucketize_embed_add(buf, 1.0, buf, 3, None, 4, buf, 1, 4, 4, other, other, None) == INV
    assert L.amp_bucketize_embed_add(buf, 1.0, buf, 3, buf, 4, buf, 70000, 4, 4, other, other, None) == UNS
    # amp_layer_norm_c_head
    assert L.amp_layer_norm_c_head(buf, buf, buf, None, 0.0, None, 1, 4, 4, 1e-5, other, None) == INV
    assert L.amp_layer_norm_c_head(buf, buf, buf, buf, 0.0, None, 1, 0, 4, 1e-5, other, None) == INV
    assert L.amp_layer_norm_c_head(buf, buf, buf, buf, 0.0, None, 1, 4, 4, -1.0, other, None) == INV
    assert L.amp_layer_norm_c_head(buf, buf, buf, buf, 0.0, None, 70000, 4, 4, 1e-5, other, None) == INV


# ---- JETS -----------------------------------------------------------------------------------------------------------------------------------
def test_jets_restatement_is_the_reference(gold):
    """Jets.inference of the real class on the ragged batch: durations decided and reproduced, the wave within the CPU bound"""
    hp = R.small_hp()
    sd = R.jets_state_dict(hp, int(gold["seed"]))
    texts, lens = torch.from_numpy(gold["jets/texts"]), torch.from_numpy(gold["jets/text_len"])
    ok, tau, gap, o64, o32 = R.jets_decided(hp, sd, texts, lens)
    print(f"jets: tau {tau:.2e}, smallest duration gap {gap:.1f} tau")
    assert ok and gap >= 4
    assert torch.equal(o32["d_predictions"], torch.from_numpy(gold["jets/d_predictions"]))
    wav = torch.from_numpy(gold["jets/wav"])
    assert o32["wav"].shape == wav.shape and float((o32["wav"] - wav).abs().max()) <= CPU_BOUND
    assert int((o32["d_predictions"][~R.pad_mask(lens)] == 0).sum()) > 0


def test_jets_state_dict_keys_and_refusals():
    from amphion_amd.models.tts.jets import Jets

    with open(os.path.join(GOLDEN, "keys_jets.json")) as f:
        keys = json.load(f)
    hp = R.small_hp()
    m = Jets(R.make_cfg(hp), stats=R.stats_of(hp))
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == keys
    m.load_state_dict(R.jets_state_dict(hp, 0))           # strict
    data = {"texts": torch.ones(1, 4, dtype=torch.long), "text_len": torch.tensor([4]), "spk_id": torch.zeros(1, dtype=torch.long)}
    with pytest.raises(NotImplementedError, match="training path"):
        m(data)
    with pytest.raises(NotImplementedError, match="training mode"):
        m.inference(data)
    m.eval()
    with pytest.raises(NotImplementedError, match="durations"):
        m.inference(dict(data, durations=torch.ones(1, 4)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.inference(data)
