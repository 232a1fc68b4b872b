"""CPU: (1) the tokenizer geometry tables (tests/tokenizer_geometry.py) reach every path of csrc/evq.hip, csrc/lstm.hip, csrc/dsconv_f16x3.hip and
csrc/seanet.hip they are meant to -- padded codebook rows of every D % 4, K below 4 / of 1 / beyond four passes / 4095 and 4096, N = 32; both of
the LSTM's lane loops at their second pass and at depth, H < 4, every batch tile full / with a tail / three times, the 64-KB LDS request; one to
five K steps of the down-sampling conv with ragged last steps and both tiles -- and no device tensor of the sweep passes 1 MiB; (2) the fp64
reference alone decides (speechtokenizer_ref.margin_rule) at least 98 % of the frames of every quantizer case at every length; (3) numpy fp32
models of evq_encode_kernel and lstm_step_kernel pass the rules the GPU tests apply, while one-slip mutants of them are each caught by those
rules on rows of these tables; (4) the even / odd plane indexing of the down-sampling conv is Conv1d(k = 3, stride 2, padding 1) at every
table length, and a clamp in place of the zero select is caught."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import speechtokenizer_ref as R  # noqa: E402
import tokenizer_geometry as tg  # noqa: E402

MODEL_WORK_CAP = 300_000                         # K x DP above which the evq model runs at T = 1 and 17 only (the 16-MiB codebook)


# ------------------------------------------------------------------------------------------------------------------------------
# the tables hold what they are meant to
# ------------------------------------------------------------------------------------------------------------------------------
def test_evq_table_reaches_every_class():
    cases = tg.EVQ
    assert len({c.id for c in cases + tg.EVQ_TIES}) == len(cases) + len(tg.EVQ_TIES)
    for c in cases + tg.EVQ_TIES + [tg.EVQ_FLAG]:
        assert 1 <= c.D <= 1024 and 1 <= c.K <= 4096 and 1 <= c.N <= 32, c.id
        # all_zq, the largest tensor of a case, with its sentinels
        assert c.N * tg.B * c.D * max(c.Ts) * 4 + 1024 <= tg.DEVICE_TENSOR_CAP, c.id
    assert {c.D % 4 for c in cases if c.D > 4} == {0, 1, 2, 3} and {c.D for c in cases if c.D < 4} == {1, 3}
    assert any(c.D == 1024 for c in cases) and any(c.D == 1023 for c in cases) and any(c.D == 1022 for c in cases)
    assert {1, 3}.issubset({c.K for c in cases}) and any(c.K == 1 and c.N > 1 for c in cases)
    assert any(c.K < 4 and c.padded for c in cases) and any(4 < c.K < 256 and c.K % 4 for c in cases)
    assert any(256 < c.K < 512 and c.K % 4 for c in cases) and any(c.K == 260 for c in cases)          # a second pass of one and of four rows
    assert any(1024 < c.K for c in cases) and {4095, 4096}.issubset({c.K for c in cases})
    assert sum(c.N == 32 for c in cases) == 2 and all(not c.decay for c in cases if c.N == 32) and any(c.N == 1 for c in cases)
    assert any(c.padded and c.K > 256 for c in cases)
    for c in cases:
        assert 1 in c.Ts and tg.EVQ_TF in c.Ts and tg.EVQ_TF + 1 in c.Ts and any(T > 2 * tg.EVQ_TF and T % tg.EVQ_TF for T in c.Ts), c.id
    # the lengths were shortened only where T = 50 would pass the cap
    for c in cases:
        over = c.N * tg.B * c.D * 50 * 4 + 1024 > tg.DEVICE_TENSOR_CAP
        assert (c.Ts == tg.EVQ_SHORT) == over and (c.Ts == tg.EVQ_LENGTHS) == (not over), c.id
    # ties: a row and its copy in one thread (one pass, and passes apart), in two threads of a wave, in two waves
    rel = {c.id: tg.evq_tie_relation(c) for c in tg.EVQ_TIES}
    assert all(c.K % 2 == 0 for c in tg.EVQ_TIES)
    assert rel["D5K4N2"] == {"thread"} and rel["D5K1024N1"] == {"thread"} and rel["D5K256N1"] == {"waves"} and rel["D130K64N2"] == {"wave"}
    assert "wave" in rel["D5K10N2"] and "wave" in rel["D6K520N2"]
    assert any(c.padded for c in tg.EVQ_TIES) and any(c.K > 256 for c in tg.EVQ_TIES)
    assert tg.EVQ_FLAG.padded and (tg.EVQ_FLAG.D + 255) // 256 == 4


def test_lstm_table_reaches_every_class():
    Hs = tg.LSTM_H
    assert {1, 2, 3}.issubset(Hs)                                                            # inactive waves in the only workgroup
    assert {63, 64, 65}.issubset(Hs) and {252, 256, 260}.issubset(Hs) and 1023 in Hs and 257 in Hs
    for Hn in (63, 65, 257, 1023):
        assert Hn % 4                                                                        # the scalar path
    assert [(Hn // 4 + 63) // 64 for Hn in (252, 256, 260)] == [1, 1, 2]                     # the 16-byte lane loop's second pass begins at H / 4 = 65
    assert [(Hn + 63) // 64 for Hn in (63, 65, 1023)] == [1, 2, 16]
    assert max(tg.LSTM_H_T) >= 3 and 1 in tg.LSTM_H_T                                        # both state buffers are read
    tiles = {(tg.lstm_tile(b), b % tg.lstm_tile(b) == 0, -(-b // tg.lstm_tile(b))) for b in tg.LSTM_B}
    for BT in (4, 8, 16):
        assert (BT, True, 1) in tiles and (BT, False, 1) in tiles, BT
    assert (1, True, 1) in tiles and (16, False, 2) in tiles and (16, False, 3) in tiles
    assert any(Hn % 4 for Hn in tg.LSTM_B_H) and any(Hn % 4 == 0 for Hn in tg.LSTM_B_H)
    Hn, Bn, T = tg.LSTM_64KB
    assert tg.lstm_lds_bytes(Hn, Bn) == 64 * 1024 and Bn % 16 and T >= 2
    assert (3 * 2 * Bn * Hn + Bn * 2 * 4 * Hn * T) * 4 + 1024 <= tg.DEVICE_TENSOR_CAP         # the workspace: state + gx
    assert (3 * 2 * Bn * Hn + Bn * 2 * 4 * Hn * (T + 1)) * 4 > tg.DEVICE_TENSOR_CAP           # (one more step would pass it)
    assert all(tg.lstm_lds_bytes(h, b) < 64 * 1024 for h in tg.LSTM_H for b in (tg.B,))
    assert {T % 2 for _, T in tg.LSTM_LONG} == {1} and {h % 4 == 0 for h, _ in tg.LSTM_LONG} == {True, False}
    assert {h % 4 == 0 for h in tg.LSTM_FLIP_H} == {True, False}
    fw = tg.LSTM_FORWARD
    assert any(In != Hn and In > Hn for In, Hn, *_ in fw) and any(In < Hn for In, Hn, *_ in fw) and any(In == 2048 for In, *_ in fw)
    assert {L for _, _, L, _, _ in fw} == {1, 2, 3, 4} and {(L, bd) for _, _, L, bd, sk in fw if sk} == {(L, bd) for L in (3, 4) for bd in (False, True)}
    assert all(In == Hn for In, Hn, _, _, sk in fw if sk)
    assert any(Hn == 1024 and L == 1 for _, Hn, L, _, _ in tg.LSTM_CREATE_EDGES) and any(L == 4 for _, _, L, _, _ in tg.LSTM_CREATE_EDGES)
    # the largest device tensors: gx of the H axis and the workspace of a forward case
    assert tg.B * 2 * 4 * max(Hs) * max(tg.LSTM_H_T) * 4 + 1024 <= tg.DEVICE_TENSOR_CAP
    for In, Hn, L, bd, _ in fw:
        nd = 2 if bd else 1
        assert (3 * nd * tg.B * Hn + 64 + tg.B * nd * 5 * Hn * max(tg.LSTM_FORWARD_T)) * 4 + 1024 <= tg.DEVICE_TENSOR_CAP
        assert tg.B * max(In, nd * Hn) * max(tg.LSTM_FORWARD_T) * 4 <= tg.DEVICE_TENSOR_CAP


def test_dsconv_and_elementwise_tables():
    cases = tg.DSCONV
    assert {c.steps for c in cases} == {1, 2, 3, 4, 5}
    assert any(c.steps == 3 and c.cin % tg.DS_KC == 1 for c in cases) and any(c.steps >= 4 and c.cin % tg.DS_KC for c in cases)
    big = [c for c in cases if any(c.big(T) for T in c.Ts)]
    assert len(big) == 1 and all(big[0].big(T) for T in big[0].Ts) and big[0].steps == 4 and big[0].cout % 128
    assert big[0].B * 1 * ((big[0].cout + 127) // 128) == 256
    assert not any(c.big(T, 1) for c in cases for T in c.Ts)                                 # the B = 1 runs take the small tile
    assert any(c.cout % 64 and c.cout < 64 for c in cases) and any(c.cin == 1 and c.cout == 1 for c in cases)
    touts = {(T - 1) // 2 + 1 for c in cases for T in c.Ts}
    assert {1, 64, 65, 128, 129}.issubset(touts)
    for c in cases + [tg.DS_RANGE]:
        for T in c.Ts:
            assert c.B * max(c.cin * T, c.cout * ((T - 1) // 2 + 1)) * 4 + 1024 <= tg.DEVICE_TENSOR_CAP, c.id
    assert tg.DS_RANGE.steps == 3 and tg.DS_RANGE.cin % tg.DS_KC == 1 and tg.DS_RANGE.B >= 3
    # elu_pad: one-sided pads both ways, pads above 10, T on both sides of max_pad
    assert any(pl == 0 and pr for pl, pr in tg.ELU_PADS) and any(pr == 0 and pl for pl, pr in tg.ELU_PADS) and any(max(p) > 10 for p in tg.ELU_PADS)
    for pl, pr in tg.ELU_PADS:
        Ts, m = tg.elu_lengths(pl, pr), max(pl, pr)
        assert {m, m + 1}.issubset(Ts) and 1 in Ts
        assert tg.ELU_B * max(tg.ELU_C) * (max(Ts) + pl + pr) * 4 <= tg.DEVICE_TENSOR_CAP
    assert {n >> 2 for n in tg.GELU_N if n < 8} == {0, 1} and {n & 3 for n in tg.GELU_N} == {0, 1, 2, 3}
    sv = tg.special_values()
    assert bool(torch.isnan(sv).any()) and bool(torch.isinf(sv).sum() == 2) and bool(((sv != 0) & (sv.abs() < 1.2e-38)).sum() == 2)
    assert bool((sv == 0).any()) and bool(torch.signbit(sv[sv == 0]).all())


# ------------------------------------------------------------------------------------------------------------------------------
# the fp64 reference decides the quantizer cases; the model of the kernel passes the rules
# ------------------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy()


def _model(ref, mutant=None):
    return tg.evq_model([_np(c) for c in ref["cbs"]], _np(ref["z"]), ref["st"], ref["n_q"], mutant)


def _model_lengths(case):
    return case.Ts if case.K * case.DP <= MODEL_WORK_CAP else (1, 17)


@pytest.mark.parametrize("case", tg.EVQ, ids=lambda c: c.id)
def test_fp64_decides_and_the_evq_model_agrees(case):
    for T in case.Ts:
        ref = tg.evq_reference(case, T)
        print(f"{case.id} T={T}: tau {ref['tau']:.3e}, smallest fp64 margin {float(ref['r64']['margin'].min()):.3e}, undecided {ref['undecided']:.4f}")
        assert ref["undecided"] <= tg.UNDECIDED_CAP, "the fp64 reference itself leaves too many frames undecided"
        if T in _model_lengths(case):
            assert tg.evq_rule_failures(ref, _model(ref)) == [], (case.id, T)
    if case.N >= 2:
        for st, n_q in ((1, case.N), (0, case.N - 1)):
            ref = tg.evq_reference(case, 17, st, n_q)
            assert ref["undecided"] <= tg.UNDECIDED_CAP, (case.id, st, n_q)
            if case.K * case.DP <= MODEL_WORK_CAP:
                out = _model(ref)
                assert out["codes"].shape[0] == n_q - st and tg.evq_rule_failures(ref, out) == [], (case.id, st, n_q)


def tie_failures(case, mutant=None):
    """the GPU test's rule on the model: every code below K/2 and equal to the run on the half codebook (which has no ties and is run unmutated)"""
    full, half, z = tg.evq_tie_inputs(case, case.Ts[0])
    got = tg.evq_model([_np(c) for c in full], _np(z), mutant=mutant)["codes"]
    want = tg.evq_model([_np(c) for c in half], _np(z))["codes"]
    bad = []
    if not (got.max() < case.K // 2 and got.min() >= 0):
        bad.append("code >= K/2")
    if not np.array_equal(got, want):
        bad.append("differs from the half codebook")
    return bad


@pytest.mark.parametrize("case", tg.EVQ_TIES, ids=lambda c: c.id)
def test_evq_model_resolves_ties_to_the_lowest_index(case):
    assert tie_failures(case) == []


MUTANT_T = 17
MUTANT_ROWS = [c for c in tg.EVQ if c.K * c.DP <= 40_000]


def _evq_catchers(mutant):
    found = {}
    for case in MUTANT_ROWS:
        runs = [(0, None)] + ([(1, case.N)] if case.N >= 2 else [])
        for st, n_q in runs:
            ref = tg.evq_reference(case, MUTANT_T, st, n_q)
            bad = tg.evq_rule_failures(ref, _model(ref, mutant))
            if bad:
                found[f"{case.id}/st{st}"] = bad
    for case in tg.EVQ_TIES:
        bad = tie_failures(case, mutant)
        if bad:
            found["ties/" + case.id] = bad
    return found


def test_unmutated_evq_model_passes_every_rule():
    assert _evq_catchers(None) == {}


@pytest.mark.parametrize("mutant", tg.EVQ_MUTANTS)
def test_evq_mutant_is_caught(mutant):
    found = _evq_catchers(mutant)
    print(f"{mutant}: caught by " + ", ".join(f"{k} ({' + '.join(v)})" for k, v in found.items()))
    assert found, f"no row of the table catches the mutant {mutant}: the table is missing a case"
    rows = {k.split("/")[0] for k in found if not k.startswith("ties/")}
    ties = {k[5:] for k in found if k.startswith("ties/")}
    by_id = {c.id: c for c in tg.EVQ}
    if mutant in ("pad_not_zeroed", "update_stride_D"):                # only a padded row has a tail to leave or a stride to get wrong
        assert all(by_id[r].padded for r in rows) and all(tg.evq_by_id(t).padded for t in ties)
        assert any(by_id[r].K < 4 for r in rows) and any(by_id[r].K > 256 for r in rows)
    if mutant == "scan_le":                                            # only an exact tie inside one thread's own rows
        assert not rows and ties == {c.id for c in tg.EVQ_TIES if "thread" in tg.evq_tie_relation(c)}
    if mutant == "merge_prefers_higher":                               # only an exact tie between two threads
        assert not rows and ties == {c.id for c in tg.EVQ_TIES if tg.evq_tie_relation(c) & {"wave", "waves"}}
    if mutant == "guard_dropped":                                      # only where K is no multiple of 4
        assert all(by_id[r].K % 4 for r in rows) and any(by_id[r].K < 4 for r in rows) and all(tg.evq_by_id(t).K % 4 for t in ties)
    if mutant == "st_from_residual":
        assert all(k.endswith("/st1") for k in found)


# ------------------------------------------------------------------------------------------------------------------------------
# the LSTM step
# ------------------------------------------------------------------------------------------------------------------------------
def _recur_failures(Hn, bidir, T, Bn, seed, with_skip, mutant=None, scale=1.0):
    w, gx, skip = tg.recur_case(Hn, bidir, T, Bn, seed, scale=scale)
    w_hh = torch.stack(w[1], 0)
    sk = skip if with_skip else None
    ref64 = R.lstm_recur(w_hh.double(), gx.double(), None if sk is None else sk.double())
    ref32 = R.lstm_recur(w_hh, gx, sk)
    y = torch.from_numpy(tg.lstm_model(_np(w_hh), _np(gx), None if sk is None else _np(sk), mutant)).double()
    bound = tg.lstm_bound(ref64, ref32, 1e-6)
    err = float((y - ref64).abs().max()) if bool(torch.isfinite(y).all()) else float("inf")
    return err / bound


@pytest.mark.parametrize("Hn", tg.LSTM_H)
def test_lstm_model_on_the_hidden_axis(Hn):
    for bidir in (False, True):
        r = _recur_failures(Hn, bidir, max(tg.LSTM_H_T), tg.B, 100 + Hn, with_skip=bidir)
        print(f"lstm model H={Hn} bidir={bidir}: error / bound {r:.3f}")
        assert r <= 1.0, (Hn, bidir, r)


def test_lstm_model_on_the_batch_axis_and_over_many_steps():
    for Hn in tg.LSTM_B_H:
        for Bn in tg.LSTM_B:
            r = _recur_failures(Hn, True, tg.LSTM_B_T, Bn, 200 + Hn + Bn, True)
            assert r <= 1.0, (Hn, Bn, r)
    for Hn, T in tg.LSTM_LONG:
        r = _recur_failures(Hn, True, T, 2, 300 + Hn, False)
        print(f"lstm model H={Hn} T={T}: error / bound {r:.3f}")
        assert r <= 1.0, (Hn, T, r)
    Hn, T, scale = tg.LSTM_SATURATED
    r = _recur_failures(Hn, True, T, tg.B, 400, False, scale=scale)
    print(f"lstm model H={Hn} T={T} gx x {scale}: error / bound {r:.3f}")
    assert r <= 1.0


def test_lstm_model_saturated_gates_are_exact():
    Hn, T = 96, 5
    gx, zero, held = tg.saturated_gx(Hn, T, tg.B, 7)
    w = tg.lstm_weights(Hn, Hn, 1, False, 8)
    y = tg.lstm_model(_np(torch.stack(w[1], 0)), _np(gx))
    assert np.isfinite(y).all() and (y[:, zero[0]:zero[1]] == 0).all()
    assert (y[:, held[0]:held[1], 1:] == y[:, held[0]:held[1], :1]).all() and (y[:, held[0]:held[1], 0] != 0).any()


def _forward_failures(In, Hn, L, bidir, skip, T, mutant=None):
    w = tg.lstm_weights(In, Hn, L, bidir, 500 + In + Hn + L)
    P = tg.lstm_named(w, L, bidir)
    x = torch.randn(tg.B, In, T, generator=torch.Generator().manual_seed(In + T))
    ref64 = R.slstm({k: v.double() for k, v in P.items()}, "", x.double(), L, bidir, skip)
    ref32 = R.slstm(P, "", x, L, bidir, skip)
    y = tg.lstm_forward_model(P, x, L, bidir, skip, mutant).double()
    err = float((y - ref64).abs().max()) if bool(torch.isfinite(y).all()) else float("inf")
    return err / tg.lstm_bound(ref64, ref32, 1e-4)


LSTM_MUTANT_ROWS = [("H", 3, True), ("H", 64, True), ("H", 65, False), ("H", 260, True), ("B", 12, 5), ("B", 12, 17), ("B", 70, 33),
                    ("F", (12, 12, 3, True, True)), ("F", (7, 12, 1, True, False))]


def _lstm_catchers(mutant):
    found = []
    for row in LSTM_MUTANT_ROWS:
        if row[0] == "H":
            r = _recur_failures(row[1], row[2], max(tg.LSTM_H_T), tg.B, 100 + row[1], row[2], mutant)
        elif row[0] == "B":
            r = _recur_failures(row[1], True, tg.LSTM_B_T, row[2], 200 + row[1] + row[2], True, mutant)
        else:
            r = _forward_failures(*row[1], T=7, mutant=mutant)
        if not r <= 1.0:
            found.append(row)
    return found


def test_unmutated_lstm_model_passes_every_row():
    assert _lstm_catchers(None) == []


@pytest.mark.parametrize("mutant", tg.LSTM_MUTANTS)
def test_lstm_mutant_is_caught(mutant):
    found = _lstm_catchers(mutant)
    print(f"{mutant}: caught by {found}")
    assert found, f"no row catches the mutant {mutant}"
    if mutant == "tail_from_previous_tile":                            # only a tail tile behind a full one
        assert found == [("B", 12, 17), ("B", 70, 33)]
    if mutant == "quad_stride":                                        # only the 16-byte path with more than 16 quads
        assert found == [("H", 260, True)]
    if mutant == "dir1_not_reversed":
        assert all(r[0] == "F" or r[0] == "B" or r[2] for r in found) and ("H", 65, False) not in found
    if mutant == "skip_both_layers":
        assert found == [("F", (12, 12, 3, True, True))]


# ------------------------------------------------------------------------------------------------------------------------------
# the down-sampling conv's window
# ------------------------------------------------------------------------------------------------------------------------------
def test_dsconv_window_indexing_is_the_strided_conv():
    g = torch.Generator().manual_seed(3)
    w = 1.0 + torch.rand(3, generator=g).double()                      # taps and samples of at least 1: an edge sample repeated is an error of at least 1
    lengths = sorted({T for c in tg.DSCONV + [tg.DS_RANGE] for T in c.Ts})
    for T in lengths:
        x = 1.0 + torch.rand(T, generator=g).double()
        ref = Fn.conv1d(x[None, None], w[None, None], stride=2, padding=1)[0, 0].numpy()
        for TN in (64, 128):
            y = tg.ds_window_model(x.numpy(), w.numpy(), TN)
            assert y.shape == ref.shape and np.abs(y - ref).max() <= 1e-12, (T, TN)
            bad = tg.ds_window_model(x.numpy(), w.numpy(), TN, clamp=True)
            assert np.abs(bad - ref).max() > 1e-3, f"T={T} TN={TN}: a clamp in place of the zero select goes unnoticed"
