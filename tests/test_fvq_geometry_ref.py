"""CPU: (1) the quantizer geometry table (tests/fvq_geometry.py) reaches every class of the kernels' index arithmetic it is meant to -- all three
row paddings DP with padded and unpadded rows, K < 16, K and D no multiple of 16, D no multiple of 4, identity and projected, both l2 settings,
an encode LDS request above 128 KB, a decode request above 64 KB, N = 32, K = 16384 -- and the semantic-prepare table every crossing of its
64 x 32 tile; (2) the fp64 reference alone decides (margin rule of codec_ref) at least 98 % of the frames of every encode case at every length
the GPU tests use; (3) a numpy fp32 model of csrc/fvq.hip's encode kernel gives the fp64 codes on every decided frame and zq / latents within the
suite's rule, while one-slip mutants of it (row stride d instead of DP, scan started one row late, <= in the scan, merge preferring the higher
index, padded rows not zeroed) are each caught by the rules the GPU tests apply, on cases of this table; (4) the d = 1, l2 case ties exactly and
resolves by sign; (5) amp_fvq_create judges its arguments on the host, before it asks for a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import fvq_geometry as fg  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------------------
# the tables hold what they are meant to
# ------------------------------------------------------------------------------------------------------------------------------
def test_encode_table_reaches_every_class():
    cases = fg.ALL_ENCODE
    assert len({c.name for c in cases + fg.TIES + [fg.SIGN]}) == len(cases) + len(fg.TIES) + 1
    for c in cases + fg.TIES + [fg.SIGN]:
        assert 1 <= c.D <= fg.MAX_D and 1 <= c.d <= fg.MAX_d and 1 <= c.K <= fg.MAX_K and 1 <= c.N <= fg.MAX_N, c.id
        assert c.DP in (8, 16, 32) and c.d <= c.DP and (c.DP == 8 or c.d > c.DP // 2), c.id
        assert all(fg.B * T <= 150 for T in c.Ts), c.id
        assert c.N * fg.B * c.D * max(c.Ts) * 4 + 1024 <= fg.DEVICE_TENSOR_CAP, c.id          # all_zq, the largest tensor of a case
    for DP in (8, 16, 32):
        at = [c for c in fg.ENCODE if c.DP == DP]
        assert any(c.padded for c in at) and any(not c.padded for c in at), DP
        assert any(c.identity for c in at) and any(not c.identity for c in at), DP
    assert any(c.identity and c.padded for c in fg.ENCODE)
    assert any(c.K < 16 for c in fg.ENCODE) and any(c.K == 16 for c in fg.ENCODE)
    assert any(c.K % 16 and c.K > 16 for c in fg.ENCODE)
    assert any(c.D % 16 and c.D > 16 and not c.identity for c in fg.ENCODE)
    assert any(c.D < 16 and not c.identity for c in fg.ENCODE) and any(c.D < 4 and not c.identity for c in fg.ENCODE)
    assert {c.D % 4 for c in fg.ENCODE if not c.identity} == {0, 1, 2, 3}        # in_project's four parts sum unequal counts
    assert {c.l2 for c in fg.ENCODE} == {True, False}
    for DP in (8, 16, 32):
        assert {c.l2 for c in fg.ENCODE if c.DP == DP} == {True, False}, DP
    assert max(fg.encode_lds_bytes(c.D, c.d) for c in fg.ENCODE) > 128 * 1024
    assert max(fg.encode_lds_bytes(c.D, c.d) for c in fg.ENCODE) == fg.encode_lds_bytes(fg.MAX_D, fg.MAX_d) <= 160 * 1024
    assert fg.decode_lds_bytes(fg.DECODE_LDS.N, fg.DECODE_LDS.d) > 64 * 1024
    assert fg.decode_lds_bytes(fg.MAX_N, fg.MAX_d) == fg.decode_lds_bytes(fg.DECODE_LDS.N, fg.DECODE_LDS.d) <= 160 * 1024
    assert all(fg.decode_lds_bytes(c.N, c.d) <= 64 * 1024 for c in fg.ENCODE)        # no other case reaches it
    assert any(c.N == fg.MAX_N for c in fg.ENCODE) and any(c.N == 1 for c in fg.ENCODE)
    assert sum(c.K == fg.MAX_K for c in fg.ENCODE) == 2 and {c.DP for c in fg.ENCODE if c.K == fg.MAX_K} == {8, 32}
    assert any(c.D == fg.MAX_D and c.d == fg.MAX_d for c in fg.ENCODE)
    assert any(c.d == 1 for c in fg.ENCODE) and any((c.D, c.d, c.K, c.N) == (1, 1, 1, 1) for c in fg.ENCODE)
    # the lengths: one frame, a length that is no multiple of the 16-frame tile, several tiles
    for c in fg.ENCODE:
        assert 1 in c.Ts and any(T % fg.FVQ_TF and T > fg.FVQ_TF for T in c.Ts), c.id
    # the largest N sits under l2 (without it the fp64 reference leaves more than the cap undecided); the decode case is outside the cap
    assert all(c.l2 for c in fg.ENCODE if c.N == fg.MAX_N) and not fg.DECODE_LDS.margin and all(c.margin for c in fg.ENCODE)
    # ties: one per DP, a padded one, a row and its copy in the same thread (K/2 a multiple of 16) and in different threads
    assert {c.DP for c in fg.TIES} == {8, 16, 32} and any(c.padded for c in fg.TIES) and all(c.K % 2 == 0 for c in fg.TIES)
    assert any((c.K // 2) % 16 == 0 for c in fg.TIES) and any((c.K // 2) % 16 for c in fg.TIES)
    # a copy in another wave ((k + K/2) / 4 mod 4 differs) and in the same wave
    for c in fg.TIES:
        if (c.K // 2) % 16:
            h = c.K // 2
            waves = {((k % 16) // 4 == ((k + h) % 16) // 4) for k in range(h)}
            assert waves == {True, False}, c.id
    assert fg.SIGN.d == 1 and fg.SIGN.l2 and not fg.SIGN.identity
    assert {fg.by_name(n).DP for n in fg.PER_DP} == {8, 16, 32} and any(fg.by_name(n).padded for n in fg.PER_DP)


def test_semantic_table_covers_the_crossings():
    rows = [(b, T, C, f, T // f) for b, T, C, f in fg.SEMANTIC]
    assert {r[2] for r in rows} == {1, 63, 64, 65, 130}
    assert {r[4] for r in rows} == {1, 31, 32, 33, 70}
    assert {r[3] for r in rows} == {1, 2, 3, 5}
    assert any(T % f for _, T, _, f, _ in rows) and any(T % f == 0 and f > 1 for _, T, _, f, _ in rows)
    assert sum(b == 3 for b, *_ in rows) == 1 and all(b in (2, 3) for b, *_ in rows)
    # both tile counts on both axes, ragged and full last tiles, together at least once
    assert any(C > fg.SP_TC and To > fg.SP_TT and C % fg.SP_TC and To % fg.SP_TT for _, _, C, _, To in rows)
    assert any(C == fg.SP_TC and To == fg.SP_TT for _, _, C, _, To in rows)
    assert any(C < fg.SP_TC and To > fg.SP_TT for _, _, C, _, To in rows) and any(C > fg.SP_TC and To < fg.SP_TT for _, _, C, _, To in rows)
    assert len(rows) <= 12 and all(b * T * C * 4 + 1024 <= fg.DEVICE_TENSOR_CAP for b, T, C, _, _ in rows)


# ------------------------------------------------------------------------------------------------------------------------------
# the fp64 reference decides the cases; the model of the kernel agrees with it
# ------------------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy()


def _model(case, T, ref, mutant=None):
    return fg.fvq_model(case.hp, fg.model_weights(ref["sd"], case.hp), _np(ref["z"]), mutant=mutant)


def margin_rule_failures(case, T, out, ref):
    """what the GPU test asserts of an encode under the margin rule, applied to `out` (numpy): -> list of the rules broken"""
    bad = []
    codes = torch.from_numpy(out["codes"])
    if not bool((codes == ref["r64"]["codes"])[ref["decided"]].all()):
        bad.append("codes")
    zmax = float(ref["z"].abs().max())
    for which, key in (("zq", "zq"), ("latents", "latents")):
        bound, mask = fg.restatement_bound(ref, which, zmax)
        got = torch.from_numpy(np.ascontiguousarray(out[key])).double()
        err = (got - ref["r64"][which])[mask].abs()
        if err.numel() and not float(err.max()) <= bound:          # (a NaN fails)
            bad.append(which)
    excess = fg.excess_over_minimum(ref["sd"], case.hp, ref["z"], codes)
    if not float(excess.max()) <= ref["tau"]:
        bad.append("near-optimality")
    return bad


@pytest.mark.parametrize("case", fg.ALL_ENCODE, ids=lambda c: c.name)
def test_fp64_decides_and_the_model_agrees(case):
    for T in case.Ts:
        ref = fg.reference(case, T)
        print(f"{case.id} T={T}: tau {ref['tau']:.3e}, smallest fp64 margin {float(ref['r64']['margin'].min()):.3e}, "
              f"undecided frames {ref['undecided']:.4f}")
        if case.margin:
            assert ref["undecided"] <= fg.UNDECIDED_CAP, "the fp64 reference itself leaves too many frames undecided for this seed"
        out = _model(case, T, ref)
        if case.margin:
            assert margin_rule_failures(case, T, out, ref) == [], (case.id, T)
        else:
            excess = fg.excess_over_minimum(ref["sd"], case.hp, ref["z"], torch.from_numpy(out["codes"]))
            assert float(excess.max()) <= ref["tau"], (case.id, T)
        acc = np.zeros_like(out["all_zq"][0])
        for q in out["all_zq"]:
            acc = (acc + q).astype(np.float32)
        assert np.array_equal(acc, out["zq"])


# ------------------------------------------------------------------------------------------------------------------------------
# exact ties and the sign case
# ------------------------------------------------------------------------------------------------------------------------------
def tie_rule_failures(case, mutant=None):
    """test_fvq_ties_resolve_to_lowest_index's rule on the model: every code below K/2 and equal to the run on the half codebook (the half
    codebook has no ties, so it is run unmutated: it is the expectation)"""
    T = case.Ts[0]
    sd, hhp, half = fg.tie_weights(case)
    z = _np(fg.latent(case, T))
    full = fg.fvq_model(case.hp, fg.model_weights(sd, case.hp), z, mutant=mutant)["codes"]
    want = fg.fvq_model(hhp, fg.model_weights(half, hhp), z)["codes"]
    bad = []
    if not (full.max() < case.K // 2 and full.min() >= 0):
        bad.append("code >= K/2")
    if not np.array_equal(full, want):
        bad.append("differs from the half codebook")
    return bad


@pytest.mark.parametrize("case", fg.TIES, ids=lambda c: c.name)
def test_model_resolves_ties_to_the_lowest_index(case):
    assert tie_rule_failures(case) == []


def sign_rule_failures(mutant=None):
    case = fg.SIGN
    T = case.Ts[0]
    sd = fg.weights(case)
    W = fg.model_weights(sd, case.hp)
    out = fg.fvq_model(case.hp, W, _np(fg.latent(case, T)), mutant=mutant)
    bad = []
    for l in range(case.N):
        want = fg.sign_rule_codes(W["cb"][l][:, 0], out["latents"][:, l, :])
        if not np.array_equal(out["codes"][l], want):
            bad.append(f"level {l}")
    return bad, out, W


def test_sign_case_ties_on_purpose():
    """d = 1 with l2: distances are exactly 0 or 4, the code is the lowest index of z_e's sign.  The case has rows of both signs at every level and
    frames of both signs, and its first matching row is not always row 0 or 1: the lowest-index rule has something to decide."""
    case = fg.SIGN
    bad, out, W = sign_rule_failures()
    assert bad == []
    for l in range(case.N):
        s = np.sign(W["cb"][l][:, 0])
        assert (s > 0).any() and (s < 0).any(), l
        ze = out["latents"][:, l, :]
        assert (ze > 0).any() and (ze < 0).any(), l
        assert (np.sign(W["cb"][l][:, 0]) == s[out["codes"][l]].reshape(-1, 1)).sum(1).min() >= 2      # every chosen row has an equal rival
    # fp64 sees the same exact distances; the near-optimality rule holds with any tau
    excess = fg.excess_over_minimum(fg.weights(case), case.hp, fg.latent(case, case.Ts[0]), torch.from_numpy(out["codes"]))
    assert float(excess.max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# one-slip mutants of the kernel: each is caught by a rule of the GPU tests on a case of the table
# ------------------------------------------------------------------------------------------------------------------------------
MUTANT_T = 17


def expected_catchers(mutant):
    """what the slip's own nature says, before any run: -> (cases that must catch it, cases that cannot)"""
    small = [c for c in fg.ALL_ENCODE if c.K <= 1000]
    everything = small + fg.TIES + [fg.SIGN]
    if mutant in ("stride_d", "padding_not_zeroed"):
        # only a padded row has a stride to get wrong or a tail to leave unzeroed.  With K = 1 every answer is row 0
        must = [c for c in small if c.padded and c.K > 1] + [c for c in fg.TIES if c.padded]
        return must, [c for c in everything if not c.padded]
    if mutant == "scan_le":
        # only an exact tie inside one thread's own rows tells <= from <: a row and its copy K/2 apart with K/2 a multiple of 16
        must = [c for c in fg.TIES if (c.K // 2) % 16 == 0]
        return must, [c for c in everything if c not in must and c is not fg.SIGN]
    if mutant == "merge_prefers_higher":
        # only an exact tie between two threads
        must = [c for c in fg.TIES if (c.K // 2) % 16] + [fg.SIGN]
        return must, [c for c in everything if c not in must]
    return [], []                                # scan_start_plus_1 never sees row 0: caught wherever row 0 wins a decided frame


def _catchers(mutant):
    found = {}
    for case in fg.ALL_ENCODE:
        if case.K > 1000:                        # the two K = 16384 cases add nothing a smaller K does not show, at 16 x the time
            continue
        ref = fg.reference(case, MUTANT_T)
        out = _model(case, MUTANT_T, ref, mutant)
        if case.margin:
            bad = margin_rule_failures(case, MUTANT_T, out, ref)
        else:
            excess = fg.excess_over_minimum(ref["sd"], case.hp, ref["z"], torch.from_numpy(out["codes"]))
            bad = [] if float(excess.max()) <= ref["tau"] else ["near-optimality"]
        if bad:
            found[case.name] = bad
    for case in fg.TIES:
        bad = tie_rule_failures(case, mutant)
        if bad:
            found[case.name] = bad
    bad = sign_rule_failures(mutant)[0]
    if bad:
        found[fg.SIGN.name] = bad
    return found


def test_unmutated_model_passes_every_rule():
    assert _catchers(None) == {}


@pytest.mark.parametrize("mutant", fg.MUTANTS)
def test_mutant_is_caught(mutant):
    found = _catchers(mutant)
    print(f"{mutant}: caught by " + ", ".join(f"{k} ({' + '.join(v)})" for k, v in found.items()))
    assert found, f"no case of the table catches the mutant {mutant}: the table is missing a case"
    must, cannot = expected_catchers(mutant)
    assert all(c.name in found for c in must), (mutant, [c.name for c in must if c.name not in found])
    assert not any(c.name in found for c in cannot), (mutant, [c.name for c in cannot if c.name in found])


# ------------------------------------------------------------------------------------------------------------------------------
# the refusals that need no device
# ------------------------------------------------------------------------------------------------------------------------------
def test_create_refuses_on_the_host():
    from amphion_amd import _lib

    L = _lib.lib()
    assert _lib.AMP_ERR_INVALID == fg.AMP_ERR_INVALID and _lib.AMP_ERR_UNSUPPORTED == fg.AMP_ERR_UNSUPPORTED
    for (D, d, K, N), given, poison, status, word in fg.CREATE_REFUSALS:
        for l2 in (1, 0):
            args, keep = fg.create_args(fg.refusal_weights(D, d, K, N, poison), given)
            h = ctypes.c_void_p()
            rc = L.amp_fvq_create(D, d, K, N, l2, *args, ctypes.byref(h))
            msg = L.amp_last_error().decode()
            assert rc == status and word in msg and not h.value, ((D, d, K, N), given, poison, l2, rc, msg)
            del keep
    args, keep = fg.create_args(fg.refusal_weights(8, 8, 16, 1), "none")
    h = ctypes.c_void_p()
    assert L.amp_fvq_create(8, 8, 16, 1, 1, None, None, None, None, None, ctypes.byref(h)) == fg.AMP_ERR_INVALID          # no codebook
    assert L.amp_fvq_create(8, 8, 16, 1, 1, *args, None) == fg.AMP_ERR_INVALID                                            # nowhere to put the handle
    # the entry points judge the handle first
    fake = ctypes.c_void_p(4096)
    assert L.amp_fvq_encode(None, fake, 1, 8, 1, fake, None, None, None) == fg.AMP_ERR_INVALID
    assert L.amp_fvq_decode(None, fake, 1, 1, 8, fake, None) == fg.AMP_ERR_INVALID
    assert L.amp_fvq_check(None, None) == fg.AMP_ERR_INVALID
