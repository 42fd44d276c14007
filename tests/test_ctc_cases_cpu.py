"""The CTC decode cases (ctc_cases.py) walked on the definitions alone — no library, no GPU: every case must really
exercise the branch it is named for, every batch must tell its lines apart, and the definition must stay cheap enough for
the GPU tests that run it again on the log-probs the kernels return (test_gpu_ctc_decode.py).

The conditions are evaluated on a float32 LogSoftmax of the cases' logits (ctc_cases.log_softmax32); they rest on equal
logits and -inf logits, which any LogSoftmax keeps.  NaN log-probs are out of scope: no case holds one, and what the
decode kernels do with a NaN stays unpinned."""
import numpy as np
import pytest

import confidence_ref as CR
import ctc_cases as CC


def _labels(case, z, masked=True):
    L = CC.log_softmax32(z)
    L = CR.masked(L, case.excluded) if masked else L
    return [CR.row_argmax(r)[0] for r in L], L


def _maxima(L):
    return [int((r == r.max()).sum()) for r in L]


# ---------------------------------------------------------------- geometries
def test_geometries_are_what_their_names_say():
    G = CC.GEOMETRIES
    assert G["g1"] == [1] and G["g2"] == [5, 1] and G["lds"] == [12, 7, 1]
    g3 = G["g3"]
    assert len(g3) == 65 and g3[0] == 40 and g3[-1] == 1 and g3 == sorted(g3, reverse=True)
    assert len(set(g3)) == 40 and max(g3.count(v) for v in set(g3)) >= 2           # every length 40 .. 1, with plateaus
    assert len(CC.packed_slots(g3)) - 64 == 1                                         # the second wave has one live lane
    g4 = G["g4"]
    assert len(g4) == 130 and set(g4) == {15, 16, 17, 31, 32, 33} and g4 != sorted(g4, reverse=True)
    slots = [g4[i] for i in CC.packed_slots(g4)]
    for wave in (slots[:64], slots[64:128]):                                          # lengths mixed within each wave
        assert len(set(wave)) >= 3
    assert {33, 32, 31, 17} <= set(slots[:64])       # one wave: lines ending in block 3, at t = 32 | 31 and inside block 2
    assert 0 < len(slots[128:]) < 64                                                  # lanes m >= M in the last wave
    for name in ("g5", "g5s"):
        g5 = G[name]
        assert len(g5) == 20 and g5.count(0) >= 3 and g5[-1] == max(g5) and g5.count(max(g5)) == 1
        assert g5 != sorted(g5, reverse=True) and CC.packed_slots(g5)[0] == 19
    assert max(G["g5"]) == 48 and max(max(g) for g in G.values()) <= 48


def test_case_lists_cover_the_grid():
    assert {c.C for c in CC.GREEDY_CASES} == {2, 5, 97}
    assert {c.geometry for c in CC.GREEDY_CASES} == {"g1", "g2", "g3", "g4", "g5"}
    for script in CC.GREEDY_SCRIPTS:
        for g in CC.GREEDY_GEOMETRIES:
            assert any(c.kind == script and c.geometry == g for c in CC.GREEDY_CASES)
    assert {c.C for c in CC.BEAM_CASES} == {2, 5, 20, 97, 128, 119, 3}   # 119, W = 120: the largest partners of 128
    assert {c.width for c in CC.BEAM_CASES} == {1, 2, 7, 32, 128, 120, 4}   # C = 3, W = 4: revived prefixes
    assert {c.kind for c in CC.BEAM_CASES} == {"sharp", "flat", "quant", "excl"}
    for C, W, kind in CC.BEAM_SETS:           # each matrix set runs on g2 and on g5
        gs = {c.geometry for c in CC.BEAM_CASES if (c.C, c.width, c.kind) == (C, W, kind)}
        assert "g2" in gs and gs & {"g5", "g5s"}
    on_g3 = [c for c in CC.BEAM_CASES if c.geometry == "g3"]
    assert {c.kind for c in on_g3} == {"sharp", "quant"} and all(c.width <= 7 and c.C <= 20 for c in on_g3)
    assert {(20, 7, "sharp"), (5, 7, "quant")} <= {(c.C, c.width, c.kind) for c in on_g3}
    lds = [c for c in CC.BEAM_CASES if c.geometry == "lds"]
    assert {(c.C, c.width) for c in lds} == {(97, 128), (119, 128), (128, 120)}
    lds_bytes = lambda C, W: (9 * W * C + 8 * C + 140 * W + 7232 + 15) & ~15      # kernels_beam.hip beam_lds_bytes
    assert all(64 * 1024 < lds_bytes(c.C, c.width) <= 160 * 1024 for c in lds)
    assert all(lds_bytes(C, W) > 160 * 1024 for C, W in CC.UNSUPPORTED_PAIRS)
    names = [c.name for c in CC.GREEDY_CASES + CC.BEAM_CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("case", CC.GREEDY_CASES + CC.BEAM_CASES, ids=repr)
def test_logits_are_finite_enough(case):
    """No NaN, no +inf, no row entirely -inf; a line's matrix has the line's length; the lines of a batch differ."""
    for z, T in zip(case.mats, case.lengths):
        assert z.dtype == np.float32 and z.shape == (T, case.C)
        assert not np.isnan(z).any() and not np.isposinf(z).any()
        assert T == 0 or np.isfinite(z).any(axis=1).all()
        L = CR.masked(CC.log_softmax32(z), case.excluded)
        assert not np.isnan(L).any() and (T == 0 or np.isfinite(L).any(axis=1).all())
    assert len({z.tobytes() for z in case.mats if z.size}) == sum(1 for z in case.mats if z.size)


# ---------------------------------------------------------------- greedy scripts
def _has_triple(lab, positions):
    return any(0 < t < len(lab) - 1 and lab[t] == 0 and lab[t - 1] == lab[t + 1] > 0 for t in positions)


@pytest.mark.parametrize("case", CC.GREEDY_CASES, ids=repr)
def test_greedy_case_reaches_its_branch(case):
    labs = [_labels(case, z)[0] for z in case.mats]
    kind, C = case.kind, case.C
    if kind == "repeat_boundary":
        for b in CC.BOUNDARIES:           # a repeat of one label across t = b - 1 | b
            assert any(len(l) > b and l[b - 1] == l[b] > 0 for l in labs), b
            hit = [(l, s) for l, (s, _, _) in zip(labs, CC.expected_on_stand_in(case)[0]) if len(l) > b and l[b - 1] == l[b] > 0]
            assert all(b not in [p for _, p in s] for _, s in hit)        # ... which adds no step at t = b
    elif kind == "blank_between":
        reached = set()
        for b in CC.BOUNDARIES:           # a 0 a with the blank at b - 1 and at b, wherever a line is long enough for it
            for mid in (b - 1, b):
                if any(T >= mid + 2 and CC.blank_mid(i, b) == mid for i, T in enumerate(case.lengths)):
                    assert any(_has_triple(l, [mid]) for l in labs), mid
                    reached.add(mid)
        assert reached >= {"g3": {15, 16, 31, 32}, "g4": {15, 16, 31}, "g5": {15, 31}}[case.geometry]
    elif kind == "all_blank":
        assert all(set(l) <= {0} for l in labs)
        assert all(s == [] for s, _, _ in CC.expected_on_stand_in(case)[0])
    elif kind == "one_label":
        assert all(len(set(l)) == 1 and l[0] > 0 for l in labs if l)
        assert all(len(s) == 1 and s[0][1] == 0 for (s, _, _), l in zip(CC.expected_on_stand_in(case)[0], labs) if l)
    elif kind == "last_label":
        assert any(C - 1 in [a for a, _ in s] for s, _, _ in CC.expected_on_stand_in(case)[0])
    elif kind == "ties":
        counts = set()
        for z in case.mats:
            lab, L = _labels(case, z)
            for t, n in enumerate(_maxima(L)):
                counts.add(n)
                if n > 1:                 # the first of the equal maxima is the label
                    assert lab[t] == int(np.flatnonzero(L[t] == L[t].max())[0])
        assert 2 in counts and (C == 2 or 3 in counts)
    else:                                  # excluded_max, exclusion_tie
        assert case.excluded
        changed = tied = 0
        for z in case.mats:
            lab, L = _labels(case, z)
            raw, R = _labels(case, z, masked=False)
            changed += sum(a != b for a, b in zip(lab, raw))
            assert all(r in case.excluded for a, r in zip(lab, raw) if a != r)      # the raw maximum was an excluded label
            tied += sum(1 for n, n0 in zip(_maxima(L), _maxima(R)) if n >= 2 and n0 == 1)
            assert not np.isneginf(R).any()
        assert changed > 0                 # the mask changes greedy labels
        assert kind != "exclusion_tie" or tied > 0


# ---------------------------------------------------------------- what every batch must satisfy
def _distinct(results, lengths, key):
    keys = [key(r) for r, T in zip(results, lengths) if T >= 4]
    return len(set(keys)) == len(keys)


@pytest.mark.parametrize("case", CC.GREEDY_CASES + CC.BEAM_CASES, ids=repr)
def test_lines_of_a_batch_are_told_apart_and_the_definition_is_quick(case):
    """The expected results of all lines with T >= 4 are pairwise different, so a kernel that reads another line's rows
    (a wrong m or off[t]) cannot pass: different in the steps alone, except where the case makes the steps equal by
    construction or the alphabet leaves them few (all blank, one label, C = 2 and C = 5 strings, flat, quantised and masked
    beam matrices) — there in steps and score together, which the scored methods return.  And the definition's time for the case stays under 5 s."""
    res, _, seconds = CC.expected_on_stand_in(case)
    both = lambda r: (tuple(r[0]), np.float64(r[2]).tobytes())
    assert _distinct(res, case.lengths, both)
    steps_alone = (case.width == 0 and case.kind not in ("all_blank", "one_label") and case.C == 97) or \
                  (case.width > 1 and case.kind == "sharp" and case.C >= 20)
    if steps_alone:
        assert _distinct(res, case.lengths, lambda r: tuple(r[0]))
    assert any(T >= 4 for T in case.lengths) or case.geometry == "g1"
    print("%s: definition %.3f s" % (case.name, seconds))
    assert seconds < 5.0


# ---------------------------------------------------------------- beam statistics
def _stats(pred):
    return [CC.expected_on_stand_in(c)[1] for c in CC.BEAM_CASES if pred(c)]


def test_quantised_cases_show_threshold_ties():
    """... on every geometry with enough steps to fill the width (g1 and g2 have one and five)."""
    quant = [c for c in CC.BEAM_CASES if c.kind == "quant" and c.geometry not in ("g1", "g2")]
    assert len(quant) >= 6
    assert [c.name for c in quant if CC.expected_on_stand_in(c)[1]["threshold_ties"] < 1] == []


def test_beam_cases_reach_short_steps_and_both_merge_orders():
    stats = _stats(lambda c: True)
    assert any(s["short"] >= 1 for s in stats)
    assert any(s["parent_earlier"] >= 1 for s in stats) and any(s["parent_later"] >= 1 for s in stats)
    wide = _stats(lambda c: (c.C, c.width) == (2, 128))
    assert wide and all(s["short"] == s["steps"] for s in wide)      # width above the candidate count at every step
    # the three-line opt-in launches prune for real: their lines fill the width
    for s in _stats(lambda c: c.geometry == "lds"):
        assert s["short"] < s["steps"]


def test_revived_prefixes_are_reached():
    """A prefix that fell out of the beams comes back beside a beam that extends it: the extension must merge with that
    beam although the prefix was away (an implementation that numbers prefixes when it creates them sees two)."""
    for c in CC.BEAM_CASES:
        if (c.C, c.width, c.kind, c.geometry) == (3, 4, "quant", "g3"):
            assert CC.expected_on_stand_in(c)[1]["revived"] >= 1, c.name
    assert sum(1 for c in CC.BEAM_CASES if CC.expected_on_stand_in(c)[1]["revived"] >= 1) >= 4
    for name, lp, w in CC.revived_matrices():
        stats = {}
        CR.beam_search(lp, w, stats)
        assert stats["revived"] >= 1, name


def test_stats_do_not_change_the_search():
    rng = np.random.default_rng(7)
    L = CC.log_softmax32(np.round(rng.normal(0, 1.5, (12, 6)) * 2) / 2)
    stats = {}
    assert CR.beam_search(L, 4) == CR.beam_search(L, 4, stats) == CR.beam_search(L, 4, None)
    assert set(stats) == set(CR.BEAM_STATS) and stats["steps"] == 12
    assert stats["merges"] <= 12 and stats["parent_later"] + stats["parent_earlier"] >= stats["merges"]
