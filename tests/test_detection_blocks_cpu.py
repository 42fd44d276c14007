"""The case list of tests/test_gpu_detection_blocks.py, without a GPU: every case is built and run through the oracle, the
oracle stays inside the float64 bound of every op (f64_ref.check_graph), no case is vacuous, and the list covers what it
claims (a table computed from the list, not from its construction).

With this passing, the reference alone is known to satisfy every condition the GPU test imposes; what is left for the GPU
is the bit comparison of the kernels with that reference.
"""
import numpy as np
import pytest

import detblock_util as D
import f64_ref as R
from oracle.nn import OracleGraph


@pytest.mark.parametrize("case", D.CASES, ids=[c.id for c in D.CASES])
def test_oracle_stays_inside_the_float64_bound_and_the_case_is_not_vacuous(case):
    built = D.build(case)
    for name, (buf, out) in built.graphs.items():
        _, slots = OracleGraph(buf).run_exact(built.x, return_slots=True)
        D.self_checks(case, built, slots)
        # float64, op by op, on the case's finite inputs (the non-finite group: the same case with those elements finite)
        worst = R.check_graph(buf, built.x_finite, case.id + " " + name)
        assert max(w for _, w in worst) <= 1.0
        o = slots[out]
        if case.values == "nonfinite":
            twin = OracleGraph(buf).run_exact(built.x_finite, return_slots=True)[1][out]
            if not any(case.relu):
                assert np.isnan(o).any(), "%s: no NaN reaches the output" % case.id
            else:     # (a ReLU turns NaN and -Inf into 0: the values may all be finite again, but not those of the finite input)
                assert not np.array_equal(o, twin, equal_nan=True), "%s: the non-finite inputs change nothing" % case.id
            assert np.isfinite(o).mean() > 0.25, "%s: hardly anything finite is left to compare" % case.id
        if case.values == "tiny":
            src = slots[built.slots["src"]]
            assert ((src != 0) & (np.abs(src) < R.MIN_NORMAL)).any(), "%s: no subnormal reaches the block" % case.id
            if case.tail in ("pool", "y") and not case.relu[3]:      # (a ReLU's zeros are all +0.0)
                z = o[o == 0]
                assert z.size and np.signbit(z).any() and (~np.signbit(z)).any(), "%s: the output's zeros have one sign" % case.id
    if case.tail == "pool" and not case.relu[3] and case.h * case.w >= 64:
        _, slots = OracleGraph(built.graphs["ypool"][0]).run_exact(built.x_finite, return_slots=True)
        assert (slots[built.slots["ypool"]] < 0).any(), "%s: the pool sees no negative maximum" % case.id
    # the companion is the same block: same weights, same block output
    _, cs = OracleGraph(built.companion).run_exact(built.x_finite, return_slots=True)
    name, (buf, _) = next(iter(built.graphs.items()))
    _, ms = OracleGraph(buf).run_exact(built.x_finite, return_slots=True)
    assert np.array_equal(cs[built.slots["y"]], ms[built.slots["y"]], equal_nan=True)
    comp_out = OracleGraph(built.companion).run_exact(built.x_finite)
    assert comp_out.shape == (case.n, 1, case.h, case.w)


def _straddles(values, t, with_double=False):
    need = {t - 1, t, t + 1} | ({2 * t + 1} if with_double else set())
    return need <= values


def test_the_case_list_covers_what_it_claims():
    cov = D.coverage()
    assert len({c.id for c in D.CASES}) == len(D.CASES)
    lines = []
    for shape in D.SHAPES:
        s = cov[shape]
        for tail, relus in s["relu"].items():
            assert relus == set(D.RELUS), (shape, tail)
        if shape == "dec8f":
            assert set(s["relu"]) == {"fin", "finsig"}
        if D.is_dec(shape):
            assert set(D.PAD_PAIRS) <= s["pads"], (shape, sorted(set(D.PAD_PAIRS) - s["pads"]))
            pyo = {p[0] // 2 for p in s["pads"]}
            pxo = {p[1] // 2 for p in s["pads"]}
            assert {0, 1, 2} <= pyo and {0, 1, 2} <= pxo
        assert set(range(1, 10)) <= s["n"], shape
        if shape not in D.TABLE:
            assert set(s["fam"]) == {(None, 0)}, shape        # never fused: the per-operator kernels
            continue
        fams = {f for f, _ in s["fam"]}
        assert fams == {None, "tiled"} | ({"wave"} if shape in D.WAVE else set()) | ({"rows"} if shape in D.ROWS else set()), shape
        th, tw = D.TILE[shape]
        for (f, seg), d in sorted(s["fam"].items(), key=str):
            if f is None:
                continue
            if f == "tiled":
                ok_h, ok_w = _straddles(d["h"], th, True), _straddles(d["w"], tw, True)
            else:
                segs = D.WAVE_S if f == "wave" else D.ROWS_S
                if seg == 1:            # the height is chosen from the request size: some segment height, covered below
                    continue
                assert seg in segs
                ok_h = _straddles(d["h"], seg)
                ok_w = _straddles(d["w"], D.STRIP) and _straddles(d["w"], 2 * D.STRIP) and min(d["w"]) < D.STRIP
            assert ok_h and ok_w, (shape, f, seg)
            assert {2, 3} <= d["h"] and {2, 3} <= d["w"], (shape, f, seg)          # from 2 upwards, odd under the pool
            assert d["relu"] == set(D.RELUS), (shape, f, seg)
            pads_needed = set(D.PAD_PAIRS) if D.is_dec(shape) else set()
            if f == "rows":
                pads_needed = {p for p in pads_needed if not (p[1] // 2) & 1}
                assert {p[1] // 2 for p in d["pads"]} >= ({0, 2, 22} if D.is_dec(shape) else set())
            assert pads_needed <= d["pads"], (shape, f, seg)
            assert set(range(1, 10)) <= d["n"], (shape, f, seg)
            lines.append("%-6s %-5s S=%-2d  h %s  w %s  pads %d  relu %d  n %s" % (
                shape, f, seg, sorted(d["h"]), sorted(d["w"]), len(d["pads"]), len(d["relu"]), sorted(d["n"])))
        if shape in D.ROWS:
            assert "n>8" in s["declined"], shape
            assert ("odd pxo" in s["declined"]) == D.is_dec(shape), shape
            assert set(range(1, 9)) <= cov[shape]["fam"][("rows", 1)]["n"] and 9 not in cov[shape]["fam"][("rows", 1)]["n"]
            if D.is_dec(shape):        # pxo = 1 (declined by the row kernels) lands on the tiled kernel
                assert any((p[1] // 2) & 1 for p in cov[shape]["fam"][("tiled", 0)]["pads"])
        if shape in ("dec8", "dec8f"):
            assert any((p[1] // 2) & 1 for p in cov[shape]["fam"][("wave", 8)]["pads"])
    print("\n".join(lines))
