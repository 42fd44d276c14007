"""The cases of the CTC decode tests: packed batch geometries, greedy label scripts and beam matrices, as head outputs
(logits) chosen so that the decode kernels meet the places where they can go wrong.  test_ctc_cases_cpu.py walks them on
the definitions alone (confidence_ref.py) and asserts that every case reaches the branch it is named for;
test_gpu_ctc_decode.py sends them through ocrs_ctc_decode_packed.

The logits are built so that LogSoftmax keeps what matters: equal logits of a row give log-probs equal bit for bit (the
same subtraction), a -inf logit gives a -inf log-prob, no row is entirely -inf and nothing is NaN.  `log_softmax32` is the
float32 stand-in the CPU test uses for the kernel; the GPU tests take the log-probs the hook returns instead."""
import time
import zlib

import numpy as np

import confidence_ref as CR

NEG = np.float32(-np.inf)


# ---------------------------------------------------------------- geometries: line lengths in the caller's order
def _g3():
    """65 lines, T descending from 40 to 1 with plateaus: slot 64, the second wave's only live lane, has T = 1."""
    return [40 - (m * 40) // 65 for m in range(65)]


def _g4():
    """130 lines with T in {15, 16, 17, 31, 32, 33}, shuffled.  Sorted by length (as the plan does) the first wave holds the
    36 lines with T >= 31 next to 28 with T = 17, the second T in {17, 16, 15}, the third two lines and 62 lanes m >= M."""
    t = [33] * 10 + [32] * 12 + [31] * 14 + [17] * 30 + [16] * 30 + [15] * 34
    return [int(v) for v in np.random.default_rng(4).permutation(t)]


GEOMETRIES = {
    "g1": [1],
    "g2": [5, 1],
    "g3": _g3(),
    "g4": _g4(),
    # unsorted, T = 0 lines among them, the longest line last
    "g5": [3, 0, 7, 1, 12, 5, 0, 9, 2, 4, 6, 0, 8, 1, 10, 3, 5, 11, 2, 48],
    # the same shape with fewer rows, for the beam cases whose W * C makes the Python definition slow
    "g5s": [2, 0, 3, 1, 4, 2, 0, 4, 1, 2, 3, 0, 3, 1, 4, 2, 3, 5, 1, 6],
    "lds": [12, 7, 1],
}


def packed_slots(lengths):
    """The plan's line order: lines with T > 0, longest first, stable (HipModel::make_packed_plan)."""
    return sorted((i for i, t in enumerate(lengths) if t > 0), key=lambda i: -lengths[i])


def log_softmax32(z):
    """LogSoftmax in float32, the CPU test's stand-in for the kernel (whose last-place rounding is test_gpu_operators.py's
    subject): m = max, out = v - (m + log(sum exp(v - m)))."""
    z = np.asarray(z, np.float32)
    if z.shape[0] == 0:
        return z.copy()
    with np.errstate(divide="ignore"):
        m = z.max(1, keepdims=True)
        s = np.exp(z - m, dtype=np.float32).sum(1, keepdims=True, dtype=np.float32)
        return (z - (m + np.log(s, dtype=np.float32))).astype(np.float32)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------- greedy label scripts
BOUNDARIES = (16, 32)   # ctc_collapse_scored_packed_kernel walks blocks of 16 steps: t = 15 | 16 and t = 31 | 32


def _random_labels(rng, T, C, avoid=()):
    """A label string with repeats (p = 0.3) and blanks, none of `avoid`."""
    allowed = [c for c in range(C) if c not in avoid]
    out = []
    for t in range(T):
        if t > 0 and rng.random() < 0.3:
            out.append(out[-1])
        else:
            out.append(int(allowed[int(rng.integers(0, len(allowed)))]))
    return out


def _nonblank(i, C, avoid=()):
    allowed = [c for c in range(1, C) if c not in avoid]
    return allowed[i % len(allowed)] if allowed else 0


def blank_mid(i, b):
    """blank_between: where line i's blank sits at boundary b — at b (a | 0 a) for even i, at b - 1 (a 0 | a) for odd i."""
    return b - (i & 1)


def _script_labels(script, i, T, C, rng, avoid=()):
    lab = _random_labels(rng, T, C, avoid)
    a = _nonblank(i, C, avoid)
    if script == "repeat_boundary":       # ... a a | a a ... across both block boundaries
        for b in BOUNDARIES:
            for t in range(b - 2, b + 2):
                if t < T:
                    lab[t] = a
    elif script == "blank_between":       # a 0 a with the blank on either side of the boundary (by line parity)
        for b in BOUNDARIES:
            mid = blank_mid(i, b)
            for t, v in ((mid - 1, a), (mid, 0), (mid + 1, a)):
                if 0 <= t < T:
                    lab[t] = v
        if T >= 3:                         # short lines too
            lab[0], lab[1], lab[2] = a, 0, a
    elif script == "all_blank":
        lab = [0] * T
    elif script == "one_label":
        lab = [a] * T
    elif script == "last_label":
        for t in range(i % 3, T, 3):
            lab[t] = C - 1
    return lab


EXCLUDED = {2: [1], 5: [2, 4], 97: [3, 50, 96]}
GREEDY_SCRIPTS = ("repeat_boundary", "blank_between", "all_blank", "one_label", "last_label", "ties", "excluded_max",
                  "exclusion_tie")
GREEDY_CLASSES = (2, 5, 97)
GREEDY_GEOMETRIES = ("g3", "g4", "g5")


def greedy_logits(script, i, T, C):
    """Line i's head output [T, C] float32 for a script: the arg-max after masking is the scripted string."""
    rng = _rng("greedy", script, i, T, C)
    excl = EXCLUDED[C] if script in ("excluded_max", "exclusion_tie") else ()
    lab = _script_labels(script, i, T, C, rng, excl)
    if script == "excluded_max" and C == 2:
        lab = [0] * T                                   # label 1 is excluded: only the blank is left
    z = rng.normal(0.0, 1.0, (T, C)).astype(np.float32)
    for t in range(T):
        top = np.float32(z[t].max() + np.float32(3.0))
        z[t, lab[t]] = top
        later = [c for c in range(lab[t] + 1, C) if c not in excl]
        if script == "ties" and t % 4 == 1 and later:                     # two equal maxima: the first wins
            z[t, later[0]] = top
        if script == "ties" and t % 4 == 3 and len(later) >= 2:           # three
            z[t, later[0]] = top
            z[t, later[-1]] = top
        if excl and t % 3 != 2:                                           # an excluded label is the raw maximum
            z[t, excl[(t + i) % len(excl)]] = top + np.float32(2.0)
            if script == "exclusion_tie" and later:                       # and masking it leaves two equal maxima
                z[t, later[len(later) // 2]] = top
    return z


class Case:
    """One packed batch: `mats` (one head output per line, caller's order), the excluded labels or None, and for a beam
    case the width."""

    def __init__(self, name, geometry, C, make, excluded=None, width=0, kind=""):
        self.name, self.geometry, self.C, self.excluded, self.width, self.kind = name, geometry, C, excluded, width, kind
        self.lengths = GEOMETRIES[geometry]
        self._make, self._mats = make, None

    @property
    def mats(self):
        if self._mats is None:
            self._mats = [self._make(i, T) for i, T in enumerate(self.lengths)]
        return self._mats

    def __repr__(self):
        return self.name


def greedy_cases():
    out = []
    for script in GREEDY_SCRIPTS:
        for C in GREEDY_CLASSES:
            if script == "exclusion_tie" and C == 2:
                continue                     # nothing is left to tie with once label 1 is excluded
            excl = EXCLUDED[C] if script in ("excluded_max", "exclusion_tie") else None
            for g in GREEDY_GEOMETRIES:
                out.append(Case("%s-C%d-%s" % (script, C, g), g, C,
                                lambda i, T, script=script, C=C: greedy_logits(script, i, T, C), excl, kind=script))
    for g in ("g1", "g2"):                   # the smallest batches
        out.append(Case("last_label-C5-%s" % g, g, 5, lambda i, T: greedy_logits("last_label", i, T, 5), kind="last_label"))
    return out


# ---------------------------------------------------------------- beam matrices
def beam_logits(kind, i, T, C):
    """Line i's head output for a beam case: `sharp` (one label stands out per step, in runs of two steps), `flat`
    (nothing stands out), `quant` (logits rounded to 0.5: exact ties at the pruning threshold), `excl` (sharp or flat
    with -inf columns, and rows where only the blank is finite; run with excluded labels on top)."""
    rng = _rng("beam", kind, i, T, C)
    if kind == "sharp" or (kind == "excl" and i % 2 == 0):
        z = rng.normal(0.0, 1.0, (T, C))
        for t in range(T):
            z[t, (t // 2 + i) % C] += 5.0
    elif kind == "quant":
        z = np.round(rng.normal(0.0, 1.5, (T, C)) * 2.0) / 2.0
    else:
        z = rng.normal(0.0, 0.4, (T, C))
        z[:, 0] -= 1.0
    z = z.astype(np.float32)
    if kind == "excl":
        if C > 3:
            z[:, C - 2] = NEG                    # a class the model never emits
        for t in range(2 - i % 2, T, 5):
            z[t, 1:] = NEG                       # only the blank is finite
    return z


BEAM_EXCLUDED = {2: [1], 3: [2], 5: [3], 20: [1, 7], 97: [3, 50, 96], 119: [2, 118], 128: [2, 127]}
# (C, width, kind): every C in {2, 5, 20, 97, 128} and W in {1, 2, 7, 32, 128}, each kind at small and large W * C.
# W = 128 with C = 128 is not among them: the kernel's LDS (9 W C + 8 C + 140 W + 7232 bytes) would be 173632 bytes, above
# the 160 KB of a CU, and ctc_beam_supported refuses the pair (the engine then searches on the host).  The largest pairs it
# takes stand in: C = 128 at W = 120 (163296 bytes) and W = 128 at C = 119 (163200 bytes).
BEAM_SETS = [(2, 1, "sharp"), (2, 128, "flat"), (2, 7, "quant"), (2, 2, "excl"),
             (5, 2, "sharp"), (5, 7, "quant"), (5, 32, "flat"), (5, 128, "excl"),
             (20, 7, "sharp"), (20, 32, "quant"), (20, 2, "excl"), (20, 128, "flat"),
             (97, 32, "sharp"), (97, 7, "quant"), (97, 128, "flat"), (97, 1, "excl"),
             (128, 7, "sharp"), (128, 120, "quant"), (128, 2, "flat"), (128, 32, "excl")]
# (3, 4, quant): prefixes fall out of the four beams and come back while a beam that extends them has stayed ("revived")
BEAM_G3_SETS = [(20, 7, "sharp"), (5, 7, "quant"), (3, 4, "quant")]
REVIVED_LINES = (0, 6, 12, 18, 31, 37, 38)   # lines of (3, 4, quant) on g3 whose answer depends on merging a revived prefix
# 64 KB < LDS <= 160 KB: the opt-in launch, on three lines
BEAM_LDS_SETS = [(97, 128, "sharp"), (119, 128, "quant"), (128, 120, "quant")]
UNSUPPORTED_PAIRS = [(128, 128), (120, 128), (128, 121)]    # (C, W) just above the limit


def _beam_case(C, W, kind, g):
    return Case("%s-C%d-W%d-%s" % (kind, C, W, g), g, C, lambda i, T: beam_logits(kind, i, T, C),
                BEAM_EXCLUDED[C] if kind == "excl" else None, width=W, kind=kind)


def beam_cases():
    out = []
    for C, W, kind in BEAM_SETS:
        out.append(_beam_case(C, W, kind, "g2"))
        out.append(_beam_case(C, W, kind, "g5" if W * C <= 4096 else "g5s"))
    out += [_beam_case(C, W, kind, "g3") for C, W, kind in BEAM_G3_SETS]
    out += [_beam_case(C, W, kind, "lds") for C, W, kind in BEAM_LDS_SETS]
    out.append(_beam_case(3, 4, "quant", "g5"))
    out.append(_beam_case(5, 7, "quant", "g1"))
    return out


GREEDY_CASES = greedy_cases()
BEAM_CASES = beam_cases()


# ---------------------------------------------------------------- the definitions on a case
def define_greedy(L):
    """confidence_ref.greedy on masked log-probs L, a T = 0 line being empty with score 0."""
    if L.shape[0] == 0:
        return [], np.zeros(0, np.float32), 0.0
    return CR.greedy(L)


def define_beam(L, width, stats=None):
    """confidence_ref.beam_search likewise -> (steps, step log-probs, score)."""
    if L.shape[0] == 0:
        return [], np.zeros(0, np.float32), 0.0
    steps, score = CR.beam_search(L, width, stats)
    return steps, CR.step_logps(L, steps), score


_expected = {}


def expected_on_stand_in(case):
    """(per-line definitions on log_softmax32 of the case's logits, beam stats summed over the lines, seconds the
    definition took), computed once per case."""
    if case.name not in _expected:
        t0 = time.perf_counter()
        stats = {}
        res = []
        for z in case.mats:
            L = CR.masked(log_softmax32(z), case.excluded)
            res.append(define_beam(L, case.width, stats) if case.width else define_greedy(L))
        _expected[case.name] = (res, stats, time.perf_counter() - t0)
    return _expected[case.name]


def revived_matrices():
    """Log-prob matrices (the stand-in's) of single lines on which a prefix is revived and the answer depends on it."""
    g3 = GEOMETRIES["g3"]
    return [("revived-line%d-T%d-C3-w4" % (i, g3[i]), log_softmax32(beam_logits("quant", i, g3[i], 3)), 4) for i in REVIVED_LINES]
