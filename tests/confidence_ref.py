"""Recognition confidence restated in Python (DESIGN.md "Recognition confidence"): what the engine's scored entry points
must return, computed from a line's log-probs L [T, C] after the reference's -inf masking (recognition.rs:547-561).

  * step log-prob of a CTC step (label, pos): L[pos][label], the float32 value unchanged;
  * greedy line score: sum over t = 0 .. T-1 of float64(max_c L[t][c]), added in ascending t (0.0 if T = 0);
  * beam line score: the returned best beam's beam_lse(pb, pnb).
"""
import math

import numpy as np

from oracle import pipeline as OP


def masked(logp, excluded):
    """L: the log-probs with the excluded labels (oracle OcrEngine.excluded_char_labels, or None) set to -inf."""
    L = np.array(logp, np.float32, copy=True)
    if excluded is not None:
        L[:, excluded] = -np.inf
    return L


def row_argmax(r):
    """(label, value) of a row's first maximum, as the engine's arg-max walks it: v > best from class 0 up (a NaN never
    wins, a NaN in class 0 is kept)."""
    if not np.isnan(r).any():
        j = int(np.argmax(r))
        return j, r[j]
    best, bv = 0, r[0]
    for j in range(1, len(r)):
        if r[j] > bv:
            best, bv = j, r[j]
    return best, bv


def greedy(L):
    """rten decode_greedy on L -> (steps [(label, pos)], step log-probs float32, line score float64)."""
    steps, last, score = [], 0, 0.0
    for t in range(L.shape[0]):
        lab, v = row_argmax(L[t])
        score += float(v)
        if lab != last and lab > 0:
            steps.append((lab, t))
        last = lab
    return steps, step_logps(L, steps), score


def step_logps(L, steps):
    return np.array([L[p, l] for l, p in steps], np.float32)


BEAM_STATS = ("steps", "threshold_ties", "short", "merges", "parent_later", "parent_earlier", "revived")


def beam_search(L, width, stats=None):
    """oracle/pipeline.py::ctc_beam_search's loop, also returning the best beam's beam_lse(pb, pnb)
    -> (steps [(label, pos)], line score float64).

    stats (optional, a dict): counts, over the time steps (BEAM_STATS), those where the scores at ranks keep - 1 and keep
    are equal (keep = min(width, candidates): a tie at the pruning threshold), where there are fewer candidates than the
    width ("short"), where an extension of a beam is the prefix of a current beam ("merges"), and among those where the
    extended (parent) beam comes later / earlier in the beam order than the beam it merges with; and those where an
    extension is a prefix that is no current beam although a current beam extends it, and both survive the pruning
    ("revived": the prefix fell out of the beams while its child stayed, and is back beside it).  The search itself does
    not look at it."""
    T, C = L.shape
    NEG = -math.inf
    lse = OP.beam_lse
    beams = [((), (), 0.0, NEG)]
    for t in range(T):
        row = [float(v) for v in L[t]]
        order = []
        cand = {}

        def add(labels, positions, pb, pnb):
            e = cand.get(labels)
            if e is None:
                cand[labels] = [positions, pb, pnb]
                order.append(labels)
            else:
                e[1] = lse(e[1], pb)
                e[2] = lse(e[2], pnb)

        index = {b[0]: i for i, b in enumerate(beams)} if stats is not None else None
        orphans = {b[0][:-1] for b in beams if b[0] and b[0][:-1] not in index} if stats is not None else None
        later = earlier = False
        back = set()
        for i, (labels, positions, pb, pnb) in enumerate(beams):
            total = lse(pb, pnb)
            add(labels, positions, total + row[0], NEG)
            last = labels[-1] if labels else -1
            for c in range(1, C):
                lp = row[c]
                if lp == NEG:
                    continue
                if index is not None:
                    j = index.get(labels + (c,))
                    if j is not None:
                        later, earlier = later or i > j, earlier or i < j
                    if labels + (c,) in orphans:
                        back.add(labels + (c,))
                if c == last:
                    add(labels, positions, NEG, pnb + lp)
                    add(labels + (c,), positions + (t,), NEG, pb + lp)
                else:
                    add(labels + (c,), positions + (t,), NEG, total + lp)
        scored = [(lse(cand[k][1], cand[k][2]), i, k) for i, k in enumerate(order)]
        scored.sort(key=lambda x: (-x[0], x[1]))
        if stats is not None:
            keep = min(width, len(scored))
            kept = {k for _, _, k in scored[:keep]}
            revived = any(k in kept and any(b and b[:-1] == k for b in kept) for k in back)
            for name, hit in zip(BEAM_STATS, (True, keep < len(scored) and scored[keep - 1][0] == scored[keep][0],
                                              len(scored) < width, later or earlier, later, earlier, revived)):
                stats[name] = stats.get(name, 0) + int(hit)
        beams = [(k, cand[k][0], cand[k][1], cand[k][2]) for _, _, k in scored[:width]]
    best = beams[0]
    best_score = lse(best[2], best[3])
    for b in beams[1:]:
        sc = lse(b[2], b[3])
        if sc > best_score:
            best, best_score = b, sc
    return [(int(a), int(b)) for a, b in zip(best[0], best[1])], best_score


def bits_equal(a, b):
    """float64 values equal bit for bit (so -0.0 != 0.0 and NaN == NaN of the same payload)."""
    return np.float64(a).tobytes() == np.float64(b).tobytes()
