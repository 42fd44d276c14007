"""Seeded synthetic model files shared by tests, smoke() and bench.py.

Real ocrs weights are not obtainable offline; the files made
here are the [UNVERIFIED-RECALL] architectures of SURVEY.md §2.4 with seeded
weights.  The recognition head is calibrated with the ORACLE's exact executor so
the file is identical on every machine.  Cached under $OCRS_AMD_CACHE (default
/tmp/ocrs_amd_cache)."""
import hashlib
import os

import numpy as np

from ocrs_amd import modelfile as mf
from ocrs_amd import synth

CACHE = os.environ.get("OCRS_AMD_CACHE", "/tmp/ocrs_amd_cache")


def _cached(name, make):
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, name)
    if os.path.exists(path):
        with open(path, "rb") as f:
            return f.read()
    buf = make()
    tmp = path + ".%d.tmp" % os.getpid()
    with open(tmp, "wb") as f:
        f.write(buf)
    os.replace(tmp, path)
    return buf


def detection_model_bytes(in_hw=(800, 600), depths=(8, 16, 32, 32, 64, 128, 256), seed=1, ink=None):
    """ink = (ink_level, ink_gain, ink_sign) of modelfile.build_detection; None = the default file."""
    key = "det_%dx%d_%s_s%d_v1.ocrsm" % (in_hw[0], in_hw[1], "-".join(map(str, depths)), seed)
    if ink is None:
        return _cached(key, lambda: mf.build_detection(in_hw=in_hw, depths=depths, seed=seed).to_bytes())
    lvl, gain, sign = float(ink[0]), float(ink[1]), int(ink[2])
    key = key.replace("_v1.ocrsm", "_ink%g_%g_%d_v1.ocrsm" % (lvl, gain, sign))
    return _cached(key, lambda: mf.build_detection(in_hw=in_hw, depths=depths, seed=seed, ink_level=lvl, ink_gain=gain,
                                                   ink_sign=sign).to_bytes())


def recognition_model_bytes(seed=2, n_classes=97):
    def make():
        from oracle.nn import OracleGraph
        g = mf.build_recognition(n_classes=n_classes, seed=seed)
        cal = synth.synthetic_line_crops(7, n=8)
        xp = np.full((8, 1, 64, 300), -0.5, np.float32)
        xp[:, 0, :, :256] = cal
        g = mf.calibrate_recognition_head(g, lambda buf, x: OracleGraph(buf).run_exact(x), xp)
        return g.to_bytes()

    return _cached("rec_c%d_s%d_v1.ocrsm" % (n_classes, seed), make)


def digest(buf):
    return hashlib.sha256(buf).hexdigest()[:16]


def oracle_line_logits(rbuf, ora, oin, lines):
    """The oracle's recognition log-probs per line, [T_i, C] float32 each, in input order: what
    oracle/pipeline.py:TextRecognizer.recognize_text_lines feeds the model, with the output kept instead of decoded.

    `ora` is the oracle OcrEngine whose recognizer gives the input height and line geometry, `oin` its prepared page,
    `lines` one list of word rects per line (oracle RotatedRects or [k, 6] arrays of the engine's layout).  Each line
    is drawn into a BLACK_VALUE row of its width group (resized width rounded up to a multiple of 50) and every group
    runs through OracleGraph(rbuf).run_exact.  Rows are independent in the oracle, so any subset of a request's lines
    gives the bits the whole request would.  A line of resized width 0 gets (0, C), as the engine returns it."""
    from oracle import clib
    from oracle import pipeline as OP
    from oracle.geometry import RotatedRect
    from oracle.nn import OP_LINEAR, OracleGraph

    graph = OracleGraph(rbuf)
    n_cls = [op["cout"] for op in graph.ops if op["type"] == OP_LINEAR][-1]
    rec = ora.recognizer
    h = rec.input_height()
    page = np.asarray(oin)[0]
    groups = {}
    for i, line in enumerate(lines):
        words = [w if isinstance(w, RotatedRect) else RotatedRect.from_array(np.asarray(w, np.float32))
                 for w in line]
        poly, rw = rec._line_geometry(words)
        groups.setdefault(-(-rw // 50) * 50, []).append((i, poly, rw))
    out = [None] * len(lines)
    for gw, members in groups.items():
        if gw == 0:
            for i, _, _ in members:
                out[i] = np.zeros((0, n_cls), np.float32)
            continue
        step = max(1, (1 << 20) // (h * gw))   # the oracle keeps every slot: bound its activations to ~0.3 GB
        for c0 in range(0, len(members), step):
            chunk = members[c0:c0 + step]
            batch = np.full((len(chunk), 1, h, gw), OP.BLACK_VALUE, np.float32)
            for bi, (_, poly, rw) in enumerate(chunk):
                clib.prepare_text_line_into(page, [(p[1], p[0]) for p in poly], rw, h, batch[bi, 0])
            y = graph.run_exact(batch)   # [T, N, C]
            for bi, (i, _, _) in enumerate(chunk):
                out[i] = np.ascontiguousarray(y[:, bi])
    return out


def small_recognition_bytes(hidden=64, in_h=64, seed=33, chans=(32, 64, 64, 64, 64, 64)):
    """A recognition model of another hidden size or input height, its head calibrated as the production file's is
    (the GPU tests' small engines: hidden 32 runs two launches per GRU step, 64 and 128 the persistent kernel)."""
    from oracle.nn import OracleGraph
    g = mf.build_recognition(n_classes=97, in_h=in_h, seed=seed, hidden=hidden, chans=chans)
    cal = synth.synthetic_line_crops(9, n=8)[:, ::64 // in_h, ::64 // in_h]
    xp = np.full((8, 1, in_h, 300), -0.5, np.float32)
    xp[:, 0, :, :cal.shape[2]] = cal
    return mf.calibrate_recognition_head(g, lambda buf, x: OracleGraph(buf).run_torch(x), xp).to_bytes()


def assert_logits_equal(got, exp, what=""):
    """Per line log-probs equal bit for bit (NaN positions included); the message names the line, step and class."""
    assert len(got) == len(exp), "%s: %d lines of log-probs, oracle %d" % (what, len(got), len(exp))
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape, "%s: line %d: shape %s, oracle %s" % (what, i, g.shape, e.shape)
        if not np.array_equal(g, e, equal_nan=True):
            bad = ~((g == e) | (np.isnan(g) & np.isnan(e)))
            t, c = np.argwhere(bad)[0]
            raise AssertionError("%s: line %d (T %d): %d of %d log-probs differ; first at step %d class %d: got %r, "
                                 "oracle %r" % (what, i, e.shape[0], bad.sum(), bad.size, t, c, g[t, c], e[t, c]))
