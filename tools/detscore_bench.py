#!/usr/bin/env python
"""Cost of detection confidence: detection-only requests of 8 synthetic 1024x1024 pages, one request at a
time — the form of README's "detection alone" figure — with or without scores.

    python tools/detscore_bench.py [--scores] [--reps N]          one leg: prints ms per 8-page request
    python tools/detscore_bench.py --abab scored [--rounds R]     unscored / scored legs alternating (A B A B ...), this library
    python tools/detscore_bench.py --abab LIB [--rounds R]        unscored on this library (A) against unscored on the
                                                                  library file LIB (B), e.g. a build of the parent commit
    rocprofv3 --kernel-trace --stats -- python tools/detscore_bench.py --scores      per-launch time of component_scores_kernel

Every leg is a fresh child process (OCRS_AMD_LIB picks its library); a leg that fails or overruns ends the run.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(scores, reps):
    import numpy as np

    from ocrs_amd import DimOrder, Model, OcrEngine, _lib, models, synth
    L = _lib.lib()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()))
    inputs = []
    for s in range(8):
        pg = synth.synthetic_page(s, 1024, 1024, lines=80)
        p = C.c_void_p()
        _lib.check(L.ocrs_device_malloc(C.c_size_t(pg.nbytes), C.byref(p)))
        _lib.check(L.ocrs_device_upload(p, pg.ctypes.data_as(C.c_void_p), C.c_size_t(pg.nbytes)))
        inputs.append(eng.prepare_input_device(p.value, np.uint8, DimOrder.Hwc, 1024, 1024, 3))
    call = (lambda: eng.detect_words_batch(inputs, scores=True)) if scores else (lambda: eng.detect_words_batch(inputs))
    for _ in range(5):
        out = call()
    _lib.check(L.ocrs_device_synchronize())
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t0))
    words = out[0] if scores else out
    print(json.dumps({"scores": bool(scores), "reps": reps, "ms_per_request_median": statistics.median(times),
                      "ms_per_request_mean": statistics.fmean(times), "pages_per_s": 8e3 / statistics.fmean(times),
                      "words_page0": len(words[0]), "lib": os.path.basename(_lib.LIB_PATH)}), flush=True)


def abab(other, rounds, reps):
    legs = {"A": ([], None), "B": (["--scores"], None) if other == "scored" else ([], os.path.abspath(other))}
    got = {"A": [], "B": []}
    for r in range(rounds):
        for name in ("A", "B"):
            flags, libpath = legs[name]
            env = dict(os.environ)
            if libpath:
                env["OCRS_AMD_LIB"] = libpath
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(reps)] + flags, env=env,
                               capture_output=True, text=True, timeout=120)
            if p.returncode != 0:
                sys.exit("leg %s of round %d failed (rc %d):\n%s" % (name, r, p.returncode, p.stderr[-2000:]))
            d = json.loads(p.stdout.strip().splitlines()[-1])
            got[name].append(d["ms_per_request_median"])
            print("round %d %s: %.3f ms per request (%s%s)" % (r, name, d["ms_per_request_median"], d["lib"],
                                                             ", scored" if d["scores"] else ""), flush=True)
    a, b = statistics.median(got["A"]), statistics.median(got["B"])
    print(json.dumps({"A_ms": got["A"], "B_ms": got["B"], "A_median_ms": a, "B_median_ms": b, "B_over_A": b / a,
                      "B": "scored" if other == "scored" else os.path.basename(other)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scores", action="store_true")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--abab")
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    if a.abab:
        abab(a.abab, a.rounds, a.reps)
    else:
        leg(a.scores, a.reps)
