#!/usr/bin/env python
"""Cost of rectified line crops: recognition-only requests of the bench pages' lines (bench.py's synthetic
1024 x 1024 pages, their lines found once by the detector and the layout), one request at a time, plain or rectified.

    python tools/rectify_bench.py [--pages N] [--rectify] [--reps R]      one leg: one JSON line
    python tools/rectify_bench.py --report [--reps R]                     plain and rectified legs, each a fresh process
    python tools/rectify_bench.py --rocprof                               prints the command for the per-kernel times

A leg times R requests after 5 warm-up requests (host clock around calls that end in a device synchronise), then repeats a
few requests with the engine's stage timers on: the "line_crop" stage is the crop launch (crop_lines_kernel or
rectify_lines_kernel) alone.  The leg also reports the output pixels of a request (recognition height x padded width,
summed over its lines) and the device's copy rate (ocrs_device_measure_peaks), to hold the kernel against 4 B written
per output pixel plus one read of the lines' page pixels.  Every leg of --report is a fresh child process; a leg that
fails or overruns ends the run.  The plain path against another build of the library (the parent commit's): an ABAB of
bench.py with OCRS_AMD_LIB naming that build (tools/ab_lib.sh).
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

ROCPROF = ("rocprofv3 --kernel-trace --stats -d rectify_prof -- python tools/rectify_bench.py --mixed --pages 16 --reps 20\n"
           "  (--mixed crops the same lines both ways in every request: crop_lines_kernel and rectify_lines_kernel appear side by\n"
           "   side in the stats, each over `out_pixels` output pixels per launch; divide the average durations by that number)")


def leg(n_pages, lines_per_page, rectify, mixed, reps):
    import numpy as np

    from ocrs_amd import DimOrder, Model, OcrEngine, _lib, line_frame, models, synth
    L = _lib.lib()
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    inputs = []
    for s in range(n_pages):
        pg = synth.synthetic_page(s, 1024, 1024, lines=lines_per_page)
        p = C.c_void_p()
        _lib.check(L.ocrs_device_malloc(C.c_size_t(pg.nbytes), C.byref(p)))
        _lib.check(L.ocrs_device_upload(p, pg.ctypes.data_as(C.c_void_p), C.c_size_t(pg.nbytes)))
        inputs.append(eng.prepare_input_device(p.value, np.uint8, DimOrder.Hwc, 1024, 1024, 3))
    words = eng.detect_words_batch(inputs)
    rects, lo, po = eng.find_text_lines_batch_raw(words)
    n_lines = len(lo) - 1
    rec_h = 64
    if mixed:   # every page twice: once plain, once rectified, through two one-kind requests per timed call
        call = lambda: (eng.recognize_text_batch_raw(inputs, rects, lo, po), eng.recognize_text_batch_raw(inputs, rects, lo, po, rectify=True))   # noqa: E731
    else:
        call = lambda: eng.recognize_text_batch_raw(inputs, rects, lo, po, rectify=rectify)   # noqa: E731
    # output pixels of one request's crop launch
    widths = []
    for i in range(n_lines):
        ws = rects[int(lo[i]):int(lo[i + 1])]
        if rectify or mixed:
            widths.append(-(-line_frame(ws, rec_h).rw // 50) * 50)
    plain_w = [-(-eng.prepare_recognition_input(inputs[0], rects[int(lo[i]):int(lo[i + 1])]).shape[1] // 50) * 50
               for i in range(int(po[0]), int(po[1]))]
    for _ in range(5):
        out = call()
    _lib.check(L.ocrs_device_synchronize())
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t0))
    k = max(3, min(20, reps // 10))
    eng.enable_timing(1)
    eng.stage_times(reset=True)
    for _ in range(k):
        call()
    st = eng.stage_times(reset=True)
    eng.enable_timing(0)
    _, copy_gbps = _lib.measure_peaks()
    chars = out[0][0] if mixed else out[0]
    print(json.dumps({"pages": n_pages, "lines": n_lines, "rectify": bool(rectify), "mixed": bool(mixed), "reps": reps,
                      "ms_per_request_median": statistics.median(times), "ms_per_request_mean": statistics.fmean(times),
                      "pages_per_s": n_pages * 1e3 / statistics.median(times), "chars": int(len(chars)),
                      "out_pixels_rectified": int(rec_h * sum(widths)) if widths else None,
                      "padded_widths_page0_plain_mean": statistics.fmean(plain_w) if plain_w else None,
                      "padded_widths_rectified_mean": statistics.fmean(widths) if widths else None,
                      "stage_ms_per_request": {s: v[0] / k for s, v in st.items() if v[1]},
                      "stage_launches_per_request": {s: v[1] / k for s, v in st.items() if v[1]},
                      "hbm_copy_gbps": copy_gbps, "lib": os.path.basename(_lib.LIB_PATH)}), flush=True)


def report(n_pages, lines, reps):
    rows = []
    for rectify in (False, True):
        cmd = [sys.executable, os.path.abspath(__file__), "--pages", str(n_pages), "--lines", str(lines), "--reps", str(reps)] + \
              (["--rectify"] if rectify else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if p.returncode != 0:
            sys.exit("leg %s failed (rc %d):\n%s" % (" ".join(cmd[2:]), p.returncode, p.stderr[-2000:]))
        d = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(d), flush=True)
        rows.append(d)
    u, r = rows
    px = r["out_pixels_rectified"]
    crop_ms = r["stage_ms_per_request"]["line_crop"]
    print("\nplain:     %.2f ms per request of %d pages / %d lines, line_crop %.3f ms" % (u["ms_per_request_median"], u["pages"], u["lines"],
                                                                                       u["stage_ms_per_request"]["line_crop"]))
    print("rectified: %.2f ms per request, line_crop %.3f ms over %d output pixels = %.3f ns / pixel; 4 B written per pixel at the "
          "copy rate (%.0f GB/s) would be %.3f ms" % (r["ms_per_request_median"], crop_ms, px, 1e6 * crop_ms / px, r["hbm_copy_gbps"],
                                                      4.0 * px / (r["hbm_copy_gbps"] * 1e9) * 1e3))
    print("per-kernel times of both crops on the same lines:\n" + ROCPROF)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--lines", type=int, default=80)
    ap.add_argument("--rectify", action="store_true")
    ap.add_argument("--mixed", action="store_true", help="every timed call makes a plain and a rectified request of the same lines")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--rocprof", action="store_true", help="print the rocprofv3 command and exit")
    a = ap.parse_args()
    if a.rocprof:
        print(ROCPROF)
    elif a.report:
        report(a.pages, a.lines, a.reps)
    else:
        leg(a.pages, a.lines, a.rectify, a.mixed, a.reps)
