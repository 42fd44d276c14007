#!/usr/bin/env python
"""Cost of tiled detection: detection-only requests of synthetic pages of one size, one request at a time,
untiled or tiled.

    python tools/tiled_bench.py --size 2048x1536 [--pages N] [--tiled [OVERLAP]] [--reps R]     one leg: one JSON line
    python tools/tiled_bench.py --report [--reps R]          untiled and tiled legs for 1024x1024, 2048x1536 and 3508x2480
    rocprofv3 --kernel-trace --stats -- python tools/tiled_bench.py --size 1024x1024 --pages 8 --tiled     per-launch kernel times

A leg times R requests after 5 warm-up requests (host clock around calls that end in a device synchronise), then repeats a
few requests with the engine's stage timers on, so that the share of the U-Net, of gather / stitch and of the page-resolution
component stage can be read off.  Every leg of --report is a fresh child process; a leg that fails or overruns ends the run.
The untiled detection-only rate against another build of the library (the parent commit's): tools/detscore_bench.py --abab LIB.
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

DET_STAGES = ("resize_to_model", "detection_cnn", "resize_threshold", "ccl", "contour_rects")
REPORT = [((1024, 1024), 8, 80), ((2048, 1536), 4, 150), ((3508, 2480), 2, 200)]   # (page size, pages per request, text lines)


def leg(hw, n_pages, lines, tiled, reps):
    import numpy as np

    from ocrs_amd import DimOrder, Model, OcrEngine, _lib, models, synth, tile_plan
    L = _lib.lib()
    _lib.require_gpu()
    model = Model.load_bytes(models.synthetic_detection_bytes())
    eng = OcrEngine(detection_model=model)
    h, w = hw
    inputs = []
    for s in range(n_pages):
        pg = synth.synthetic_page(s, h, w, lines=lines)
        p = C.c_void_p()
        _lib.check(L.ocrs_device_malloc(C.c_size_t(pg.nbytes), C.byref(p)))
        _lib.check(L.ocrs_device_upload(p, pg.ctypes.data_as(C.c_void_p), C.c_size_t(pg.nbytes)))
        inputs.append(eng.prepare_input_device(p.value, np.uint8, DimOrder.Hwc, h, w, 3))
    call = lambda: eng.detect_words_batch(inputs, tiled=tiled)   # noqa: E731
    for _ in range(5):
        out = call()
    _lib.check(L.ocrs_device_synchronize())
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t0))
    # the stage timers, in a pass of their own (they add events to the stream)
    k = max(3, min(20, reps // 10))
    eng.enable_timing(1)
    eng.stage_times(reset=True)
    for _ in range(k):
        call()
    st = eng.stage_times(reset=True)
    eng.enable_timing(0)
    tiles = 1
    if tiled is not False:
        oy, _, ox, _ = tile_plan(hw, model.input_shape()[2:], None if tiled is True else tiled)
        tiles = len(oy) * len(ox)
    print(json.dumps({"size": "%dx%d" % hw, "pages": n_pages, "tiled": tiled, "tiles_per_page": tiles, "reps": reps,
                      "ms_per_request_median": statistics.median(times), "ms_per_request_mean": statistics.fmean(times),
                      "pages_per_s": n_pages * 1e3 / statistics.median(times), "words_page0": len(out[0]),
                      "stage_ms_per_request": {s: st[s][0] / k for s in DET_STAGES},
                      "stage_launches_per_request": {s: st[s][1] / k for s in DET_STAGES},
                      "lib": os.path.basename(_lib.LIB_PATH)}), flush=True)


def report(reps):
    rows = []
    for hw, n_pages, lines in REPORT:
        for tiled in (False, True):
            cmd = [sys.executable, os.path.abspath(__file__), "--size", "%dx%d" % hw, "--pages", str(n_pages), "--lines", str(lines),
                   "--reps", str(reps)] + (["--tiled"] if tiled else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            if p.returncode != 0:
                sys.exit("leg %s failed (rc %d):\n%s" % (" ".join(cmd[2:]), p.returncode, p.stderr[-2000:]))
            d = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(d), flush=True)
            rows.append(d)
    print("\nsize        pages  tiles/page  untiled pages/s  tiled pages/s  tiled ms/page   tiles x untiled U-Net ms/page   "
          "tiled stages ms/page: gather  U-Net  stitch  ccl  contours")
    for u, t in zip(rows[0::2], rows[1::2]):
        n = t["pages"]
        unet = u["stage_ms_per_request"]["detection_cnn"] / u["pages"]
        s = t["stage_ms_per_request"]
        print("%-10s  %5d  %10d  %15.1f  %13.1f  %13.3f  %29.3f   %27.3f  %5.3f  %6.3f  %3.3f  %8.3f"
              % (t["size"], n, t["tiles_per_page"], u["pages_per_s"], t["pages_per_s"], t["ms_per_request_median"] / n,
                 t["tiles_per_page"] * unet, s["resize_to_model"] / n, s["detection_cnn"] / n, s["resize_threshold"] / n,
                 s["ccl"] / n, s["contour_rects"] / n))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1024x1024", help="page HEIGHTxWIDTH")
    ap.add_argument("--pages", type=int, default=8)
    ap.add_argument("--lines", type=int, default=80)
    ap.add_argument("--tiled", nargs="?", type=int, const=-1, default=None, metavar="OVERLAP")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--report", action="store_true")
    a = ap.parse_args()
    if a.report:
        report(a.reps)
    else:
        leg(tuple(int(x) for x in a.size.split("x")), a.pages, a.lines,
            False if a.tiled is None else True if a.tiled < 0 else a.tiled, a.reps)
