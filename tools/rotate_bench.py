#!/usr/bin/env python
"""Cost of quarter turns and of the orientation probe; writes profiles/rotate_cost.txt.

    python tools/rotate_bench.py [--reps R] [--out FILE]
    rocprofv3 --kernel-trace --stats -d rotate_prof -- python tools/rotate_bench.py --only-batch --reps 50
                                                           (the kernel's own time: every launch is the 16-page batch)

1. OcrEngine.rotate per page, k = 0 .. 3, at 1024 x 1024 and 2200 x 3000, and rotate_batch of 16 pages of 1024 x 1024
   (k = 0 .. 3 mixed, one launch): the median of R calls after 5 warm-up calls, host clock around a call that ends in a
   device synchronise.  A call is: the new page's buffer from the pool, 40 B of descriptor per page uploaded, one launch,
   one wait, so a single small page is launch-and-wait latency as much as traffic; the batch shows the traffic.  Bytes
   moved are 8 per pixel (4 read, 4 written), held against the copy rate ocrs_device_measure_peaks reports in the same run.
2. detect_orientation(max_lines=8) beside get_text on the same page (bench.py's synthetic page as given and turned by 90
   degrees), the same way.

No threshold gates anything here; the file says which figures were measured.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_util import timed   # tools/, beside this file


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotate_cost.txt"))
    ap.add_argument("--only-batch", action="store_true", help="only the 16-page rotate_batch loop, nothing written: for a kernel trace")
    a = ap.parse_args()

    import numpy as np

    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, models, synth
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    if a.only_batch:
        rng = np.random.default_rng(0)
        pages = [eng.input_from_grey(rng.random((1024, 1024), dtype=np.float32)) for _ in range(16)]
        print("rotate_batch 16 x 1024 x 1024: %.3f ms median, %.3f ms min" % timed(lambda: eng.rotate_batch(pages, [i % 4 for i in range(16)]), a.reps))
        return
    _, copy_gbps = _lib.measure_peaks()
    out = ["Cost of quarter turns and of the orientation probe (DESIGN.md 8.5).  Written by tools/rotate_bench.py --reps %d on one"
           % a.reps,
           "MI355X; every figure below is MEASURED in that run unless its line says otherwise.  Times are the median (and the",
           "minimum) of the calls, host clock around a call that ends in a device synchronise: buffer from the pool, descriptor",
           "upload, one launch, one wait.  Bytes moved: 8 per pixel.  Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s."
           % copy_gbps, ""]
    rng = np.random.default_rng(0)
    for h, w in ((1024, 1024), (2200, 3000)):
        inp = eng.input_from_grey(rng.random((h, w), dtype=np.float32))
        for k in range(4):
            med, best = timed(lambda: eng.rotate(inp, k), a.reps)
            gb = 8.0 * h * w / 1e9
            out.append("rotate %4d x %4d k=%d: %7.3f ms median, %7.3f ms min; %.1f MB moved: %6.0f GB/s at the median, %6.0f at the "
                       "minimum (%.0f %% / %.0f %% of the copy rate)" % (h, w, k, med, best, gb * 1e3, gb / med * 1e3, gb / best * 1e3,
                                                                      100 * gb / med * 1e3 / copy_gbps, 100 * gb / best * 1e3 / copy_gbps))
    pages = [eng.input_from_grey(rng.random((1024, 1024), dtype=np.float32)) for _ in range(16)]
    ks = [i % 4 for i in range(16)]
    med, best = timed(lambda: eng.rotate_batch(pages, ks), a.reps)
    gb = 16 * 8.0 * 1024 * 1024 / 1e9
    out.append("rotate_batch 16 x 1024 x 1024, k = 0 .. 3 mixed, one launch: %.3f ms median, %.3f ms min = %.3f ms per page; %.0f GB/s "
               "at the median (%.0f %% of the copy rate)" % (med, best, med / 16, gb / med * 1e3, 100 * gb / med * 1e3 / copy_gbps))
    out.append("")
    px = synth.synthetic_page(0, 1024, 1024, lines=80)
    for turn in (0, 1):
        inp = eng.prepare_input(ImageSource.from_tensor(np.ascontiguousarray(np.rot90(px, turn)), DimOrder.Hwc))
        text_med, text_min = timed(lambda: eng.get_text(inp), a.reps)
        probe_med, probe_min = timed(lambda: eng.detect_orientation(inp, max_lines=8), a.reps)
        found = eng.detect_orientation(inp, max_lines=8)
        out.append("bench page turned by %3d degrees: get_text %.2f ms median (%.2f min); detect_orientation(max_lines=8) %.2f ms "
                   "median (%.2f min) = %.2f x get_text; found quarter_turns=%d, vote %.0f : %.0f, scores %s over %s chars"
                   % (90 * turn, text_med, text_min, probe_med, probe_min, probe_med / text_med, found.quarter_turns, found.vote[0],
                      found.vote[1], ["%.3f" % s for s in found.scores], found.n_chars.tolist()))
    out += ["",
            "The probe is two or three detections (the page as given, then one batch of the one or two turned candidates), the",
            "turn, and one recognition batch of up to 16 lines; get_text is one detection and a recognition of every line.  The",
            "scores are those of the synthetic recognition model: uncalibrated (DESIGN.md 8.3), so which turn wins here says",
            "nothing about real models.",
            "NOT MEASURED by this tool: the kernel's own time without the call around it (a kernel trace of --only-batch: the",
            "command is in the tool's docstring; figures of such a run are appended below by hand), LDS bank conflicts",
            "(SQ_LDS_BANK_CONFLICT), bench.py against the parent commit (the plain path's kernels and code objects did not change).",
            "Static (cross-compiled for gfx950): rotate_pages_kernel 22 VGPRs, 16 640 B LDS per block, no scratch, no spills,",
            "occupancy 8 waves per SIMD."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
