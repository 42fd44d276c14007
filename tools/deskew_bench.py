#!/usr/bin/env python
"""Cost of page deskew; writes profiles/deskew_cost.txt.

    python tools/deskew_bench.py [--reps R] [--out FILE]

1. The score kernels (the 61 coarse angles of the default search) and the warp (3 degrees, expanded) on a page of
   1024 x 1024 and on one of 3000 x 2200 (height x width), per kernel, from a kernel trace of its own: before it opens the
   GPU itself, the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/deskew_bench.py --only-kernel --reps R
   as a child, which launches nothing but R + 5 calls of each per page, and reads the per-launch durations from the trace.
   The score kernel is set beside the bytes it must read once (4 B per pixel) at the copy rate
   ocrs_device_measure_peaks reports in this run; the warp beside 4 B read + 4 B written per output pixel.
2. estimate_skew, skew_scores, warp and deskew beside detect_words of the same page: the median of R calls after 5 warm-up
   calls, host clock around a call that ends in a device synchronise.

No threshold gates anything here; the file says which figures were measured.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_util import last_launches, timed, traced   # tools/, beside this file

SIZES = ((1024, 1024, 80), (3000, 2200, 200))   # height, width, text lines
KERNELS = ("skew_profiles_kernel", "skew_scores_kernel", "warp_pages_kernel")
ANGLE = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deskew_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the kernel loops, nothing written: what the kernel trace runs")
    a = ap.parse_args()

    # before this process opens the GPU; making the skewed pages launches the warp before the loops
    trace, how = (None, None) if a.only_kernel else traced(__file__, [], a.reps, KERNELS, "deskew_prof_",
                                                           last_launches(KERNELS, len(SIZES) * (a.reps + 5)))

    import ocrs_amd
    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, models, synth
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    import numpy as np
    coarse = np.concatenate([ocrs_amd.skew_table(5 * k, 1, 0.1) for k in range(-30, 31)])
    pages = []
    for h, w, lines in SIZES:   # a text page, skewed by the library's own warp so that the estimate has something to find
        px = synth.synthetic_page(0, h, w, lines=lines)
        straight = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
        pages.append(eng.warp(straight, ocrs_amd.deskew_map((h, w), -ANGLE, expand=False)[1], (h, w), fill=0.5))
    maps = [ocrs_amd.deskew_map((h, w), ANGLE) for h, w, _ in SIZES]
    if a.only_kernel:
        for page, (out_hw, m) in zip(pages, maps):
            for _ in range(a.reps + 5):
                eng.skew_scores([page], coarse)
                eng.warp(page, m, out_hw)
        return
    _, copy_gbps = _lib.measure_peaks()
    out = ["Cost of page deskew (DESIGN.md 7.6).  Written by tools/deskew_bench.py --reps %d on one MI355X; every figure below is" % a.reps,
           "MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of the calls,",
           "host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, "",
           "Pages: the benchmark's synthetic text page at each size, skewed by %g degrees.  Scores: the 61 coarse angles of the" % ANGLE,
           "default search, one call.  Warp: deskew_map(%g degrees, expanded), one call." % ANGLE]
    if trace is None:
        out.append("Per-kernel times: NOT MEASURED (%s)." % how)
    else:
        out.append("Per kernel, from a kernel trace of its own (%d launches per page and kernel, the first 5 dropped):" % (a.reps + 5))
        out.append("    " + how)
        n = a.reps + 5
        for i, ((h, w, _), (out_hw, _m)) in enumerate(zip(SIZES, maps)):
            out.append("page of %d x %d:" % (h, w))
            for name in KERNELS:
                us = sorted(trace[name][i * n + 5:(i + 1) * n])
                med = statistics.median(us)
                line = "  %-21s %8.1f us median, %8.1f min, %8.1f max" % (name, med, us[0], us[-1])
                if name == "skew_profiles_kernel":
                    mb = 4.0 * h * w / 1e6
                    line += "; the page read once is %.1f MB = %.1f us at the copy rate: %.1f x that; %.2f us per angle" % (
                        mb, mb / copy_gbps * 1e3, med / (mb / copy_gbps * 1e3), med / len(coarse))
                elif name == "warp_pages_kernel":
                    mb = 8.0 * out_hw[0] * out_hw[1] / 1e6
                    line += "; %d x %d out, 4 B read + 4 B written per output pixel = %.1f MB = %.0f GB/s (%.0f %% of the copy rate)" % (
                        out_hw[0], out_hw[1], mb, mb / med * 1e3, 100 * mb / med * 1e3 / copy_gbps)
                else:
                    line += "; one block per angle"
                out.append(line)
        out.append("The pages fit the 256 MB last-level cache and are read again in every repetition, so these are no HBM figures; a cold")
        out.append("figure was NOT MEASURED.")
    out.append("")
    for (h, w, _), page, (out_hw, m) in zip(SIZES, pages, maps):
        for name, call in (("estimate_skew", lambda: eng.estimate_skew(page)), ("skew_scores (61 angles)", lambda: eng.skew_scores([page], coarse)),
                           ("warp", lambda: eng.warp(page, m, out_hw)), ("deskew (estimate + warp)", lambda: eng.deskew(page)),
                           ("detect_words", lambda: eng.detect_words(page))):
            med, best = timed(call, a.reps)
            out.append("one page of %d x %d, %-26s %7.3f ms median (%7.3f min)" % (h, w, name + ":", med, best))
        sk = eng.estimate_skew(page)
        out.append("    (estimate_skew found %.1f degrees on a work page of %d x %d; best / runner-up coarse score %.2f)" % (
            sk.angle, sk.work_hw[0], sk.work_hw[1], sk.scores[0] / max(sk.scores[1], 1)))
    out += ["",
            "NOT MEASURED by this run: the rate of LDS atomics for this access pattern on its own (the profile kernel's time holds",
            "it together with the loads and the flush); the cost of the warp's gathers against a staged (LDS) variant, which was not",
            "built; a row-wise walk of the histogram, which was not built (DESIGN.md 7.6 says why the column-wise one was chosen); a",
            "cold-cache rate; bench.py against the parent commit (the plain path launches the parent's kernels from code objects that",
            "did not change).",
            "Static (cross-compiled for gfx950; VGPRs / SGPRs / LDS bytes; no scratch, no spills, occupancy 8 waves per SIMD each):",
            "skew_profiles_kernel 25 / 62 / 17696, skew_scores_kernel 9 / 22 / 32, warp_pages_kernel 37 / 52 / 0."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
