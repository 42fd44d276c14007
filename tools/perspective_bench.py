#!/usr/bin/env python
"""Cost of perspective correction; writes profiles/perspective_cost.txt.

    python tools/perspective_bench.py [--reps R] [--out FILE]

1. The edge kernels (the 61 angles of the default search, min_step 8) on a photo of 512 x 384 and on the work copy of one
   of 3000 x 2200 (height x width), skew_profiles_kernel on the same pages and angles, and the projective warp of each
   photo onto its sheet, per kernel, from a kernel trace of its own: before it opens the GPU itself, the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perspective_bench.py --only-kernel --reps R
   as a child, which launches nothing but R + 5 calls of each per page, and reads the per-launch durations from the trace.
   The profile kernels are set beside the bytes they must read once (4 B per pixel) at the copy rate
   ocrs_device_measure_peaks reports in this run; the warp beside 4 B read + 4 B written per output pixel.
2. find_outline, edge_peaks, project and straighten beside detect_words of the same photo: the median of R calls after 5
   warm-up calls, host clock around a call that ends in a device synchronise.

No threshold gates anything here; the file says which figures were measured.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_util import last_launches, timed, traced

SIZES = ((512, 384, 30), (3000, 2200, 200))   # height, width, text lines
KERNELS = ("edge_profiles_kernel", "edge_peaks_kernel", "skew_profiles_kernel", "project_pages_kernel")
QUAD = (0.12, 0.08, 0.88, 0.10, 0.95, 0.93, 0.05, 0.90)   # of the sheet, as fractions of the photo's width and height
DESK = -0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perspective_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the kernel loops, nothing written: what the kernel trace runs")
    a = ap.parse_args()

    # before this process opens the GPU; making the photos launches the warp before the loops
    trace, how = (None, None) if a.only_kernel else traced(__file__, [], a.reps, KERNELS, "perspective_prof_",
                                                           last_launches(KERNELS, len(SIZES) * (a.reps + 5)))

    import numpy as np
    import ocrs_amd
    from perspective_ref import plant_map   # tests/: the map that shows a sheet through a quad
    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, models, synth
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    table = ocrs_amd.skew_table(-30, 61, 0.5)
    photos, works, maps = [], [], []
    for h, w, lines in SIZES:   # a text page seen through a quad on a desk, by the library's own projection
        sheet = eng.prepare_input(ImageSource.from_tensor(synth.synthetic_page(0, h, w, lines=lines), DimOrder.Hwc))
        quad = np.array([v * (w if i % 2 == 0 else h) for i, v in enumerate(QUAD)], np.float32)
        photo = eng.project(sheet, plant_map(quad, (h, w)), (h, w), fill=DESK)
        photos.append(photo)
        work_hw = ocrs_amd.work_size((h, w), max_side=512)
        works.append(photo if work_hw == (h, w) else eng.resize(photo, work_hw, filter="area"))
        maps.append(ocrs_amd.quad_map(quad))
    if a.only_kernel:
        for photo, work, (out_hw, m) in zip(photos, works, maps):
            for _ in range(a.reps + 5):
                eng.edge_peaks([work], table, 8)
                eng.skew_scores([work], table)
                eng.project(photo, m, out_hw)
        return
    _, copy_gbps = _lib.measure_peaks()
    out = ["Cost of perspective correction (DESIGN.md 7.7).  Written by tools/perspective_bench.py --reps %d on one MI355X; every figure" % a.reps,
           "below is MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of",
           "the calls, host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, "",
           "Photos: the benchmark's synthetic text page at each size, seen through a quad on a desk of level %g.  Edge kernels and" % DESK,
           "skew_profiles_kernel: the 61 angles of the default search on the photo's work copy (longer side at most 512), one call.",
           "Projection: quad_map of the planted quad, the full photo onto its sheet, one call."]
    if trace is None:
        out.append("Per-kernel times: NOT MEASURED (%s)." % how)
    else:
        out.append("Per kernel, from a kernel trace of its own (%d launches per photo and kernel, the first 5 dropped):" % (a.reps + 5))
        out.append("    " + how)
        n = a.reps + 5
        for i, ((h, w, _), work, (out_hw, _m)) in enumerate(zip(SIZES, works, maps)):
            wh, ww = work.shape[-2:]
            out.append("photo of %d x %d, work copy %d x %d:" % (h, w, wh, ww))
            for name in KERNELS:
                us = sorted(trace[name][i * n + 5:(i + 1) * n])
                med = statistics.median(us)
                line = "  %-21s %8.1f us median, %8.1f min, %8.1f max" % (name, med, us[0], us[-1])
                if name in ("edge_profiles_kernel", "skew_profiles_kernel"):
                    mb = 4.0 * wh * ww / 1e6
                    line += "; the work copy read once is %.2f MB = %.2f us at the copy rate: %.0f x that; %.2f us per angle" % (
                        mb, mb / copy_gbps * 1e3, med / (mb / copy_gbps * 1e3), med / len(table))
                elif name == "project_pages_kernel":
                    mb = 8.0 * out_hw[0] * out_hw[1] / 1e6
                    line += "; %d x %d out, 4 B read + 4 B written per output pixel = %.1f MB = %.0f GB/s (%.0f %% of the copy rate)" % (
                        out_hw[0], out_hw[1], mb, mb / med * 1e3, 100 * mb / med * 1e3 / copy_gbps)
                else:
                    line += "; one block per (family, sign, angle)"
                out.append(line)
        out.append("The pages fit the 256 MB last-level cache and are read again in every repetition, so these are no HBM figures; a cold")
        out.append("figure was NOT MEASURED.")
    out.append("")
    for (h, w, _), photo, work, (out_hw, m) in zip(SIZES, photos, works, maps):
        for name, call in (("find_outline", lambda: eng.find_outline(photo)), ("edge_peaks (61 angles, work copy)", lambda: eng.edge_peaks([work], table, 8)),
                           ("project", lambda: eng.project(photo, m, out_hw)), ("straighten (outline + project)", lambda: eng.straighten(photo)),
                           ("detect_words", lambda: eng.detect_words(photo))):
            med, best = timed(call, a.reps)
            out.append("one photo of %d x %d, %-34s %7.3f ms median (%7.3f min)" % (h, w, name + ":", med, best))
        o = eng.find_outline(photo)
        quad = np.array([v * (w if i % 2 == 0 else h) for i, v in enumerate(QUAD)], np.float64).reshape(4, 2)
        err = float(np.hypot(*(o.corners.astype(np.float64) - quad).T).max()) if o.found else float("nan")
        out.append("    (find_outline: found %d on a work copy of %d x %d, corners within %.1f pixels of the planted ones, edge pixels %s)" % (
            int(o.found), o.work_hw[0], o.work_hw[1], err, list(o.counts)))
    out += ["",
            "NOT MEASURED by this run: the rate of LDS atomics for this access pattern on its own; a variant that keeps |g| instead of",
            "a count, or one sub-profile for both signs, neither of which was built; the cost of the projection's gathers against a",
            "staged (LDS) variant, which was not built; a cold-cache rate; what find_outline finds on real photographs (none exist",
            "here); bench.py against the parent commit (a request that does not ask for perspective launches the parent's kernels from",
            "code objects that did not change).",
            "Static (cross-compiled for gfx950, -Rpass-analysis=kernel-resource-usage; VGPRs / SGPRs / LDS bytes / waves per SIMD; no",
            "scratch, no VGPR spills, no SGPR spills): edge_profiles_kernel 53 / 36 / 20864 / 7 (its LDS allows 7 blocks of four waves on",
            "a CU), edge_peaks_kernel 19 / 23 / 0 / 8, project_pages_kernel 35 / 56 / 0 / 8."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
