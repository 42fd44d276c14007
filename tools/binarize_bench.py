#!/usr/bin/env python
"""Cost of adaptive binarisation; writes profiles/binarize_cost.txt.

    python tools/binarize_bench.py [--reps R] [--out FILE]

1. The three passes on a batch of 16 shaded text pages of 1024 x 1024, at radius 15 and again at radius 127, per kernel, each
   from a kernel trace of its own: before it opens the GPU itself, the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/binarize_bench.py --only-kernel --radius N --reps R
   as a child, which launches nothing but R + 5 batches, and reads the per-launch durations from the trace (no counters in
   that run).  The medians are set beside the copy rate ocrs_device_measure_peaks reports in this run and beside the time one
   read and one write of the float pages (8 B per pixel) take at that rate.
2. OcrEngine.binarize of one 1024 x 1024 page and get_text(binarize=True) beside get_text on the same page: the median of R
   calls after 5 warm-up calls, host clock around a call that ends in a device synchronise.

No threshold gates anything here; the file says which figures were measured.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_util import timed, traced   # tools/, beside this file

BATCH, SIDE = 16, 1024
RADII = (15, 127)
# kernel -> (bytes per pixel it reads, bytes per pixel it writes), but for the records of the window's run-in
KERNELS = (("bin_rows_kernel", 4, 8), ("bin_cols_kernel", 12, 4), ("bin_info_kernel", 0, 0))
WHAT = {"bin_rows_kernel": "the page read once, 8 B of row sums written per pixel",
        "bin_cols_kernel": "two records of row sums (16 B) and the page (4 B) read per pixel, and the run-in of every segment; the page written",
        "bin_info_kernel": "one block per page"}


def shaded_page(seed, side):
    """A synthetic text page as a prepared page under the shade of DESIGN.md §7.10: an illumination that falls from 1 at the
    left edge to 0.3 at the right one, and a dark blotch (a Gaussian dip of 0.8, 40 pixels wide)."""
    import numpy as np
    from ocrs_amd import synth
    px = synth.synthetic_page(seed, side, side, 80, 2, 1)
    grey = px.reshape(side, side).astype(np.float64) / 255.0
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    light = 1.0 - 0.7 * xx / (side - 1)
    light = light * (1.0 - 0.8 * np.exp(-((yy - 0.55 * side) ** 2 + (xx - 0.35 * side) ** 2) / (2.0 * 40.0 * 40.0)))
    return (grey * light - 0.5).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binarize_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the batch loop, nothing written: what the kernel trace runs")
    ap.add_argument("--radius", type=int, default=15, help="with --only-kernel: the radius of the batch")
    a = ap.parse_args()

    # before this process opens the GPU
    traces = [] if a.only_kernel else [(r,) + traced(__file__, ["--radius", str(r)], a.reps, [k[0] for k in KERNELS], "binarize_prof_")
                                       for r in RADII]

    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, models, synth
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    batch = [eng.input_from_grey(shaded_page(i, SIDE)) for i in range(BATCH)]
    if a.only_kernel:
        med, best = timed(lambda: eng.binarize_batch(batch, {"radius": a.radius}), a.reps)
        print("binarize_batch of %d pages of %d x %d, radius %d: %.3f ms median, %.3f ms min" % (BATCH, SIDE, SIDE, a.radius, med, best))
        return
    _, copy_gbps = _lib.measure_peaks()
    pixels = BATCH * SIDE * SIDE
    total_mb = 8.0 * pixels / 1e6
    copy_us = total_mb / copy_gbps * 1e3
    out = ["Cost of adaptive binarisation (DESIGN.md 7.10).  Written by tools/binarize_bench.py --reps %d on one MI355X; every figure" % a.reps,
           "below is MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of",
           "the calls, host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, "",
           "A batch of %d pages of %d x %d (synthetic text under a falling illumination and a dark blotch), one call, k = 0.34.  One" % (BATCH, SIDE, SIDE),
           "read and one write of the float pages are 8 B per pixel: %.0f MB, %.1f us at the copy rate.  The passes move more than" % (total_mb, copy_us),
           "that: pass 1 reads the page (4 B) and writes the row sums (8 B); pass 2 reads two records of row sums per pixel (16 B),",
           "the records of every segment's run-in (2 r + 1 rows of 8 B per segment; the segment lengths are given below), and",
           "the page again (4 B), and writes the page (4 B)."]
    for r, trace, how in traces:
        _, infos = eng.binarize_batch(batch, {"radius": r}, info=True)
        med, best = timed(lambda: eng.binarize_batch(batch, {"radius": r}), a.reps)
        seg = (2 * r + 1 + 31) // 32 * 32   # bin_seg_rows of kernels_binarize.hip
        while seg > 32 and ((SIDE + 255) // 256) * ((SIDE + seg - 1) // seg) < 64:
            seg //= 2
        seg = min(seg, SIDE)
        out.append("")
        out.append("radius %d (segments of %d rows: %d blocks of pass 2, %d of pass 1): %d pixels of ink of %d counted." % (
            r, seg, BATCH * ((SIDE + 255) // 256) * ((SIDE + seg - 1) // seg), BATCH * ((SIDE + 3) // 4), sum(i["ink"] for i in infos),
            sum(i["counted"] for i in infos)))
        if trace is None:
            out.append("Per-kernel times: NOT MEASURED (%s)." % how)
        else:
            out.append("Per kernel, from a kernel trace of its own (%d launches each):" % len(trace[KERNELS[0][0]]))
            out.append("    " + how)
            total = 0.0
            for name, rd, wr in KERNELS:
                us = trace[name]
                m = statistics.median(us)
                total += m
                mb = (rd + wr) * pixels / 1e6
                line = "%-16s %8.1f us median, %8.1f min, %8.1f max" % (name, m, us[0], us[-1])
                if mb:
                    line += "; %3.0f MB without the run-in = %5.0f GB/s at the median (%.1f us at the copy rate)" % (mb, mb / m * 1e3, mb / copy_gbps * 1e3)
                out.append(line + "; " + WHAT[name])
            out.append("sum of the medians: %.1f us = %.1f x the time of one read and one write of the pages at the copy rate (reported," % (
                total, total / copy_us))
            out.append("not required).")
        out.append("binarize_batch of the %d pages, host clock: %.3f ms median, %.3f ms min (%d result buffers and %d workspace" % (
            BATCH, med, best, BATCH, BATCH + 3))
        out.append("buffers from the pool, one upload, three launches, one wait).")
    out.append("")
    out.append("The %d MB of source pages and the %d MB of row sums are touched again in every repetition and fit the 256 MB" % (
        4 * pixels // 1000000, 8 * pixels // 1000000))
    out.append("last-level cache: they were CACHE-RESIDENT, so these are no HBM figures; a cold figure was NOT MEASURED.")
    out.append("")
    px = synth.synthetic_page(0, SIDE, SIDE, lines=80)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    for name, call in (("binarize (default parameters)", lambda: eng.binarize(inp)),
                       ("binarize(radius=127)", lambda: eng.binarize(inp, radius=127)),
                       ("binarize(mask=True, info=True)", lambda: eng.binarize(inp, mask=True, info=True)),
                       ("get_text", lambda: eng.get_text(inp)), ("get_text(binarize=True)", lambda: eng.get_text(inp, binarize=True))):
        m, b = timed(call, a.reps)
        out.append("one page of %d x %d (the benchmark's page), %-36s %7.3f ms median (%7.3f min)" % (SIDE, SIDE, name + ":", m, b))
    out += ["",
            "Workspace per page pixel: 8 B of row sums; 1 B more for the byte mask when it is asked for; per block of pass 2 a record",
            "of 64 B of counts.",
            "What a detector or a recogniser gains from a binarised page is UNCALIBRATED here: the synthetic model files were not",
            "trained on text.",
            "NOT MEASURED by this run: a cold-cache rate, pages larger than the last-level cache, radii other than the two above,",
            "pages so small or so narrow that most lanes of a strip are off the page, sums kept in LDS across both passes (not built).",
            "Static (cross-compiled for gfx950; VGPRs / SGPRs / LDS bytes; no scratch, no spills): bin_rows_kernel 27 / 29 / 24576",
            "(6 waves per SIMD, by its LDS), bin_cols_kernel 36 / 57 / 0, bin_info_kernel 24 / 17 / 64 (8 waves per SIMD)."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
