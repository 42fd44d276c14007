#!/usr/bin/env python
"""Cost of page normalisation; writes profiles/normalize_cost.txt.

    python tools/normalize_bench.py [--reps R] [--out FILE]

1. The five passes on a batch of 16 pages of 1024 x 1024 (default parameters), per kernel, from a kernel trace of its own:
   before it opens the GPU itself, the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/normalize_bench.py --only-kernel --reps R
   as a child, which launches nothing but R + 5 batches, and reads the per-launch durations from the trace.  They are set
   beside the bytes each pass must move (4 B read per pixel in passes 1, 3 and 5, 4 B written in pass 5: three reads and one
   write) at the copy rate ocrs_device_measure_peaks reports in this run.
2. OcrEngine.normalize of one 1024 x 1024 page beside get_text on the same page: the median of R calls after 5 warm-up calls,
   host clock around a call that ends in a device synchronise.

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
# kernel -> bytes per pixel it must move
KERNELS = (("norm_tiles_kernel", 4), ("norm_grid_kernel", 0), ("norm_hist_kernel", 4), ("norm_range_kernel", 0), ("norm_map_kernel", 8))


def text_page(seed, h, w):
    """Paper with a tenth of ink under a light that falls off to the left: most pixels of a tile share a bin or two."""
    import numpy as np
    rng = np.random.default_rng(seed)
    g = np.where(rng.random((h, w)) < 0.1, 0.2, 0.85) + 0.02 * (rng.random((h, w)) - 0.5)
    return (g * (0.6 + 0.4 * np.arange(w) / w)[None, :] - 0.5).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalize_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the batch loop, nothing written: what the kernel trace runs")
    a = ap.parse_args()

    # before this process opens the GPU
    trace, how = (None, None) if a.only_kernel else traced(__file__, [], a.reps, [k[0] for k in KERNELS], "normalize_prof_")

    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, models, synth
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    batch = [eng.input_from_grey(text_page(i, SIDE, SIDE)) for i in range(BATCH)]
    med, best = timed(lambda: eng.normalize_batch(batch), a.reps)
    if a.only_kernel:
        print("normalize_batch of %d pages of %d x %d: %.3f ms median, %.3f ms min" % (BATCH, SIDE, SIDE, med, best))
        return
    _, copy_gbps = _lib.measure_peaks()
    pixels = BATCH * SIDE * SIDE
    total_mb = 16.0 * pixels / 1e6
    out = ["Cost of page normalisation (DESIGN.md 7.4).  Written by tools/normalize_bench.py --reps %d on one MI355X; every figure" % a.reps,
           "below is MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of",
           "the calls, host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, "",
           "A batch of %d pages of %d x %d (paper with a tenth of ink under uneven light), default parameters (tile 64, auto," % (BATCH, SIDE, SIDE),
           "flatten, levels), one call.  The passes must move three reads and one write of 4 B per pixel: %.0f MB, %.1f us at" % (total_mb, total_mb / copy_gbps * 1e3),
           "the copy rate."]
    if trace is None:
        out.append("Per-kernel times: NOT MEASURED (%s)." % how)
    else:
        out.append("Per kernel, from a kernel trace of its own (%d launches each):" % len(trace[KERNELS[0][0]]))
        out.append("    " + how)
        total = 0.0
        for name, bpp in KERNELS:
            us = trace[name]
            m = statistics.median(us)
            total += m
            mb = bpp * pixels / 1e6
            line = "%-18s %8.1f us median, %8.1f min, %8.1f max" % (name, m, us[0], us[-1])
            if bpp:
                line += "; %5.0f MB = %5.0f GB/s at the median (%.0f %% of the copy rate; %.1f us at that rate)" % (
                    mb, mb / m * 1e3, 100 * mb / m * 1e3 / copy_gbps, mb / copy_gbps * 1e3)
            else:
                line += "; one block per page"
            out.append(line)
        out.append("sum of the medians: %.1f us = %.1f x the time of the bytes at the copy rate." % (total, total / (total_mb / copy_gbps * 1e3)))
        out.append("The %d MB of source pages are read again in every pass and repetition and fit the 256 MB last-level cache, so these" % (4 * pixels // 1000000))
        out.append("are no HBM figures; a cold figure was NOT MEASURED.")
    out.append("normalize_batch of the %d pages, host clock: %.3f ms median, %.3f ms min (%d result buffers from the pool, one upload," % (BATCH, med, best, BATCH))
    out.append("one memset, five launches, one download, one wait).")
    out.append("")
    px = synth.synthetic_page(0, SIDE, SIDE, lines=80)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    for name, call in (("normalize (default parameters)", lambda: eng.normalize(inp)), ("normalize(info=True)", lambda: eng.normalize(inp, info=True)),
                       ("get_text", lambda: eng.get_text(inp)), ("get_text(normalize=True)", lambda: eng.get_text(inp, normalize=True))):
        m, b = timed(call, a.reps)
        out.append("one page of %d x %d (the benchmark's page), %-32s %7.3f ms median (%7.3f min)" % (SIDE, SIDE, name + ":", m, b))
    out += ["",
            "What a detector gains from a normalised page is UNCALIBRATED here: the word counts of DESIGN.md 7.4 are those of the",
            "synthetic detection files, which were not trained on text.",
            "NOT MEASURED by this run: a cold-cache rate, pages larger than the last-level cache, tiles other than 64, bench.py",
            "against the parent commit (the plain path launches the parent's kernels from code objects that did not change).",
            "Static (cross-compiled for gfx950; VGPRs / SGPRs / LDS bytes; no scratch, no spills, occupancy 8 waves per SIMD each):",
            "norm_tiles_kernel 15 / 36 / 4144, norm_grid_kernel 18 / 42 / 40, norm_hist_kernel 34 / 47 / 4096, norm_range_kernel",
            "16 / 20 / 40, norm_map_kernel 33 / 52 / 0."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
