#!/usr/bin/env python
"""Cost of ruled-line removal; writes profiles/rules_cost.txt.

    python tools/rules_bench.py [--reps R] [--out FILE]

1. The eight passes on a batch of 16 ruled text pages of 1024 x 1024 (default parameters), per kernel, from a kernel trace of
   its own: before it opens the GPU itself, the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rules_bench.py --only-kernel --reps R
   as a child, which launches nothing but R + 5 batches, and reads the per-launch durations from the trace.  Their sum is set
   beside the bytes the float pages must move (4 B read per pixel in passes 1 and 7, 4 B written in pass 7: two reads and one
   write) at the copy rate ocrs_device_measure_peaks reports in this run.
2. OcrEngine.remove_rules of one 1024 x 1024 page beside get_text on the same page: the median of R calls after 5 warm-up
   calls, host clock around a call that ends in a device synchronise.

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
# kernel -> (how a trace may spell it, bytes of the float page per pixel it must move)
KERNELS = (("rules_mask_kernel", ("rules_mask_kernel",), 4), ("rules_paper_kernel", ("rules_paper_kernel",), 0),
           ("rules_open_kernel<0>", ("rules_open_kernel<0>", "rules_open_kernelILi0E"), 0),
           ("rules_transpose_kernel", ("rules_transpose_kernel",), 0),
           ("rules_open_kernel<1>", ("rules_open_kernel<1>", "rules_open_kernelILi1E"), 0),
           ("rules_sets_kernel", ("rules_sets_kernel",), 0), ("rules_map_kernel", ("rules_map_kernel",), 8),
           ("rules_info_kernel", ("rules_info_kernel",), 0))


def ruled_page(seed, side):
    """A synthetic text page as a prepared page, with a 2-pixel table grid and 1-pixel underlines drawn at -0.5."""
    import numpy as np
    from ocrs_amd import synth
    px = synth.synthetic_page(seed, side, side, 80, 2, 1)
    page = (px.reshape(side, side).astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
    for r in range(8, side - 2, 128):
        page[r:r + 2, 6:side - 6] = -0.5
    for c in (6, side // 2, side - 8):
        page[8:side - 8, c:c + 2] = -0.5
    for r in range(70, side - 2, 97):
        page[r, 40:340] = -0.5
    return page


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rules_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the batch loop, nothing written: what the kernel trace runs")
    a = ap.parse_args()

    # before this process opens the GPU
    trace, how = (None, None) if a.only_kernel else traced(__file__, [], a.reps, [k[:2] for k in KERNELS], "rules_prof_")

    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, models, synth
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    batch = [eng.input_from_grey(ruled_page(i, SIDE)) for i in range(BATCH)]
    med, best = timed(lambda: eng.remove_rules_batch(batch), a.reps)
    if a.only_kernel:
        print("remove_rules_batch of %d pages of %d x %d: %.3f ms median, %.3f ms min" % (BATCH, SIDE, SIDE, med, best))
        return
    _, infos = eng.remove_rules_batch(batch, info=True)
    _, copy_gbps = _lib.measure_peaks()
    pixels = BATCH * SIDE * SIDE
    total_mb = 12.0 * pixels / 1e6
    out = ["Cost of ruled-line removal (DESIGN.md 7.8).  Written by tools/rules_bench.py --reps %d on one MI355X; every figure" % a.reps,
           "below is MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of",
           "the calls, host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, "",
           "A batch of %d pages of %d x %d (synthetic text, a 2-pixel table grid, 1-pixel underlines; %d pixels overwritten" % (
               BATCH, SIDE, SIDE, sum(i["overwritten"] for i in infos)),
           "in all, %d kept at crossings), default parameters (min_length 96, max_thickness 8, margin 1), one call.  The float" % sum(i["kept"] for i in infos),
           "pages must move two reads and one write of 4 B per pixel: %.0f MB, %.1f us at the copy rate; the bit masks between" % (total_mb, total_mb / copy_gbps * 1e3),
           "them are 1/32 of a page each."]
    if trace is None:
        out.append("Per-kernel times: NOT MEASURED (%s)." % how)
    else:
        out.append("Per kernel, from a kernel trace of its own (%d launches each):" % len(trace[KERNELS[0][0]]))
        out.append("    " + how)
        total = 0.0
        for name, _, bpp in KERNELS:
            us = trace[name]
            m = statistics.median(us)
            total += m
            mb = bpp * pixels / 1e6
            line = "%-22s %8.1f us median, %8.1f min, %8.1f max" % (name, m, us[0], us[-1])
            if bpp:
                line += "; %5.0f MB = %5.0f GB/s at the median (%.0f %% of the copy rate; %.1f us at that rate)" % (
                    mb, mb / m * 1e3, 100 * mb / m * 1e3 / copy_gbps, mb / copy_gbps * 1e3)
            else:
                line += "; one block per page" if name in ("rules_paper_kernel", "rules_info_kernel") else "; bit masks only"
            out.append(line)
        out.append("sum of the medians: %.1f us = %.1f x the time of two reads and one write of the pages at the copy rate (reported," % (
            total, total / (total_mb / copy_gbps * 1e3)))
        out.append("not required).")
        out.append("The %d MB of source pages are read again in every repetition and fit the 256 MB last-level cache: the pages were" % (4 * pixels // 1000000))
        out.append("CACHE-RESIDENT, so these are no HBM figures; a cold figure was NOT MEASURED.")
    out.append("remove_rules_batch of the %d pages, host clock: %.3f ms median, %.3f ms min (%d result buffers from the pool, one" % (BATCH, med, best, BATCH))
    out.append("upload, one memset, eight launches, one wait).")
    out.append("")
    px = synth.synthetic_page(0, SIDE, SIDE, lines=80)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    for name, call in (("remove_rules (default parameters)", lambda: eng.remove_rules(inp)),
                       ("remove_rules(mask=True, info=True)", lambda: eng.remove_rules(inp, mask=True, info=True)),
                       ("get_text", lambda: eng.get_text(inp)), ("get_text(rules=True)", lambda: eng.get_text(inp, rules=True))):
        m, b = timed(call, a.reps)
        out.append("one page of %d x %d (the benchmark's page), %-36s %7.3f ms median (%7.3f min)" % (SIDE, SIDE, name + ":", m, b))
    out += ["",
            "What a detector or a recogniser gains from a page without its rules is UNCALIBRATED here: the word counts of DESIGN.md",
            "7.8 are those of the synthetic detection file, which was not trained on text.",
            "NOT MEASURED by this run: a cold-cache rate, pages larger than the last-level cache, parameters other than the default,",
            "bench.py against the parent commit (the plain path launches the parent's kernels from code objects that did not change:",
            "no existing .hip file was edited).",
            "Static (cross-compiled for gfx950; VGPRs / SGPRs / LDS bytes; no scratch, no spills): rules_mask_kernel 32 / 66 / 4608,",
            "rules_paper_kernel 16 / 12 / 40, rules_open_kernel<0> 49 / 91 / 0, rules_transpose_kernel 13 / 32 / 0,",
            "rules_open_kernel<1> 49 / 92 / 0, rules_sets_kernel 70 / 66 / 0 (7 waves per SIMD), rules_map_kernel 40 / 47 / 2048,",
            "rules_info_kernel 42 / 15 / 160; 8 waves per SIMD but for the one named."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
