#!/usr/bin/env python
"""Cost of despeckling; writes profiles/despeckle_cost.txt.

    python tools/despeckle_bench.py [--reps R] [--out FILE]

1. The eight passes on a batch of 16 noisy text pages of 1024 x 1024, at default parameters and again with keep_near = 2,
   per kernel, each from a kernel trace of its own: before it opens the GPU itself, the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/despeckle_bench.py --only-kernel --keep-near K --reps R
   as a child, which launches nothing but R + 5 batches, and reads the per-launch durations from the trace.  Their sum is set
   beside one read and one write of the float pages (8 B per pixel) at the copy rate ocrs_device_measure_peaks reports in
   this run, and beside the figures of profiles/rules_cost.txt.
2. OcrEngine.despeckle of one 1024 x 1024 page and get_text(despeckle=True) beside get_text on the same page: the median of
   R calls after 5 warm-up calls, host clock around a call that ends in a device synchronise.

No threshold gates anything here; the file says which figures were measured.
"""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_util import timed, traced   # tools/, beside this file

BATCH, SIDE, NOISE = 16, 1024, 0.002
# kernel -> bytes of the float page per pixel it must move
KERNELS = (("speckle_mask_kernel", 4), ("speckle_levels_kernel", 0), ("speckle_merge_kernel", 0), ("speckle_area_kernel", 0),
           ("speckle_big_kernel", 0), ("speckle_near_kernel", 0), ("speckle_map_kernel", 8), ("speckle_info_kernel", 0))
WHAT = {"speckle_mask_kernel": "the page read once; writes the bit mask, 4 B of label, 4 B of area and 1 B of flag per pixel",
        "speckle_levels_kernel": "one block per page", "speckle_merge_kernel": "bit mask in, find / atomicMin unions on the labels",
        "speckle_area_kernel": "a find per run, every label flattened (4 B written per pixel), one atomic add per run, one per wave for its commonest root",
        "speckle_big_kernel": "bit masks; returns at once on a page without keep_near", "speckle_near_kernel": "bit masks; returns at once on a page without keep_near",
        "speckle_info_kernel": "one block per page"}


def noisy_page(seed, side):
    """A synthetic text page as a prepared page, with pepper at -0.5 on 0.2 % of its pixels and then salt at +0.5 on 0.2 %."""
    import numpy as np
    from ocrs_amd import synth
    px = synth.synthetic_page(seed, side, side, 80, 2, 1)
    page = (px.reshape(side, side).astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
    rng = np.random.default_rng(seed)
    page[rng.random(page.shape) < NOISE] = -0.5
    page[rng.random(page.shape) < NOISE] = 0.5
    return page


def rules_total():
    """The sum of the medians profiles/rules_cost.txt records, in us, or None."""
    try:
        with open(os.path.join(ROOT, "profiles", "rules_cost.txt"), encoding="utf-8") as f:
            m = re.search(r"sum of the medians: ([0-9.]+) us", f.read())
        return float(m.group(1)) if m else None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "despeckle_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the batch loop, nothing written: what the kernel trace runs")
    ap.add_argument("--keep-near", type=int, default=0, help="with --only-kernel: the keep_near of the batch")
    a = ap.parse_args()

    # before this process opens the GPU
    traces = [] if a.only_kernel else [(K,) + traced(__file__, ["--keep-near", str(K)], a.reps, [k[0] for k in KERNELS], "despeckle_prof_")
                                       for K in (0, 2)]

    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, models, synth
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    batch = [eng.input_from_grey(noisy_page(i, SIDE)) for i in range(BATCH)]
    if a.only_kernel:
        med, best = timed(lambda: eng.despeckle_batch(batch, {"keep_near": a.keep_near}), a.reps)
        print("despeckle_batch of %d pages of %d x %d, keep_near %d: %.3f ms median, %.3f ms min" % (BATCH, SIDE, SIDE, a.keep_near, med, best))
        return
    _, copy_gbps = _lib.measure_peaks()
    pixels = BATCH * SIDE * SIDE
    total_mb = 8.0 * pixels / 1e6
    copy_us = total_mb / copy_gbps * 1e3
    rules_us = rules_total()
    out = ["Cost of despeckling (DESIGN.md 7.9).  Written by tools/despeckle_bench.py --reps %d on one MI355X; every figure" % a.reps,
           "below is MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of",
           "the calls, host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, "",
           "A batch of %d pages of %d x %d (synthetic text with pepper on %.1f %% and salt on %.1f %% of the pixels), one call.  One" % (
               BATCH, SIDE, SIDE, 100 * NOISE, 100 * NOISE),
           "read and one write of the float pages are 8 B per pixel: %.0f MB, %.1f us at the copy rate.  The passes move more than" % (total_mb, copy_us),
           "that: the page is read twice and written once (12 B), the labels are written, read and rewritten, and read again",
           "(16 B), the areas are zeroed (4 B) and gathered, the flags zeroed (1 B); the three bit masks are 1/32 of a page each.",
           "The labelling is the FLAT one (unions in global memory, as ccl_merge_kernel); the 64 x 64 tile version with unions in",
           "LDS first was NOT BUILT and NOT TIMED."]
    for K, trace, how in traces:
        _, infos = eng.despeckle_batch(batch, {"keep_near": K}, info=True)
        med, best = timed(lambda: eng.despeckle_batch(batch, {"keep_near": K}), a.reps)
        out.append("")
        out.append("max_area 4, max_hole 0, keep_near %d: %d specks of %d pixels removed, %d candidates kept, of %d pixels of ink in all." % (
            K, sum(i["specks"] for i in infos), sum(i["speck_pixels"] for i in infos), sum(i["kept"] for i in infos), sum(i["ink"] for i in infos)))
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
                line = "%-22s %8.1f us median, %8.1f min, %8.1f max" % (name, m, us[0], us[-1])
                if bpp:
                    line += "; %3.0f MB of float pages = %5.0f GB/s at the median (%.1f us at the copy rate)" % (mb, mb / m * 1e3, mb / copy_gbps * 1e3)
                if name in WHAT:
                    line += "; " + WHAT[name]
                out.append(line)
            out.append("sum of the medians: %.1f us = %.1f x the time of one read and one write of the pages at the copy rate (reported," % (
                total, total / copy_us))
            out.append("not required)%s." % ("" if rules_us is None else "; %.2f x the %.1f us profiles/rules_cost.txt records for the eight passes of rule removal on a batch of the same size" % (
                total / rules_us, rules_us)))
        out.append("despeckle_batch of the %d pages, host clock: %.3f ms median, %.3f ms min (%d result buffers and %d workspace" % (
            BATCH, med, best, BATCH, 3 * BATCH + 4))
        out.append("buffers from the pool, one upload, one memset, eight launches, one wait).")
    out.append("")
    out.append("The %d MB of source pages and the %d MB of labels, areas and flags are touched again in every repetition and fit the" % (
        4 * pixels // 1000000, 9 * pixels // 1000000))
    out.append("256 MB last-level cache: they were CACHE-RESIDENT, so these are no HBM figures; a cold figure was NOT MEASURED.")
    out.append("")
    px = synth.synthetic_page(0, SIDE, SIDE, lines=80)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    for name, call in (("despeckle (default parameters)", lambda: eng.despeckle(inp)),
                       ("despeckle(keep_near=2)", lambda: eng.despeckle(inp, keep_near=2)),
                       ("despeckle(mask=True, info=True)", lambda: eng.despeckle(inp, mask=True, info=True)),
                       ("get_text", lambda: eng.get_text(inp)), ("get_text(despeckle=True)", lambda: eng.get_text(inp, despeckle=True))):
        m, b = timed(call, a.reps)
        out.append("one page of %d x %d (the benchmark's page), %-36s %7.3f ms median (%7.3f min)" % (SIDE, SIDE, name + ":", m, b))
    out += ["",
            "Workspace per page pixel: 4 B of label, 4 B of area, 1 B of flag and 3 bits of masks, 9.4 B; 1 B more for the byte mask",
            "when it is asked for; per 64 x 64 tile a record of 256 B of counts; per page two histograms of 2 KB each.",
            "What a detector or a recogniser gains from a page without its specks is UNCALIBRATED here: the word counts of DESIGN.md",
            "7.9 are those of the synthetic detection file, which was not trained on text.",
            "NOT MEASURED by this run: a cold-cache rate, pages larger than the last-level cache, worst-case chains (a serpentine or",
            "a spiral that makes one component of the whole page, where the unions of pass 3 serialise on one root), parameters",
            "other than the two sets above.",
            "Static (cross-compiled for gfx950; VGPRs / SGPRs / LDS bytes; no scratch, no spills): speckle_mask_kernel 50 / 98 / 8192,",
            "speckle_levels_kernel 26 / 34 / 40, speckle_merge_kernel 20 / 51 / 0, speckle_area_kernel 24 / 28 / 0,",
            "speckle_big_kernel 14 / 34 / 0, speckle_near_kernel 20 / 44 / 512, speckle_map_kernel 70 / 72 / 0 (7 waves per SIMD),",
            "speckle_info_kernel 60 / 15 / 192; 8 waves per SIMD but for the one named."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
