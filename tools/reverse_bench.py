#!/usr/bin/env python
"""Cost of reverse-video repair; writes profiles/reverse_cost.txt.

    python tools/reverse_bench.py [--reps R] [--out FILE]

1. The nine passes on a batch of 16 noisy text pages of 1024 x 1024 (the pages of tools/measure_bench.py), each with a band
   of its lines planted in reverse video, and on one A4 page at 300 dpi (3508 x 2480) with such a band, per kernel, from a
   kernel trace of its own: before it opens the GPU itself, the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/reverse_bench.py --only-kernel --op OP --reps R
   as a child, which launches nothing but R + 5 batches, and reads the per-launch durations from the trace.
2. The same for measure_pages and despeckle_pages on the same sixteen pages (--op measure, --op despeckle): the yardsticks,
   since the repair is roughly one of each.
3. OcrEngine.unreverse_batch with and without the byte mask and the info, host clock around a call that ends in a device
   synchronise: the median of R calls after 5 warm-up calls.

No threshold gates anything here; the file says which figures were measured.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_util import timed, traced   # tools/, beside this file
from despeckle_bench import NOISE, noisy_page

BATCH, SIDE = 16, 1024
A4 = (3508, 2480)
# kernel -> (bytes per pixel it must move at the least, what they are)
REVERSE = (("reverse_mask_kernel", 4.125, "the page read once (4 B) and the ink mask written (1 bit); also 4 B of label per ink pixel and 16 B per in-word run"),
           ("reverse_merge_ink_kernel", 0.125, "the ink mask read once; find / atomicMin unions on the labels of ink"),
           ("reverse_boxes_kernel", 0.125, "the ink mask read once; a find per in-word run of ink, 4 B of label written per ink pixel, four atomics per series of runs of one root"),
           ("reverse_candidates_kernel", 0.25, "the ink mask read and the M mask written; four words per in-word run of ink, 4 B of label written per pixel outside M"),
           ("reverse_merge_rest_kernel", 0.125, "the M mask read once; find / atomicMin unions outside M; 8 B reset per in-word run"),
           ("reverse_rest_area_kernel", 0.125, "the M mask read once; a find per in-word run outside M, 4 B of label written per pixel outside M, an atomic per run"),
           ("reverse_holes_kernel", 0.125, "the M mask read once; a label per in-word run outside M"),
           ("reverse_map_kernel", 8.125, "the page read and written (8 B), the M mask read; up to five words per in-word run"),
           ("reverse_info_kernel", 0.0, "one block per page"))
MEASURE = ("measure_mask_kernel", "measure_runs_kernel", "measure_merge_kernel", "measure_boxes_kernel", "measure_components_kernel")
SPECKLE = ("speckle_mask_kernel", "speckle_levels_kernel", "speckle_merge_kernel", "speckle_area_kernel", "speckle_big_kernel",
           "speckle_near_kernel", "speckle_map_kernel", "speckle_info_kernel")
TWINS = (("reverse_mask_kernel", "measure", "measure_mask_kernel"), ("reverse_merge_ink_kernel", "measure", "measure_merge_kernel"),
         ("reverse_boxes_kernel", "measure", "measure_boxes_kernel"), ("reverse_merge_rest_kernel", "despeckle", "speckle_merge_kernel"),
         ("reverse_rest_area_kernel", "despeckle", "speckle_area_kernel"), ("reverse_map_kernel", "despeckle", "speckle_map_kernel"))


def with_band(page):
    """The page with the middle third of its rows, but for a margin of 1/16 of its width, in reverse video."""
    import numpy as np
    h, w = page.shape
    page = page.copy()
    page.view(np.uint32)[h // 3:2 * h // 3, w // 16:w - w // 16] ^= np.uint32(0x80000000)
    return page


def a4_page():
    import numpy as np
    from ocrs_amd import synth
    h, w = A4
    px = synth.synthetic_page(7, h, w, 240, 2, 1)
    return with_band((px.reshape(h, w).astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reverse_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the batch loop, nothing written: what the kernel trace runs")
    ap.add_argument("--op", choices=("unreverse", "unreverse_a4", "measure", "despeckle"), default="unreverse", help="with --only-kernel: the call of the batch loop")
    a = ap.parse_args()

    ops = (("unreverse", [k[0] for k in REVERSE]), ("unreverse_a4", [k[0] for k in REVERSE]), ("measure", list(MEASURE)), ("despeckle", list(SPECKLE)))
    # before this process opens the GPU
    traces = {} if a.only_kernel else {op: traced(__file__, ["--op", op], a.reps, names, "reverse_prof_") for op, names in ops}

    from ocrs_amd import Model, OcrEngine, _lib, models
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    if a.only_kernel and a.op == "unreverse_a4":
        batch = [eng.input_from_grey(a4_page())]
    else:
        batch = [eng.input_from_grey(with_band(noisy_page(i, SIDE))) for i in range(BATCH)]
    calls = {"unreverse": lambda: eng.unreverse_batch(batch), "unreverse_a4": lambda: eng.unreverse_batch(batch),
             "measure": lambda: eng.measure_batch(batch), "despeckle": lambda: eng.despeckle_batch(batch)}
    if a.only_kernel:
        med, best = timed(calls[a.op], a.reps)
        print("%s of %d pages: %.3f ms median, %.3f ms min" % (a.op, len(batch), med, best))
        return
    _, copy_gbps = _lib.measure_peaks()
    big = [eng.input_from_grey(a4_page())]
    infos = eng.unreverse_batch(batch, info=True)[1]
    big_info = eng.unreverse_batch(big, info=True)[1][0]
    out = ["Cost of reverse-video repair (DESIGN.md 7.15).  Written by tools/reverse_bench.py --reps %d on one MI355X; every figure" % a.reps,
           "below is MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of",
           "the calls, host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, "",
           "A batch of %d pages of %d x %d (synthetic text with pepper on %.1f %% and salt on %.1f %% of the pixels, the middle third of the" % (
               BATCH, SIDE, SIDE, 100 * NOISE, 100 * NOISE),
           "rows in reverse video), one call at the default parameters (uncalibrated): %d pixels of ink in %d components, %d candidates," % (
               sum(i["ink"] for i in infos), sum(i["components"] for i in infos), sum(i["candidates"] for i in infos)),
           "%d panels of %d pixels with %d holes of %d pixels; %d pixels inverted." % (
               sum(i["panels"] for i in infos), sum(i["panel_pixels"] for i in infos), sum(i["holes"] for i in infos),
               sum(i["hole_pixels"] for i in infos), sum(i["inverted"] for i in infos)),
           "One A4 page at 300 dpi, %d x %d, with such a band: %d pixels of ink in %d components, %d candidates, %d panels, %d holes," % (
               A4[0], A4[1], big_info["ink"], big_info["components"], big_info["candidates"], big_info["panels"], big_info["holes"]),
           "%d pixels inverted." % big_info["inverted"]]
    medians = {}
    for op, names in ops:
        trace, how = traces[op]
        pixels = A4[0] * A4[1] if op == "unreverse_a4" else BATCH * SIDE * SIDE
        out.append("")
        if trace is None:
            out.append("%s, per-kernel times: NOT MEASURED (%s)." % (op, how))
            continue
        out.append("%s (%s), per kernel, from a kernel trace of its own (%d launches each):" % (
            op, "the A4 page" if op == "unreverse_a4" else "the %d pages" % BATCH, len(trace[names[0]])))
        out.append("    " + how)
        out.append("    one read of the float pages is %.1f MB, %.1f us at the copy rate" % (4.0 * pixels / 1e6, 4.0 * pixels / 1e6 / copy_gbps * 1e3))
        total = 0.0
        for name in names:
            us = trace[name]
            m = statistics.median(us)
            medians[(op, name)] = m
            total += m
            line = "%-26s %8.1f us median, %8.1f min, %8.1f max" % (name, m, us[0], us[-1])
            for k, bpp, what in REVERSE:
                if k == name and op.startswith("unreverse"):
                    mb = bpp * pixels / 1e6
                    line += "; must move %.1f MB = %.1f us at the copy rate; %s" % (mb, mb / copy_gbps * 1e3, what)
            out.append(line)
        medians[op] = total
        out.append("sum of the medians: %.1f us" % total)
    if all(op in medians for op in ("unreverse", "measure", "despeckle")):
        out.append("")
        out.append("unreverse / (measure + despeckle) on the same sixteen pages: %.2f (sums of the medians: %.1f, %.1f and %.1f us)." % (
            medians["unreverse"] / (medians["measure"] + medians["despeckle"]), medians["unreverse"], medians["measure"], medians["despeckle"]))
        out.append("Each pass beside its twin:")
        for mine, op, theirs in TWINS:
            out.append("    %-26s %8.1f us   beside %-22s %8.1f us   (%.2f)" % (
                mine, medians[("unreverse", mine)], theirs, medians[(op, theirs)], medians[("unreverse", mine)] / medians[(op, theirs)]))
        out.append("(The twins do not do the same work: the second labelling covers everything outside M, which on these pages is the")
        out.append("paper and all the ink of the text, where despeckle's forest holds both classes and measure's the ink alone.)")
    out.append("")
    for what, fn in (("unreverse_batch", lambda: eng.unreverse_batch(batch)), ("unreverse_batch(info=True)", lambda: eng.unreverse_batch(batch, info=True)),
                     ("unreverse_batch(mask=True)", lambda: eng.unreverse_batch(batch, mask=True)),
                     ("unreverse_batch(mask=True, info=True)", lambda: eng.unreverse_batch(batch, mask=True, info=True)),
                     ("measure_batch", lambda: eng.measure_batch(batch)), ("despeckle_batch", lambda: eng.despeckle_batch(batch))):
        med, best = timed(fn, a.reps)
        out.append("%-40s of the %d pages, host clock: %.3f ms median, %.3f ms min" % (what, BATCH, med, best))
    for what, fn in (("unreverse", lambda: eng.unreverse_batch(big)), ("unreverse(mask=True, info=True)", lambda: eng.unreverse_batch(big, mask=True, info=True))):
        med, best = timed(fn, a.reps)
        out.append("%-40s of the A4 page, host clock: %.3f ms median, %.3f ms min" % (what, med, best))
    out += ["(With mask=True every page's byte mask, 1 B a pixel, is downloaded and copied into a numpy array.)",
            "",
            "Workspace per page pixel: 4 B of label, 4 B of area and 3 x 4 B of box words, 20 B, and 2 bits of masks; per 64 x 64 tile a",
            "record of 256 B; per page a record of 72 B.",
            "The source pages and the workspace are touched again in every repetition; the sixteen pages (%d MB of floats, %d MB of" % (
                4 * BATCH * SIDE * SIDE // 1000000, 20 * BATCH * SIDE * SIDE // 1000000),
            "workspace) do not all fit the 256 MB last-level cache together with the result pages, the A4 page (%d MB and %d MB) does:" % (
                4 * A4[0] * A4[1] // 1000000, 20 * A4[0] * A4[1] // 1000000),
            "how much of either was cache-resident was NOT MEASURED, so these are no HBM figures.",
            "NOT MEASURED by this run: a cold-cache rate, pages beyond the last-level cache, worst-case chains (a serpentine or a",
            "spiral that makes one component of the whole page), counters."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
