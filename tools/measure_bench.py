#!/usr/bin/env python
"""Cost of page measurement; writes profiles/measure_cost.txt.

    python tools/measure_bench.py [--reps R] [--out FILE]

1. The five passes on a batch of 16 noisy text pages of 1024 x 1024 (the pages of tools/despeckle_bench.py), per kernel, from
   a kernel trace of its own: before it opens the GPU itself, the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/measure_bench.py --only-kernel --op measure --reps R
   as a child, which launches nothing but R + 5 batches, and reads the per-launch durations from the trace.  Each pass is
   set beside the bytes it must move at the copy rate ocrs_device_measure_peaks reports in this run.
2. The same for despeckle_pages on the same pages (--op despeckle), the nearest existing neighbour: it shares the mask,
   merge and area / boxes passes.
3. OcrEngine.measure and text_scale of one page, and detect_words with and without work_text_height: the median of R calls
   after 5 warm-up calls, host clock around a call that ends in a device synchronise.

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
# kernel -> (bytes per pixel it must move at the least, what they are)
MEASURE = (("measure_mask_kernel", 4.125, "the page read once (4 B) and the bit mask written (1 bit); also 4 B of label per ink pixel and 16 B per in-word run"),
           ("measure_runs_kernel", 0.125, "the bit mask read once; each block also reads the 255 rows of words above its tile (5 x the mask in all)"),
           ("measure_merge_kernel", 0.125, "the bit mask read once; find / atomicMin unions on the labels of ink"),
           ("measure_boxes_kernel", 0.125, "the bit mask read once; a find per in-word run of ink, four atomics per series of consecutive runs of one root"),
           ("measure_components_kernel", 0.125, "the bit mask read once; a label read per in-word run, four words per root"))
SPECKLE = ("speckle_mask_kernel", "speckle_levels_kernel", "speckle_merge_kernel", "speckle_area_kernel", "speckle_big_kernel",
           "speckle_near_kernel", "speckle_map_kernel", "speckle_info_kernel")
SHARED = {"measure_mask_kernel": "speckle_mask_kernel", "measure_merge_kernel": "speckle_merge_kernel", "measure_boxes_kernel": "speckle_area_kernel"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the batch loop, nothing written: what the kernel trace runs")
    ap.add_argument("--op", choices=("measure", "despeckle"), default="measure", help="with --only-kernel: the call of the batch loop")
    a = ap.parse_args()

    # before this process opens the GPU
    traces = {} if a.only_kernel else {op: traced(__file__, ["--op", op], a.reps, names, "measure_prof_")
                                       for op, names in (("measure", [k[0] for k in MEASURE]), ("despeckle", list(SPECKLE)))}

    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, measure_choose, models, synth
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    batch = [eng.input_from_grey(noisy_page(i, SIDE)) for i in range(BATCH)]
    call = (lambda: eng.measure_batch(batch)) if a.op == "measure" else (lambda: eng.despeckle_batch(batch))
    if a.only_kernel:
        med, best = timed(call, a.reps)
        print("%s_batch of %d pages of %d x %d: %.3f ms median, %.3f ms min" % (a.op, BATCH, SIDE, SIDE, med, best))
        return
    _, copy_gbps = _lib.measure_peaks()
    pixels = BATCH * SIDE * SIDE
    infos = eng.measure_batch(batch)
    scales = [measure_choose(i) for i in infos]
    runs = sum(int(i["run_h"].sum()) for i in infos)
    out = ["Cost of page measurement (DESIGN.md 7.14).  Written by tools/measure_bench.py --reps %d on one MI355X; every figure" % a.reps,
           "below is MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of",
           "the calls, host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, "",
           "A batch of %d pages of %d x %d (synthetic text with pepper on %.1f %% and salt on %.1f %% of the pixels), one call:" % (
               BATCH, SIDE, SIDE, 100 * NOISE, 100 * NOISE),
           "%d pixels of ink in %d components, %d counted, %d horizontal runs; strokes %s, text heights %s." % (
               sum(i["ink"] for i in infos), sum(i["components"] for i in infos), sum(i["counted"] for i in infos), runs,
               sorted(set(s.stroke for s in scales)), sorted(set(s.text_height for s in scales))),
           "One read of the float pages is %.0f MB, %.1f us at the copy rate; the bit masks are %.1f MB." % (
               4.0 * pixels / 1e6, 4.0 * pixels / 1e6 / copy_gbps * 1e3, pixels / 8e6)]
    medians = {}
    for op, names in (("measure", [k[0] for k in MEASURE]), ("despeckle", list(SPECKLE))):
        trace, how = traces[op]
        out.append("")
        if trace is None:
            out.append("%s, per-kernel times: NOT MEASURED (%s)." % (op, how))
            continue
        out.append("%s, per kernel, from a kernel trace of its own (%d launches each):" % (op, len(trace[names[0]])))
        out.append("    " + how)
        total = 0.0
        for name in names:
            us = trace[name]
            m = statistics.median(us)
            medians[name] = m
            total += m
            line = "%-26s %8.1f us median, %8.1f min, %8.1f max" % (name, m, us[0], us[-1])
            for k, bpp, what in MEASURE:
                if k == name:
                    mb = bpp * pixels / 1e6
                    line += "; must move %.1f MB = %.1f us at the copy rate, %.0f GB/s at the median; %s" % (mb, mb / copy_gbps * 1e3, mb / m * 1e3, what)
            out.append(line)
        medians[op] = total
        out.append("sum of the medians: %.1f us" % total)
    if "measure" in medians and "despeckle" in medians:
        out.append("")
        out.append("measure / despeckle on the same pages: %.2f (sums of the medians).  The passes they share:" % (medians["measure"] / medians["despeckle"]))
        for mine, theirs in SHARED.items():
            out.append("    %-26s %8.1f us   beside %-22s %8.1f us" % (mine, medians[mine], theirs, medians[theirs]))
    out.append("")
    for op, fn in (("measure_batch", lambda: eng.measure_batch(batch)), ("despeckle_batch", lambda: eng.despeckle_batch(batch))):
        med, best = timed(fn, a.reps)
        out.append("%s of the %d pages, host clock: %.3f ms median, %.3f ms min" % (op, BATCH, med, best))
    out.append("(measure_batch: four workspace buffers from the pool, one upload, one memset of the records, five launches, one")
    out.append("download of %d x 6160 B, one wait, and the records turned into numpy arrays.)" % BATCH)
    out.append("")
    px = synth.synthetic_page(0, SIDE, SIDE, lines=80)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    for name, fn in (("measure", lambda: eng.measure(inp)), ("text_scale", lambda: eng.text_scale(inp)),
                     ("detect_words", lambda: eng.detect_words(inp)), ("detect_words(work_text_height=True)", lambda: eng.detect_words(inp, work_text_height=True)),
                     ("detect_words(work_text_height=28)", lambda: eng.detect_words(inp, work_text_height=28))):
        m, b = timed(fn, a.reps)
        out.append("one page of %d x %d (the benchmark's page), %-38s %7.3f ms median (%7.3f min)" % (SIDE, SIDE, name + ":", m, b))
    out += ["",
            "Workspace per page pixel: 4 B of label, 4 B of area and 3 x 4 B of box words, 20 B, and 1 bit of mask; per page a record",
            "of 6160 B.  Labels are written on ink alone and area and box words at the heads of in-word runs of ink alone, so most",
            "of the 20 B are never touched on a text page.",
            "Every block adds its histogram bins that are not zero to the page's record with one atomic each; there are no per-block",
            "records and no sixth pass.  What that costs beside per-block records was NOT MEASURED: the per-kernel figures above",
            "include it.",
            "The %d MB of source pages and the workspace are touched again in every repetition and fit the 256 MB last-level" % (4 * pixels // 1000000),
            "cache: they were CACHE-RESIDENT, so these are no HBM figures; a cold figure was NOT MEASURED.",
            "NOT MEASURED by this run: a cold-cache rate, pages larger than the last-level cache, worst-case chains (a serpentine or",
            "a spiral that makes one component of the whole page), a page of solid ink (where every vertical run is walked 254 rows",
            "up)."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
