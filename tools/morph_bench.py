#!/usr/bin/env python
"""Cost of stroke repair; writes profiles/morph_cost.txt.

    python tools/morph_bench.py [--reps R] [--out FILE]

1. Every op at radii 1, 7 and 63 on a batch of 16 damaged text pages of 1024 x 1024, per kernel, from one kernel trace:
   before it opens the GPU itself, the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/morph_bench.py --only-kernel --reps R
   as a child, which launches nothing but R + 5 batches of every configuration in a fixed order and then as many of
   binarize at radius 15, and reads the per-launch durations from the trace in the order of their start (no counters in
   that run).  The medians are set beside two yardsticks of the same run: the time one read and one write of the float
   pages (8 B per pixel) take at the copy rate ocrs_device_measure_peaks reports, and binarize at radius 15.
2. OcrEngine.morph of one 1024 x 1024 page and get_text(morph=True) beside get_text on the same page: the median of R calls
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

BATCH, SIDE = 16, 1024
OPS = ("thicken", "thin", "close", "open")
STAGES = {"thicken": 1, "thin": 1, "close": 2, "open": 2}
RADII = (1, 7, 63)
CONFIGS = [(op, r) for op in OPS for r in RADII]
WARM = 5
MORPH_KERNELS = ("morph_rows_kernel", "morph_cols_kernel", "morph_info_kernel")
BIN_KERNELS = ("bin_rows_kernel", "bin_cols_kernel", "bin_info_kernel")


def damaged_page(seed, side):
    """A synthetic text page as a prepared page with 30 % of its ink pixels turned to paper."""
    import numpy as np
    from ocrs_amd import synth
    px = synth.synthetic_page(seed, side, side, 80, 2, 1)
    grey = (px.reshape(side, side).astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
    grey[(grey < 0) & (np.random.default_rng(seed).random(grey.shape) < 0.3)] = np.float32(0.5)
    return grey


def per_batch(reps):
    """traced's pick: (per configuration and kernel the sum of a batch's launches in us, one per batch; the same for binarize)."""
    def pick(found):
        batches = reps + WARM
        want = {"morph_rows_kernel": sum(STAGES[op] for op, _ in CONFIGS) * batches, "morph_cols_kernel": sum(STAGES[op] for op, _ in CONFIGS) * batches,
                "morph_info_kernel": len(CONFIGS) * batches}
        want.update({name: batches for name in BIN_KERNELS})
        for name, n in want.items():
            if len(found[name]) != n:
                return None, "the trace holds %d launches of %s, not %d" % (len(found[name]), name, n)
        per = {}
        at = dict.fromkeys(MORPH_KERNELS, 0)
        for op, radius in CONFIGS:
            per[(op, radius)] = {}
            for name in MORPH_KERNELS:
                k = 1 if name == "morph_info_kernel" else STAGES[op]   # launches of a batch
                us = found[name][at[name]:at[name] + k * batches]
                at[name] += k * batches
                per[(op, radius)][name] = sorted(sum(us[i * k:(i + 1) * k]) for i in range(WARM, batches))
        bins = {name: sorted(found[name][WARM:]) for name in BIN_KERNELS}
        return (per, bins), None
    return pick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the batch loops, nothing written: what the kernel trace runs")
    a = ap.parse_args()

    # before this process opens the GPU
    trace, how = (None, None) if a.only_kernel else traced(__file__, [], a.reps, MORPH_KERNELS + BIN_KERNELS, "morph_prof_",
                                                           per_batch(a.reps), limit=400)
    per, bins = trace or (None, None)

    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, models, synth
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    batch = [eng.input_from_grey(damaged_page(i, SIDE)) for i in range(BATCH)]
    if a.only_kernel:
        for op, radius in CONFIGS:
            for _ in range(a.reps + WARM):
                eng.morph_batch(batch, {"op": op, "rx": radius, "ry": radius})
        for _ in range(a.reps + WARM):
            eng.binarize_batch(batch, {"radius": 15})
        print("%d batches of every op at radii %s, and of binarize at radius 15" % (a.reps + WARM, RADII))
        return
    _, copy_gbps = _lib.measure_peaks()
    pixels = BATCH * SIDE * SIDE
    total_mb = 8.0 * pixels / 1e6
    copy_us = total_mb / copy_gbps * 1e3
    out = ["Cost of stroke repair (DESIGN.md 7.11).  Written by tools/morph_bench.py --reps %d on one MI355X; every figure below is" % a.reps,
           "MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of the calls,",
           "host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, "",
           "A batch of %d pages of %d x %d (synthetic text with 30 %% of its ink pixels lost), one call per configuration, rx = ry." % (BATCH, SIDE, SIDE),
           "The floor: one read and one write of the float pages are 8 B per pixel: %.0f MB, %.1f us at the copy rate.  A stage moves" % (total_mb, copy_us),
           "more than that: its horizontal pass reads the page (4 B, and 2 rx of every 256 + 2 rx pixels again as halo) and writes",
           "the keys (4 B); its vertical pass reads the keys (4 B, and 2 ry rows of run-in per segment again) and the source word",
           "(4 B) and writes the page (4 B): 20 B per pixel and stage without halo and run-in."]
    if per is None:
        out += ["", "Per-kernel times: NOT MEASURED (%s)." % how]
    else:
        out += ["", "Per kernel, from one kernel trace (%d batches per configuration after %d warm-up batches; a batch's launches of a" % (a.reps, WARM),
                "kernel summed: close and open launch the two passes twice), median us:", "    " + how, "",
                "%-8s %6s %12s %12s %12s %10s %10s" % ("op", "radius", "rows passes", "cols passes", "counts", "sum", "x floor")]
        total = {}
        for op, radius in CONFIGS:
            med = [statistics.median(per[(op, radius)][name]) for name in MORPH_KERNELS]
            total[(op, radius)] = sum(med)
            out.append("%-8s %6d %12.1f %12.1f %12.1f %10.1f %10.2f" % (op, radius, med[0], med[1], med[2], sum(med), sum(med) / copy_us))
        bmed = [statistics.median(bins[name]) for name in BIN_KERNELS]
        out.append("%-8s %6d %12.1f %12.1f %12.1f %10.1f %10.2f   (the sibling of DESIGN.md 7.10: 32 B per pixel)" % (
            "binarize", 15, bmed[0], bmed[1], bmed[2], sum(bmed), sum(bmed) / copy_us))
        out.append("")
        for op in OPS:
            out.append("%-8s radius 63 / radius 1: %.2f; radius 7 / radius 1: %.2f; radius 1 / binarize: %.2f; radius 63 / binarize: %.2f" % (
                op, total[(op, 63)] / total[(op, 1)], total[(op, 7)] / total[(op, 1)], total[(op, 1)] / sum(bmed), total[(op, 63)] / sum(bmed)))
        out.append("(reported, not required.)")
    out.append("")
    for op, radius in (("close", 1), ("close", 63), ("thicken", 1)):
        med, best = timed(lambda: eng.morph_batch(batch, {"op": op, "rx": radius, "ry": radius}), a.reps)
        out.append("morph_batch of the %d pages, %s at radius %d, host clock: %.3f ms median, %.3f ms min." % (BATCH, op, radius, med, best))
    out.append("(%d result buffers and up to %d workspace buffers from the pool, one upload, three or five launches, one wait.)" % (BATCH, 2 * BATCH + 3))
    out.append("")
    out.append("The %d MB of source pages and the %d MB of keys are touched again in every repetition and fit the 256 MB last-level" % (
        4 * pixels // 1000000, 4 * pixels // 1000000))
    out.append("cache: they were CACHE-RESIDENT, so these are no HBM figures; a cold figure was NOT MEASURED.")
    out.append("")
    px = synth.synthetic_page(0, SIDE, SIDE, lines=80)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    for name, call in (("morph (close at radius 1)", lambda: eng.morph(inp)),
                       ("morph(op='close', rx=63)", lambda: eng.morph(inp, rx=63)),
                       ("morph(op='thicken', rx=1, ry=0)", lambda: eng.morph(inp, op="thicken", rx=1, ry=0)),
                       ("morph(mask=True, info=True)", lambda: eng.morph(inp, mask=True, info=True)),
                       ("get_text", lambda: eng.get_text(inp)), ("get_text(morph=True)", lambda: eng.get_text(inp, morph=True))):
        m, b = timed(call, a.reps)
        out.append("one page of %d x %d (the benchmark's page), %-36s %7.3f ms median (%7.3f min)" % (SIDE, SIDE, name + ":", m, b))
    out += ["",
            "Workspace per page pixel: 4 B of keys; 4 B more for the page between the stages of close and open; 1 B more for the byte",
            "mask when it is asked for; per block of a vertical pass a record of 32 B of counts.",
            "What a detector or a recogniser gains from a repaired page is UNCALIBRATED here: the synthetic model files were not",
            "trained on text.",
            "NOT MEASURED by this run: a cold-cache rate, pages larger than the last-level cache, rx != ry, pages so small or so narrow",
            "that most lanes of a strip are off the page, both passes of a stage fused over LDS tiles (not built).",
            "Static (cross-compiled for gfx950; VGPRs / LDS bytes; no scratch, no spills): morph_rows_kernel 21 / 6144, morph_cols_kernel",
            "40 / 3840 (ry <= 7), 42 / 16128 (ry <= 31), 42 / 32512 (ry <= 63: four one-wave blocks per CU by its LDS), morph_info_kernel",
            "23 / 128.  Segments of the vertical pass on these pages (morph_seg_rows): 64 rows at ry = 1, 61 at ry = 7, 128 at ry = 63."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
