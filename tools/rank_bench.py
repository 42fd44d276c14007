#!/usr/bin/env python
"""Cost of grain removal; writes profiles/rank_cost.txt.

    python tools/rank_bench.py [--reps R] [--out FILE]

1. The median at radii 1, 2, 3 and 7 with tail 0 and tail 20 on a batch of 16 grainy text pages of 1024 x 1024, per kernel,
   from one kernel trace: before it opens the GPU itself, the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rank_bench.py --only-kernel --reps R
   as a child, which launches nothing but R + 5 batches of every configuration in a fixed order and then as many of morph's
   thicken at every radius, and reads the per-launch durations from the trace in the order of their start (no counters in
   that run).  The medians are set beside two yardsticks of the same run: the time one read and one write of the float
   pages (8 B per pixel) take at the copy rate ocrs_device_measure_peaks reports, and thicken at the same radius.
2. OcrEngine.rank of one 1024 x 1024 page and get_text(rank=True) beside get_text on the same page: the median of R calls
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
RADII = (1, 2, 3, 7)
TAILS = (0, 20)
CONFIGS = [(r, t) for r in RADII for t in TAILS]
WARM = 5
RANK_KERNELS = ("rank_kernel", "rank_info_kernel")
MORPH_KERNELS = ("morph_rows_kernel", "morph_cols_kernel", "morph_info_kernel")
HOLDS = {1: "3 x 3 sorted in regs", 2: "5 x 5 sorted in regs", 3: "bisected in LDS", 7: "bisected in LDS"}


def grainy_page(seed, side):
    """A synthetic text page as a prepared page with 10 % salt and pepper."""
    import numpy as np
    from ocrs_amd import synth
    px = synth.synthetic_page(seed, side, side, 80, 2, 1)
    grey = (px.reshape(side, side).astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
    u = np.random.default_rng(seed).random(grey.shape)
    grey[u < 0.05] = np.float32(0.5)
    grey[(u >= 0.05) & (u < 0.10)] = np.float32(-0.5)
    return grey


def per_batch(reps):
    """traced's pick: (per configuration and kernel a batch's launch in us, sorted; per radius the same for thicken's kernels)."""
    def pick(found):
        batches = reps + WARM
        want = {name: len(CONFIGS) * batches for name in RANK_KERNELS}
        want.update({name: len(RADII) * batches for name in MORPH_KERNELS})
        for name, n in want.items():
            if len(found[name]) != n:
                return None, "the trace holds %d launches of %s, not %d" % (len(found[name]), name, n)
        per = {c: {name: sorted(found[name][i * batches + WARM:(i + 1) * batches]) for name in RANK_KERNELS} for i, c in enumerate(CONFIGS)}
        thick = {r: {name: sorted(found[name][i * batches + WARM:(i + 1) * batches]) for name in MORPH_KERNELS} for i, r in enumerate(RADII)}
        return (per, thick), None
    return pick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the batch loops, nothing written: what the kernel trace runs")
    a = ap.parse_args()

    # before this process opens the GPU
    trace, how = (None, None) if a.only_kernel else traced(__file__, [], a.reps, RANK_KERNELS + MORPH_KERNELS, "rank_prof_",
                                                           per_batch(a.reps), limit=400)
    per, thick = trace or (None, None)

    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, models, synth
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    batch = [eng.input_from_grey(grainy_page(i, SIDE)) for i in range(BATCH)]
    if a.only_kernel:
        for radius, tail in CONFIGS:
            for _ in range(a.reps + WARM):
                eng.rank_batch(batch, {"rx": radius, "ry": radius, "percent": 50, "tail": tail})
        for radius in RADII:
            for _ in range(a.reps + WARM):
                eng.morph_batch(batch, {"op": "thicken", "rx": radius, "ry": radius})
        print("%d batches of the median at radii %s with tails %s, and of thicken at the same radii" % (a.reps + WARM, RADII, TAILS))
        return
    _, copy_gbps = _lib.measure_peaks()
    pixels = BATCH * SIDE * SIDE
    total_mb = 8.0 * pixels / 1e6
    copy_us = total_mb / copy_gbps * 1e3
    out = ["Cost of grain removal (DESIGN.md 7.13).  Written by tools/rank_bench.py --reps %d on one MI355X; every figure below is" % a.reps,
           "MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of the calls,",
           "host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, "",
           "A batch of %d pages of %d x %d (synthetic text with 10 %% salt and pepper), one call per configuration, rx = ry, percent 50." % (BATCH, SIDE, SIDE),
           "First yardstick: one read and one write of the float pages are 8 B per pixel: %.0f MB, %.1f us at the copy rate.  The kernel" % (total_mb, copy_us),
           "moves little more (the halo of a 16 x 64 tile and the pixel's own word again, from cache) but selects: at radii 1 and 2 a",
           "sorting network of 28 and 140 compare-exchanges over the window in registers, above that 33 sweeps over the (2 r + 1)^2",
           "keys of the window in LDS, a compare and an add per key and sweep.  Second yardstick: morph's thicken (the percent-0",
           "filter by running minima, DESIGN.md 7.11) at the same radius in the same run, its three kernels summed."]
    if per is None:
        out += ["", "Per-kernel times: NOT MEASURED (%s)." % how]
    else:
        out += ["", "Per kernel, from one kernel trace (%d batches per configuration after %d warm-up batches), median us:" % (a.reps, WARM),
                "    " + how, "",
                "%6s %5s %-20s %12s %10s %10s %10s %10s %10s" % ("radius", "tail", "window held", "rank_kernel", "counts", "sum", "x copy", "thicken", "x thicken")]
        for radius, tail in CONFIGS:
            med = [statistics.median(per[(radius, tail)][name]) for name in RANK_KERNELS]
            th = sum(statistics.median(thick[radius][name]) for name in MORPH_KERNELS)
            out.append("%6d %5d %-20s %12.1f %10.1f %10.1f %10.2f %10.1f %10.2f" % (radius, tail, HOLDS[radius], med[0], med[1], sum(med), sum(med) / copy_us,
                                                                                  th, sum(med) / th))
        out.append("(reported, not required.)")
    out.append("")
    for radius, tail in ((1, 20), (2, 20), (7, 20)):
        med, best = timed(lambda: eng.rank_batch(batch, {"rx": radius, "percent": 50, "tail": tail}), a.reps)
        out.append("rank_batch of the %d pages, the median at radius %d with tail %d, host clock: %.3f ms median, %.3f ms min." % (BATCH, radius, tail, med, best))
    out.append("(%d result buffers and 3 workspace buffers from the pool, one upload, two launches (three for a batch that mixes radii above and up to 2), one wait.)" % BATCH)
    out.append("")
    out.append("The %d MB of source pages are touched again in every repetition and fit the 256 MB last-level cache: they were" % (4 * pixels // 1000000))
    out.append("CACHE-RESIDENT, so these are no HBM figures; a cold figure was NOT MEASURED.")
    out.append("")
    px = synth.synthetic_page(0, SIDE, SIDE, lines=80)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    for name, call in (("rank (median of 3 x 3, tail 20)", lambda: eng.rank(inp)),
                       ("rank(rx=2)", lambda: eng.rank(inp, rx=2)),
                       ("rank(rx=7)", lambda: eng.rank(inp, rx=7)),
                       ("rank(mask=True, info=True)", lambda: eng.rank(inp, mask=True, info=True)),
                       ("get_text", lambda: eng.get_text(inp)), ("get_text(rank=True)", lambda: eng.get_text(inp, rank=True))):
        m, b = timed(call, a.reps)
        out.append("one page of %d x %d (the benchmark's page), %-36s %7.3f ms median (%7.3f min)" % (SIDE, SIDE, name + ":", m, b))
    out += ["",
            "Workspace per page pixel: none but the result page; 1 B for the byte mask when it is asked for; per block (16 x 64",
            "pixels) a record of 40 B of counts.",
            "What a detector or a recogniser gains from a filtered page is UNCALIBRATED here: the synthetic model files were not",
            "trained on text.",
            "NOT MEASURED by this run: a cold-cache rate, pages larger than the last-level cache, rx != ry, percents other than 50,",
            "pages so small or so narrow that most lanes of a tile are off the page, a batch that mixes the classes, a 7 x 7 window",
            "sorted in registers (not built).",
            "Static (cross-compiled for gfx950; no scratch, no spills; both instantiations 9520 B of LDS: a staged region of 30 x 78",
            "keys and the block's counts): rank_kernel<true>, the 3 x 3 and 5 x 5 windows sorted in registers, 74 VGPRs, 61 SGPRs, 6",
            "waves per SIMD; rank_kernel<false>, the window bisected in LDS, 40 VGPRs, 52 SGPRs, 8 waves per SIMD; rank_info_kernel 25",
            "VGPRs, 160 B of LDS."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
