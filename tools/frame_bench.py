#!/usr/bin/env python
"""Cost of page framing; writes profiles/frame_cost.txt.

    python tools/frame_bench.py [--reps R] [--out FILE]

1. The six passes of clean_frame on one bordered text page, per kernel, on the benchmark's 1024 x 1024 page and on an A4 page
   at 300 dpi (3508 x 2480), at depth 128 and at depth 0, each from a kernel trace of its own: before it opens the GPU itself,
   the tool starts
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/frame_bench.py --only-kernel --op OP --page P --depth D --reps R
   as a child, which launches nothing but R + 5 calls, and reads the per-launch durations from the trace.  The yardstick is
   despeckling (whose kernels this change leaves as they were) on the same pages, from traces of the same kind, beside the time
   of two reads and one write of the float page (12 B per pixel) at the copy rate ocrs_device_measure_peaks reports in this run.
2. ink_profiles and crop on the same pages, and OcrEngine.frame, host clock.
3. The detector's word counts on the bordered page before and after framing, on the synthetic models: uncalibrated.

No threshold gates anything here; the file says which figures were measured.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_util import timed, traced   # tools/, beside this file

PAGES = {"bench": (1024, 1024, 80), "a4": (3508, 2480, 200)}   # height, width, text lines
FRAME_KERNELS = ("frame_mask_kernel", "frame_levels_kernel", "frame_merge_kernel", "frame_area_kernel", "frame_map_kernel", "frame_info_kernel")
SPECKLE_KERNELS = ("speckle_mask_kernel", "speckle_levels_kernel", "speckle_merge_kernel", "speckle_area_kernel", "speckle_big_kernel",
                   "speckle_near_kernel", "speckle_map_kernel", "speckle_info_kernel")


def bordered_page(name):
    """A synthetic text page as a prepared page with a 9-pixel bar down the left, a 14-row wedge along the top and a 6-pixel
    slice of a neighbouring page down the right -> (page, the clean page)."""
    import numpy as np
    from ocrs_amd import synth
    h, w, lines = PAGES[name]
    px = synth.synthetic_page(3, h, w, lines, 2, 1)
    clean = (px.reshape(h, w).astype(np.float32) / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
    page = clean.copy()
    page[:, :9] = -0.45
    for y in range(14):
        page[y, 9:9 + (w - 22) * (14 - y) // 14] = -0.45
    page[1:h - 1, w - 6:] = -0.45
    return page, clean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the call loop, nothing written: what the kernel trace runs")
    ap.add_argument("--op", choices=("frame", "despeckle"), default="frame")
    ap.add_argument("--page", choices=tuple(PAGES), default="bench")
    ap.add_argument("--depth", type=int, default=128)
    a = ap.parse_args()

    # before this process opens the GPU
    traces = []
    if not a.only_kernel:
        for page in PAGES:
            for op, depth, kernels in (("frame", 128, FRAME_KERNELS), ("frame", 0, FRAME_KERNELS), ("despeckle", 0, SPECKLE_KERNELS)):
                traces.append((page, op, depth, kernels) + traced(__file__, ["--op", op, "--page", page, "--depth", str(depth)], a.reps, list(kernels),
                                                                  "frame_prof_"))

    from ocrs_amd import Model, OcrEngine, _lib, models
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    if a.only_kernel:
        inp = eng.input_from_grey(bordered_page(a.page)[0])
        call = (lambda: eng.clean_frame(inp, depth=a.depth)) if a.op == "frame" else (lambda: eng.despeckle(inp))
        med, best = timed(call, a.reps)
        print("%s of the %s page, depth %d: %.3f ms median, %.3f ms min" % (a.op, a.page, a.depth, med, best))
        return
    _, copy_gbps = _lib.measure_peaks()
    out = ["Cost of page framing (DESIGN.md 7.12).  Written by tools/frame_bench.py --reps %d on one MI355X; every figure below is" % a.reps,
           "MEASURED in that run unless its line says otherwise.  Host-clocked times are the median (and the minimum) of the calls,",
           "host clock around a call that ends in a device synchronise.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps]
    sums = {}
    for page, op, depth, kernels, trace, how in traces:
        h, w, _ = PAGES[page]
        copy_us = 12.0 * h * w / 1e6 / copy_gbps * 1e3
        out.append("")
        out.append("%s of one bordered text page of %d x %d%s; two reads and one write of the page: %.1f us at the copy rate." % (
            "clean_frame" if op == "frame" else "despeckle (the yardstick; default parameters)", h, w, ", depth %d" % depth if op == "frame" else "", copy_us))
        if trace is None:
            out.append("Per-kernel times: NOT MEASURED (%s)." % how)
            continue
        out.append("Per kernel, from a kernel trace of its own (%d launches each):" % len(trace[kernels[0]]))
        out.append("    " + how)
        total = 0.0
        for name in kernels:
            us = trace[name]
            m = statistics.median(us)
            total += m
            out.append("%-22s %8.1f us median, %8.1f min, %8.1f max" % (name, m, us[0], us[-1]))
        sums[(page, op, depth)] = total
        out.append("sum of the medians: %.1f us = %.1f x the time of two reads and one write at the copy rate (reported, not required)." % (
            total, total / copy_us))
    out.append("")
    for page in PAGES:
        d = sums.get((page, "despeckle", 0))
        for depth in (128, 0):
            f = sums.get((page, "frame", depth))
            if d is not None and f is not None:
                out.append("%s page, clean_frame at depth %d: %.2f x the sum of despeckling's passes (%.1f us against %.1f us)." % (page, depth, f / d, f, d))
    out.append("The pages and the workspaces are touched again in every repetition: they were CACHE-RESIDENT where they fit the 256 MB")
    out.append("last-level cache, so these are no HBM figures; a cold figure was NOT MEASURED.")
    out.append("")
    for page in PAGES:
        h, w, _ = PAGES[page]
        src, clean = bordered_page(page)
        inp = eng.input_from_grey(src)
        cleaned, info = eng.clean_frame(inp, info=True)
        for name, call in (("clean_frame (default parameters)", lambda: eng.clean_frame(inp)), ("clean_frame(depth=0)", lambda: eng.clean_frame(inp, depth=0)),
                           ("clean_frame(mask=True, info=True)", lambda: eng.clean_frame(inp, mask=True, info=True)),
                           ("despeckle (default parameters)", lambda: eng.despeckle(inp)),
                           ("ink_profiles", lambda: eng.ink_profiles(cleaned)), ("crop of the inner half", lambda: eng.crop(cleaned, (w // 4 + 1, h // 4, 3 * w // 4 + 1, 3 * h // 4))),
                           ("frame", lambda: eng.frame(inp))):
            m, b = timed(call, a.reps)
            out.append("one page of %d x %d, %-36s %7.3f ms median (%7.3f min)" % (h, w, name + ":", m, b))
        before, after = len(eng.detect_words(inp)), len(eng.detect_words(eng.frame(inp)[0]))
        plain = len(eng.detect_words(eng.input_from_grey(clean)))
        out.append("one page of %d x %d: %d components of %d pixels removed; words detected on the bordered page %d, on the framed page %d, on the" % (
            h, w, info["removed"], info["removed_pixels"], before, after))
        out.append("page without the planted border %d (synthetic detection file, not trained on text: UNCALIBRATED)." % plain)
    out += ["",
            "Workspace per page pixel: 4 B of label, 4 B of area, 1 B of flag and 1 bit of mask, allocated for the whole page and",
            "touched on the ink of the ring only; 1 B more for the byte mask when it is asked for; per 64 x 64 tile a record of 256 B of",
            "counts; per page a histogram of 2 KB.",
            "NOT MEASURED by this run: a cold-cache rate, batches, worst-case chains (a spiral that makes one component of the whole",
            "page at depth 0)."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
