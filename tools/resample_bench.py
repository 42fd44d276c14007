#!/usr/bin/env python
"""Cost of page resampling and of detection at a working resolution; writes profiles/resample_cost.txt.

    python tools/resample_bench.py [--reps R] [--out FILE]
    rocprofv3 --kernel-trace --stats -d resample_prof -- python tools/resample_bench.py --only-kernel --reps 50
    python tools/resample_bench.py --append-trace resample_prof [--out FILE]
                                (the kernel's own time: the first run launches nothing but the two shapes below, one loop after the other;
                                 the second reads the trace's per-launch durations and appends them to the file)

1. OcrEngine.resize per page at 3508 x 2480 -> 1754 x 1240 (area, a 2 x 2 box) and 1024 x 1024 -> 1536 x 1536 (bilinear):
   the median of R calls after 5 warm-up calls, host clock around a call that ends in a device synchronise.  A call is: the
   new page's buffer from the pool, 56 B of descriptor uploaded, one launch, one wait, so it is launch-and-wait latency as
   much as traffic.  Bytes moved are 4 per source pixel plus 4 per result pixel, held against the copy rate
   ocrs_device_measure_peaks reports in the same run.
2. detect_words(work_size=half) beside the plain and the tiled call on an A4-sized synthetic page (3508 x 2480), the same way.

No threshold gates anything here; the file says which figures were measured.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_util import kernel_launches, timed   # tools/, beside this file

SHAPES = (((3508, 2480), (1754, 1240), "area"), ((1024, 1024), (1536, 1536), "bilinear"))
KERNEL = "resample_pages_kernel"


def moved_bytes(src, dst):
    return 4.0 * (src[0] * src[1] + dst[0] * dst[1])


def append_trace(trace_dir, out):
    """Per-launch durations of the kernel from a kernel trace of --only-kernel, which runs the loop of SHAPES[0] to its end
    and then that of SHAPES[1], the same number of launches each: the first half of the launches is the one, the second
    half the other."""
    launches = kernel_launches(trace_dir, [KERNEL])[KERNEL]   # us, in the order of their start
    if not launches or len(launches) % len(SHAPES):
        raise SystemExit("%d launches of %s under %s: expected the same number per shape" % (len(launches), KERNEL, trace_dir))
    per = len(launches) // len(SHAPES)
    lines = ["", "Appended by tools/resample_bench.py --append-trace, MEASURED in a run of its own on one MI355X:",
             "    rocprofv3 --kernel-trace --stats -d resample_prof -- python tools/resample_bench.py --only-kernel --reps %d" % (per - 5)]
    for i, (src, dst, filt) in enumerate(SHAPES):
        us = sorted(launches[i * per:(i + 1) * per])
        mb = moved_bytes(src, dst) / 1e6
        med = statistics.median(us)
        lines.append("%s, %s %d x %d -> %d x %d, %d launches: %.1f us median, %.1f us minimum, %.1f us maximum per launch; %.1f MB "
                     "moved = %.0f GB/s at the median." % ((KERNEL, filt) + src + dst + (len(us), med, us[0], us[-1], mb, mb / med * 1e3)))
    lines.append("The source is read again in every repetition and fits the 256 MB last-level cache, so these are no HBM figures; a "
                 "cold figure was NOT MEASURED.")
    with open(out, "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_cost.txt"))
    ap.add_argument("--only-kernel", action="store_true", help="only the resize loops, nothing written: for a kernel trace")
    ap.add_argument("--append-trace", metavar="DIR", help="append the kernel's per-launch times from a rocprofv3 output directory")
    a = ap.parse_args()
    if a.append_trace:
        return append_trace(a.append_trace, a.out)

    import numpy as np

    from ocrs_amd import DimOrder, ImageSource, Model, OcrEngine, _lib, models, synth, work_size
    _lib.require_gpu()
    eng = OcrEngine(detection_model=Model.load_bytes(models.synthetic_detection_bytes()),
                    recognition_model=Model.load_bytes(models.synthetic_recognition_bytes()))
    rng = np.random.default_rng(0)
    pages = [eng.input_from_grey(rng.random(src, dtype=np.float32) - np.float32(0.5)) for src, _, _ in SHAPES]
    if a.only_kernel:
        for inp, (src, dst, filt) in zip(pages, SHAPES):
            print("resize %s %s -> %s: %.3f ms median, %.3f ms min" % ((filt, src, dst) + timed(lambda: eng.resize(inp, dst, filt), a.reps)))
        return
    _, copy_gbps = _lib.measure_peaks()
    out = ["Cost of page resampling and of detection at a working resolution (DESIGN.md 7.3).  Written by tools/resample_bench.py",
           "--reps %d on one MI355X; every figure below is MEASURED in that run unless its line says otherwise.  Times are the" % a.reps,
           "median (and the minimum) of the calls, host clock around a call that ends in a device synchronise.  A resize call is:",
           "buffer from the pool, descriptor upload, one launch, one wait.  Bytes moved: 4 per source pixel + 4 per result pixel.",
           "Copy rate of this run (ocrs_device_measure_peaks): %.0f GB/s." % copy_gbps, ""]
    for inp, (src, dst, filt) in zip(pages, SHAPES):
        med, best = timed(lambda: eng.resize(inp, dst, filt), a.reps)
        gb = moved_bytes(src, dst) / 1e9
        out.append("resize %-8s %4d x %4d -> %4d x %4d: %7.3f ms median, %7.3f ms min; %.1f MB moved: %6.0f GB/s at the median, %6.0f "
                   "at the minimum (%.0f %% / %.0f %% of the copy rate)"
                   % ((filt,) + src + dst + (med, best, gb * 1e3, gb / med * 1e3, gb / best * 1e3, 100 * gb / med * 1e3 / copy_gbps,
                                            100 * gb / best * 1e3 / copy_gbps)))
    out.append("")
    px = synth.synthetic_page(13, 3508, 2480, lines=200, columns=2)
    inp = eng.prepare_input(ImageSource.from_tensor(px, DimOrder.Hwc))
    half = work_size((3508, 2480), scale=0.5)
    reps = max(5, a.reps // 5)
    for name, call in (("plain (one squeeze to 800 x 600)", lambda: eng.detect_words(inp)),
                       ("work_size=%d x %d (area), untiled" % half, lambda: eng.detect_words(inp, work_size=half)),
                       ("work_size=%d x %d (area), tiled" % half, lambda: eng.detect_words(inp, work_size=half, tiled=True)),
                       ("tiled at full size (25 tiles)", lambda: eng.detect_words(inp, tiled=True))):
        med, best = timed(call, reps)
        out.append("detect_words on 3508 x 2480, %-40s %7.2f ms median (%7.2f min), %4d words" % (name + ":", med, best, len(call())))
    out += ["",
            "The word counts are those of the synthetic detector, which was not trained on text and is not scale-sensitive: they",
            "say that the scheme is sane, not what a trained detector gains from a working resolution.  That gain is",
            "UNCALIBRATED here (DESIGN.md 7.3).",
            "NOT MEASURED by this run: the kernel's own time without the call around it (a kernel trace of --only-kernel, appended",
            "below by --append-trace when it was taken), a cold-cache rate, bench.py against the parent commit (recorded in",
            "DESIGN.md 7.3 when it was run).",
            "Static (cross-compiled for gfx950): resample_pages_kernel 26 VGPRs, 29 SGPRs, no LDS, no scratch, no spills,",
            "occupancy 8 waves per SIMD."]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
