"""What the tools/*_bench.py cost tools share: the host-clocked loop, and the kernel trace a tool takes of itself.

A tool traces itself by starting `rocprofv3 ... -- python tools/<tool> --only-kernel ...` as a child BEFORE it opens the GPU
itself (traced), and reads the per-launch durations from what the child left (kernel_launches, kernel_durations).  A kernel
is asked for by its name, or by (name, spellings) where a trace may spell it in several ways, as it does a template's.
"""
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time


def timed(call, reps, warm=5):
    """-> (median, minimum) in ms of `reps` calls after `warm` warm-up calls, host clock around each call."""
    for _ in range(warm):
        call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), min(times)


def kernel_launches(trace_dir, kernels):
    """kernel -> per-launch durations in us in the order of their start, from a rocprofv3 output directory (kernel-trace
    CSV, or the rocpd database)."""
    import sqlite3
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += [(r.get("Kernel_Name", ""), int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    if not rows:
        for path in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
            db = sqlite3.connect(path)
            tables = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
            kd = [t for t in tables if t.startswith("rocpd_kernel_dispatch")][0]
            ks = [t for t in tables if t.startswith("rocpd_info_kernel_symbol")][0]
            scols = [r[1] for r in db.execute("pragma table_info(%s)" % ks)]
            name_col = "kernel_name" if "kernel_name" in scols else "display_name"
            rows += list(db.execute("select s.%s, d.start, d.end from %s d join %s s on d.kernel_id = s.id" % (name_col, kd, ks)))
    rows.sort(key=lambda r: r[1])
    out = {}
    for k in kernels:
        name, spellings = (k, (k,)) if isinstance(k, str) else k
        out[name] = [(en - st) / 1e3 for n, st, en in rows if any(s in n for s in spellings)]
    return out


def kernel_durations(trace_dir, kernels):
    """kernel -> sorted per-launch durations in us (kernel_launches, sorted)."""
    return {name: sorted(us) for name, us in kernel_launches(trace_dir, kernels).items()}


def last_launches(kernels, want):
    """traced's pick: the last `want` launches of every kernel, in launch order (the launches before them set the pages up)."""
    def pick(found):
        found = {name: found[name][-want:] for name in kernels}
        if not all(len(found[name]) == want for name in kernels):
            return None, "the trace holds %s launches, not %d each" % (", ".join("%d of %s" % (len(found[n]), n) for n in kernels), want)
        return found, None
    return pick


def traced(script, extra_args, reps, kernels, tmp_prefix, pick=None, limit=300):
    """Runs `script --only-kernel <extra_args> --reps <reps>` under rocprofv3 in a child process -> (kernel -> sorted
    durations, the command) or (None, why not).  Every kernel must have been launched.  pick(launches), if given, takes
    kernel_launches' result instead and returns (what traced returns first, None) or (None, why not)."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 was not found"
    tmp = tempfile.mkdtemp(prefix=tmp_prefix)
    args = ["--only-kernel"] + list(extra_args) + ["--reps", str(reps)]
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(script)] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            return None, "the traced run ended with status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-300:].replace("\n", " | "))
        found = kernel_launches(tmp, kernels)
        if pick:
            found, why = pick(found)
            if found is None:
                return None, why
        else:
            if not all(found.values()):
                return None, "the trace holds no launches of %s" % ", ".join(n for n in found if not found[n])
            found = {name: sorted(us) for name, us in found.items()}
        return found, " ".join(["rocprofv3"] + cmd[1:5] + ["-d", "DIR", "--", "python", "tools/" + os.path.basename(script)] + args)
    except subprocess.TimeoutExpired:
        return None, "the traced run did not end within %d s" % limit
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
