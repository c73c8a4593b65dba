"""Times the softmax-matrix-factorization half-steps (cu2rec_model_softmax) on the synthetic ML-20M shape, per call and per kernel,
next to a logistic (cu2rec_model_lmf) sweep from the same run.

    python tools/softmax_probe.py [--shapes ml-20m] [--factors 100] [--reps 3] [--no-kernels] [--out FILE]

Call times are wall clock around the synchronous call (a half-step returns after a device-to-host read of its unchanged-row count),
best of --reps after one warm-up sweep of each trainer (it builds the item-major view and the accumulators).  The kernel times are
device times: a child process runs one warm-up sweep and --reps sweeps of softmax, then the same of lmf, under
`rocprofv3 --kernel-trace`; per kernel name the warm-up sweep's launches are dropped and the rest averaged per sweep.  The AdaGrad
step's kernel is launched by both trainers: its launches are split by their order on the one stream (softmax's sweeps come first).
By contraction count a softmax sweep is 4 scorings (the users' log-sum-exp before either half-step, and one per half-step) plus 2
pushes against lmf's 2 + 2, so 1.5 x an lmf sweep is what the arithmetic predicts.  No time is a pass condition."""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cu2rec_amd as cu  # noqa: E402
from cu2rec_amd import synth  # noqa: E402

HYPER = (0.05, 0.6, 0.6, 0.0, 0.6)
# kernel (as named in the trace, template arguments kept) -> launches per softmax sweep
SOFTMAX_KERNELS = {"softmax_weights": 2, "softmax_lse": 2, "softmax_dense<users>": 1, "softmax_dense<items>": 1,
                   "softmax_sparse<users>": 1, "softmax_sparse<items>": 1, "lmf_step": 2}
LMF_KERNELS = {"lmf_dense": 2, "lmf_sparse": 2, "lmf_step": 2}


def best(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def kernel_name(text):
    m = re.search(r"\b(softmax_\w+|lmf_\w+)_kernel(?:<([^>]*)>)?", text)
    if not m:
        return None
    name = m.group(1)
    if name in ("softmax_dense", "softmax_sparse"):  # the last template argument: the item side?
        last = (m.group(2) or "").split(",")[-1].strip()
        name += "<items>" if last.endswith("true") or last.endswith("1") else "<users>"
    return name


def kernel_times(shape, f, reps):
    """-> ({kernel: ms per softmax sweep}, {kernel: ms per lmf sweep}), or a word on why not."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--shapes", shape, "--factors", str(f), "--reps", str(reps)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        except (OSError, subprocess.TimeoutExpired) as err:
            return "the traced child did not run: %s" % err
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if res.returncode != 0 or not traces:
            return "the traced child failed (%d): %s" % (res.returncode, res.stderr[-300:])
        with open(traces[0]) as fh:
            rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh))
    by_name = {}
    for a, b, text in rows:
        name = kernel_name(text)
        if name:
            by_name.setdefault(name, []).append((b - a) / 1e6)
    steps = by_name.pop("lmf_step", [])
    if len(steps) != 4 * (1 + reps):
        return "expected %d AdaGrad steps in the trace, found %d" % (4 * (1 + reps), len(steps))
    out = ({}, {})
    for table, kernels, mine in ((out[0], SOFTMAX_KERNELS, steps[:2 * (1 + reps)]), (out[1], LMF_KERNELS, steps[2 * (1 + reps):])):
        for name, per_sweep in kernels.items():
            times = mine if name == "lmf_step" else by_name.get(name, [])
            if len(times) != per_sweep * (1 + reps):
                return "expected %d launches of %s in the trace, found %d" % (per_sweep * (1 + reps), name, len(times))
            table[name] = sum(times[per_sweep:]) / reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml-20m")
    ap.add_argument("--factors", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help="the sweeps and leave (what the kernel trace wraps)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    f = args.factors
    if args.child:
        tr, _ = synth.make_named(args.shapes)
        d = cu.DeviceCSR(tr)
        m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        m.softmax(d, HYPER, "both", sweeps=1 + args.reps)
        m.lmf_reset()
        m.lmf(d, HYPER, 1.0, "both", sweeps=1 + args.reps)
        return
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for name in args.shapes.split(","):
        tr, _ = synth.make_named(name)
        d = cu.DeviceCSR(tr)
        m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        scoring = 2.0 * tr.rows * tr.cols * f
        say("%s: %d users, %d items, %d entries, f = %d; one scoring or one push of every pair is %.2e flop" % (name, tr.rows, tr.cols, tr.nnz, f, scoring))
        m.softmax(d, HYPER, "both")  # warm-up: the item-major view, the accumulators, the kernels' first launches
        calls = [("softmax users", 3, lambda: m.softmax(d, HYPER, "users")), ("softmax items", 3, lambda: m.softmax(d, HYPER, "items")),
                 ("softmax sweep", 6, lambda: m.softmax(d, HYPER, "both")), ("softmax objective", 1, lambda: m.softmax_objective(d, HYPER)),
                 ("softmax lse (to the host)", 1, lambda: m.softmax_lse(d))]
        t = {}
        for label, passes, fn in calls:
            t[label] = best(fn, args.reps)
            say("  %-28s %9.2f ms   %d passes over every pair: %6.2f TFLOP/s" % (label, 1e3 * t[label], passes, passes * scoring / t[label] / 1e12))
        m.lmf_reset()
        m.lmf(d, HYPER, 1.0, "both")
        for label, passes, fn in (("lmf users", 2, lambda: m.lmf(d, HYPER, 1.0, "users")), ("lmf items", 2, lambda: m.lmf(d, HYPER, 1.0, "items")),
                                  ("lmf sweep", 4, lambda: m.lmf(d, HYPER, 1.0, "both"))):
            t[label] = best(fn, args.reps)
            say("  %-28s %9.2f ms   %d passes over every pair: %6.2f TFLOP/s" % (label, 1e3 * t[label], passes, passes * scoring / t[label] / 1e12))
        say("  a softmax sweep is %.2f x an lmf sweep by wall clock (the contraction count predicts 1.5)" % (t["softmax sweep"] / t["lmf sweep"]))
        if not args.no_kernels:
            got = kernel_times(name, f, args.reps)
            if isinstance(got, str):
                say("  kernels: NOT MEASURED (%s)" % got)
            else:
                for title, table in (("softmax", got[0]), ("lmf", got[1])):
                    say("  kernel times per %s sweep (a traced child; the warm-up sweep dropped, %d sweeps averaged):" % (title, args.reps))
                    for kernel, ms in table.items():
                        say("    %-26s %9.3f ms" % (kernel, ms))
                    say("    %-26s %9.3f ms" % ("the sweep's kernels", sum(table.values())))
                say("  a softmax sweep is %.2f x an lmf sweep by kernel time" % (sum(got[0].values()) / sum(got[1].values())))
        m.close()
        d.close()
    say("NOT MEASURED: what bounds each kernel (no counters were read), other f or shapes, real data, the once-per-CSR item-major view")
    say("(inside the warm-up), the host's share of a call beyond wall clock minus kernel time.")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
