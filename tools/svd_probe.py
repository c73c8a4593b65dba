"""Times PureSVD (cu2rec_model_svd) on the synthetic ML-20M shape: the call as a whole, and its stages as device times.

    python tools/svd_probe.py [--shapes ml-20m] [--factors 100] [--sweeps 2] [--reps 3] [--no-stages] [--out FILE]

Call times are wall clock around the synchronous call, best of --reps after one warm-up call (the warm-up builds the item-major view
and the two row plans, which the CSR keeps).  The stages are kernel times: a child process runs one warm-up and one timed call under
`rocprofv3 --kernel-trace`, and the second call's kernels are summed per stage.  The two products launch the same kernels, so they
are told apart by their order on the one stream: the products alternate X Q, X^T Y, ..., and end with P = X Q; every Gram, factor
and apply kernel belongs to the product before it.  A product's bytes are the algorithm's: entries x f x 4 gathered, plus the rows it
writes.  No time is a pass condition: there is no earlier PureSVD here to compare with."""
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

PRODUCT = ("svd_multiply", "svd_chunk", "svd_long_sum")
GRAM = ("als_chunk", "als_gram_sum", "cg_unpack_g0")
STAGES = ("product", "gram", "factor", "apply")


def best(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out)


def stage_times(shape, f, sweeps):
    """The second of two calls in a child under a kernel trace -> {(side, stage): [ms, kernels]}, side "X Q" or "X^T Y"; or a word on
    why not."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--shapes", shape, "--factors", str(f), "--sweeps", str(sweeps)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        except (OSError, subprocess.TimeoutExpired) as err:
            return "the traced child did not run: %s" % err
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if res.returncode != 0 or not traces:
            return "the traced child failed (%d): %s" % (res.returncode, res.stderr[-300:])
        with open(traces[0]) as fh:
            rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh))
    named = [(m.group(1), a, b) for m, a, b in ((re.search(r"\b(svd_\w+|als_\w+|cg_\w+)_kernel\b", n), a, b) for a, b, n in rows) if m]
    starts = [i for i, (n, _, _) in enumerate(named) if n == "svd_multiply"]
    per_call = 2 * sweeps + 1
    if len(starts) != 2 * per_call:
        return "expected %d products in the trace, found %d" % (2 * per_call, len(starts))
    out = {}
    product = -1
    for n, a, b in named[starts[per_call]:]:  # the second call
        if n == "svd_multiply":
            product += 1
        side = "X^T Y" if product % 2 else "X Q"
        stage = "product" if n in PRODUCT else "gram" if n in GRAM else "factor" if n == "svd_factor" else "apply" if n == "svd_apply" else None
        if stage is None:
            continue
        if stage == "product" and product == per_call - 1:
            side = "P = X Q"
        cell = out.setdefault((side, stage), [0.0, 0])
        cell[0] += (b - a) / 1e6
        cell[1] += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml-20m")
    ap.add_argument("--factors", type=int, default=100)
    ap.add_argument("--sweeps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-stages", action="store_true")
    ap.add_argument("--child", action="store_true", help="two calls and leave (what the kernel trace wraps)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    f, sweeps = args.factors, args.sweeps
    if args.child:
        tr, _ = synth.make_named(args.shapes)
        d = cu.DeviceCSR(tr)
        for _ in range(2):
            m = cu.Model(tr.rows, tr.cols, f, 0.0)
            m.svd(d, sweeps)
            m.close()
        return
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for name in args.shapes.split(","):
        tr, _ = synth.make_named(name)
        d = cu.DeviceCSR(tr)
        say("%s: %d users, %d items, %d entries; f = %d, %d sweeps" % (name, tr.rows, tr.cols, tr.nnz, f, sweeps))
        m = cu.Model(tr.rows, tr.cols, f, 0.0)
        rep = m.svd(d, sweeps)  # warm-up
        say("  captured / total after the warm-up's %d sweeps: %.6f" % (sweeps, rep["captured"] / rep["total"]))
        t_call = best(lambda: m.svd(d, sweeps), args.reps)
        t_one = best(lambda: m.svd(d, 1), args.reps)
        say("  svd, %d sweeps            %10.2f ms   (wall clock around the call, best of %d; with the final product, the two norms,"
            % (sweeps, 1e3 * t_call, args.reps))
        say("                                         the scratch buffers' allocation and the copy into the model)")
        say("  svd, 1 sweep             %10.2f ms   -> a sweep more costs %.2f ms" % (1e3 * t_one, 1e3 * (t_call - t_one) / max(sweeps - 1, 1)))
        t_proj = best(lambda: m.project(d), args.reps)
        say("  project, every row       %10.2f ms   (with the download of %d x %d floats)" % (1e3 * t_proj, tr.rows, f))
        if not args.no_stages:
            stages = stage_times(name, f, sweeps)
            if isinstance(stages, str):
                say("  stages: NOT MEASURED (%s)" % stages)
            else:
                ld_p, ld_q = f + (-f) % 4, f + (-f) % 32
                moved = {"X Q": 4.0 * tr.nnz * f + 4.0 * tr.rows * ld_p, "X^T Y": 4.0 * tr.nnz * f + 4.0 * tr.cols * ld_q}
                say("  kernel times of the second of two traced calls, per sweep (summed by kernel name, divided by the %d sweeps):" % sweeps)
                sweep_ms, orth_ms = 0.0, 0.0
                for side in ("X Q", "X^T Y"):
                    for stage in STAGES:
                        ms, count = stages.get((side, stage), (0.0, 0))
                        ms /= sweeps
                        sweep_ms += ms
                        orth_ms += ms if stage != "product" else 0.0
                        extra = ""
                        if stage == "product" and ms > 0:
                            extra = "   %.3g bytes (entries x f x 4 + the rows written): %.2f TB/s" % (moved[side], moved[side] / (ms * 1e-3) / 1e12)
                        say("    %-6s %-8s %9.3f ms in %4d kernels per call%s" % (side, stage, ms, count, extra))
                ms, count = stages.get(("P = X Q", "product"), (0.0, 0))
                say("    the final P = X Q   %9.3f ms in %4d kernels per call" % (ms, count))
                say("    a sweep: %.3f ms of kernels, of which orth (gram, factor, apply; both passes, both sides) %.3f ms = %.1f %%"
                    % (sweep_ms, orth_ms, 100.0 * orth_ms / sweep_ms if sweep_ms else 0.0))
        m.close()
        d.close()
    say("NOT MEASURED: cache hit rates, what bounds each stage (no counters were read), the once-per-CSR item-major view and row plans")
    say("(inside the warm-up), other f, sweeps or shapes, the host's share of a call beyond wall clock minus kernel time.")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
